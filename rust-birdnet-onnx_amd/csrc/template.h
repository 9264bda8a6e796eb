// The kernel of bn_recording_template_match (template.hip), launched by recording.cpp: the Pearson correlation of every template
// of a packed set (template_plan.h) with a U8 code image on the device at every frame offset, exact integer sums on the i8 matrix
// pipe.  The image is what launch_spectrogram wrote (spectrogram.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "template_plan.h"

namespace bn {

// The opt-in of the kernels to more than 64 KiB of LDS on `device`: once per device, before the first launch there that needs it,
// never during a capture (LdsOptIn, capi_internal.h)
hipError_t template_match_prepare(int device);

// What a launch needs of a packed set on the device
struct TemplateSet {
    const void *image;          // the fragments, 16-byte aligned
    const tmatch::Meta *meta;   // [16 * n_tiles]
    tmatch::Tiles tiles;
    uint32_t n_templates, n_rows, n_tiles, max_frames;
};

// out [set.n_templates][n_offsets] floats <- the scores of offsets 0 .. n_offsets - 1 over image [n_image_frames][set.n_rows]
// bytes (16-byte aligned), n_image_frames >= n_offsets + set.max_frames - 1, n_offsets <= tmatch::piece_offsets.  A plan the kernel
// cannot take launches nothing and is a launch_error (kernels.h)
void launch_template_match(hipStream_t s, float *out, const uint8_t *image, size_t n_image_frames, size_t n_offsets, const TemplateSet &set);

}  // namespace bn
