// The kernels of bn_recording_spectrogram (spectrogram.hip), launched by recording.cpp: the one-sided power of consecutive frames of
// a recording as bin rows or through a packed filter bank (spectrogram_plan.h), stored as floats or as threshold codes.  The
// tables are band levels' (band_levels.h, band_tables).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm_layout.h"
#include "spectrogram_plan.h"

namespace bn {

// The opt-in of the kernels of frame 2048 to more than 64 KiB of LDS on `device`: once per device, before the first launch there,
// never during a capture (LdsOptIn, capi_internal.h)
hipError_t spectrogram_prepare(int device);

// out [n_frames][plan.n_rows] (floats, or bytes for BN_SPECTROGRAM_U8; 16-byte aligned) <- frames starting at start + t * plan.hop
// of the recording's n_samples samples, zeros past them; start <= n_samples, n_frames <= spectro::piece_frames.  tab / scale from
// band_tables; thr: the 255 thresholds on the device (U8 only); image / tiles: the packed bank on the device (plan.bank only).  A
// plan the kernels cannot take or a layout no reader knows launches nothing and is a launch_error (kernels.h)
void launch_spectrogram(hipStream_t s, void *out, const PcmSrc &src, uint64_t n_samples, uint64_t start, uint32_t n_frames, const spectro::Plan &plan,
                        const float *tab, float scale, const float *thr, const void *image, const spectro::BankTiles *tiles, uint32_t n_tiles);

}  // namespace bn
