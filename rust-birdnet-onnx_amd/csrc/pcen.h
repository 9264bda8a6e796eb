// The kernels of bn_recording_pcen (pcen.hip), launched by recording.cpp: per-channel energy normalisation of an f32 spectrogram
// image on the device, a chunked scan over time (pcen_plan.h), stored as floats or as threshold codes.  The image is what
// launch_spectrogram wrote (spectrogram.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcen_plan.h"

namespace bn {

// the device memory of a call's launches, sized for its longest piece
struct PcenScratch {
    float *sums;       // [chunks][n_rows]: S of each chunk
    uint32_t *counts;  // [chunks][n_rows]: n of each chunk
    float *carry;      // [chunks][n_rows]: M in front of each chunk
    float *state;      // [n_rows]: M in front of the piece; behind it when the launches are done
    const float *apow; // [CHUNK + 1]
    const float *thr;  // the 255 thresholds (BN_PCEN_U8 only)
};

// out [n_frames][n_rows] (floats, or bytes for BN_PCEN_U8) <- PCEN of image [n_frames][n_rows] floats, a piece that starts at a
// chunk's first frame; n_frames * n_rows <= 2^26.  first_rule: M in front of the piece is the first frame's rule (the call's first
// piece without a state_in), not sc.state.  Three launches: the chunks' sums, the carries, the values.  A plan the kernels cannot
// take launches nothing and is a launch_error (kernels.h)
void launch_pcen(hipStream_t s, void *out, const float *image, size_t n_frames, uint32_t n_rows, const pcen::Plan &plan, const PcenScratch &sc, bool first_rule);

}  // namespace bn
