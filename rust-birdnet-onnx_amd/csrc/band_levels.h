// The kernel of bn_recording_band_levels (band_levels.hip), launched by recording.cpp: per window the power inside the bands of a checked
// spec (band_plan.h), mean and maximum over the window's frames.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "band_plan.h"
#include "pcm_layout.h"

namespace bn {

// what band_levels_kernel stores per window: include/birdnet_hip.h's bn_window_bands, field for field
struct WindowBands {
    float mean[BN_BAND_MAX], max[BN_BAND_MAX];
    float total_mean, total_max;
    uint32_t flags, n_frames;
};
static_assert(sizeof(WindowBands) == 80 && sizeof(WindowBands) == sizeof(bn_window_bands), "20 dwords per window");

// The tables of a frame length on `device` (band_plan.h, fill_tables), computed and uploaded on first use and kept for the life of the
// process; *scale is 1 / (N * sum hann^2).  The thread's device must be `device`.  hipSuccess or the runtime's error
hipError_t band_tables(int device, uint32_t N, const float **tab, float *scale);

// out [count] <- the bands of windows first_start + w * step of the recording (counts in frames), S >= plan.N, tab / scale from
// band_tables.  A frame length without a kernel or a layout no reader knows launches nothing and is a launch_error (kernels.h)
void launch_band_levels(hipStream_t s, WindowBands *out, const PcmSrc &src, uint64_t n_samples, uint64_t first_start, uint64_t step, uint32_t S,
                        uint32_t count, const band::Plan &plan, const float *tab, float scale);

}  // namespace bn
