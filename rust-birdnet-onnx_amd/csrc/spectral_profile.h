// The kernel of bn_recording_spectral_profile (spectral_profile.hip), launched by recording.cpp: per window the mean power, the summed
// amplitude and the summed absolute change of the amplitude of every bin of a checked spec (profile_plan.h), and the acoustic
// complexity index they give.  The tables are band levels' (band_levels.h, band_tables).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm_layout.h"
#include "profile_plan.h"

namespace bn {

// what spectral_profile_kernel stores per window: include/birdnet_hip.h's bn_window_profile, field for field
struct WindowProfile {
    float aci, total_mean;
    uint32_t flags, n_frames;
};
static_assert(sizeof(WindowProfile) == 16 && sizeof(WindowProfile) == sizeof(bn_window_profile), "4 dwords per window");

// out [count] <- the records of windows first_start + w * step of the recording (counts in frames), and, unless planes is NULL,
// planes [count][BN_PROFILE_PLANES][plan.n_bins] <- their planes; S >= plan.N, tab / scale from band_tables.  A frame length without
// a kernel or a layout no reader knows launches nothing and is a launch_error (kernels.h)
void launch_spectral_profile(hipStream_t s, WindowProfile *out, float *planes, const PcmSrc &src, uint64_t n_samples, uint64_t first_start, uint64_t step,
                             uint32_t S, uint32_t count, const profile::Plan &plan, const float *tab, float scale);

}  // namespace bn
