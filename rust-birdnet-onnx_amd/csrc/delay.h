// The kernel of bn_recording_delay (delay.hip), launched by recording.cpp: per window the generalised cross-correlation of two
// recordings over the lags of a checked spec (delay_plan.h), its peak and the two values beside it.  The tables are band levels'
// (band_levels.h, band_tables).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "delay_plan.h"
#include "pcm_layout.h"

namespace bn {

// what delay_kernel stores per window: include/birdnet_hip.h's bn_window_delay, field for field
struct WindowDelay {
    int32_t peak_lag;
    float peak, before, after;
    uint32_t flags, n_frames;
};
static_assert(sizeof(WindowDelay) == 24 && sizeof(WindowDelay) == sizeof(bn_window_delay), "6 dwords per window");

// out [count] <- the records of windows first_start + w * step of a against the same windows of b (counts in frames), and, unless
// curve is NULL, curve [count][plan.n_lags] <- their correlations at lags -max_lag .. +max_lag; S >= plan.N, tab from band_tables.
// a and b must take the same reader (wlist::reader_kind): a pair of two kinds, a frame length without a kernel or a layout no reader
// knows launches nothing and is a launch_error (kernels.h)
void launch_delay(hipStream_t s, WindowDelay *out, float *curve, const PcmSrc &a, uint64_t n_a, const PcmSrc &b, uint64_t n_b, uint64_t first_start,
                  uint64_t step, uint32_t S, uint32_t count, const delay::Plan &plan, const float *tab);

}  // namespace bn
