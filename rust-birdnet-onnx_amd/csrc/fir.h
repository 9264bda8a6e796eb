// The kernel of bn_recording_create_filtered (fir.hip), launched by recording.cpp: an FIR filter over a whole recording as a banded
// Toeplitz product on the bf16 matrix pipe, f32-complete (bf16x3.h).  Geometry and the packed taps: fir_plan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fir_plan.h"
#include "pcm_layout.h"

namespace bn {

// dst [n] <- y[i] = sum_t taps[t] x[i + (n_taps - 1) / 2 - t], x the layout rule's sample of `src`, 0 outside [0, n).  `image` is
// fir::pack_taps(taps, n_taps) on the device (16-byte aligned), dst 16-byte aligned.  A tap count the plan refuses, a misaligned
// pointer, more chunks than a grid holds or a layout no reader knows launches nothing and is a launch_error (kernels.h)
void launch_fir(hipStream_t s, float *dst, const PcmSrc &src, uint64_t n, const void *image, uint32_t n_taps);

}  // namespace bn
