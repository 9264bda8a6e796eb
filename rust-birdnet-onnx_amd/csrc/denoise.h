// The kernel of bn_recording_create_denoised (denoise.hip), launched by recording.cpp: spectral gating of a whole recording, one frame
// per wave in registers there and back (denoise_fft.h), the overlap-add in the same registers.  Geometry and tables: denoise_plan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "denoise_plan.h"
#include "pcm_layout.h"

namespace bn {

// The window table of frame length N on `device` (denoise::fill_tables, cached for the life of the process as band_tables caches its
// own) and the scale 1 / (N sum w^2) of the one-sided power
hipError_t denoise_tables(int device, uint32_t N, const float **tab, float *scale);

// dst [n] <- the rule of include/birdnet_hip.h, "Noise reduction", over the layout rule's samples of `src`, 0 outside [0, n).
// band_tab: band_tables' (the twiddles), win_tab / scale: denoise_tables', a: the plan's N/2 + 1 thresholds alpha * noise[k] on the
// device.  dst is 8-byte aligned.  A frame length without an instance, a missing table, more workgroups than a grid holds or a
// layout no reader knows launches nothing and is a launch_error (kernels.h); n == 0 launches nothing
void launch_denoise(hipStream_t s, float *dst, const PcmSrc &src, uint64_t n, const denoise::Plan &plan, const float *band_tab, const float *win_tab,
                    const float *a, float scale);

}  // namespace bn
