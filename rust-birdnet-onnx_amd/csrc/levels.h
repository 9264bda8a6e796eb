// Kernels in front of the plan that read chosen windows of recordings (levels.hip), launched by recording.cpp: the level meter
// (bn_recording_levels) and the gather of an explicit window list (bn_step_window_list, bn_recording_window_list).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm_layout.h"
#include "window_list_plan.h"

namespace bn {

// what levels_kernel stores per window: include/birdnet_hip.h's bn_window_level, field for field
struct WindowLevel {
    float peak, mean, mean_square;
    uint32_t flags;
};
static_assert(sizeof(WindowLevel) == 16 && sizeof(WindowLevel) == sizeof(bn_window_level), "one 16-byte store per window");

// out [count] <- the levels of windows first_start + w * step of the recording (counts in frames; S >= 1)
void launch_levels(hipStream_t s, WindowLevel *out, const PcmSrc &src, uint64_t n_samples, uint64_t first_start, uint64_t step, uint32_t S, uint32_t count);

// one row of a window-list launch: a window of any recording whose layout takes the launch's reader
struct WindowListRow {
    const void *base;   // first byte of the window's first frame (the recording's frame `start`)
    uint32_t valid;     // frames of the window the recording holds, 1..S; the rest reads as 0
    uint32_t dst;       // the row of dst it fills: its position in the list
    uint16_t channels;  // the interleaved readers' fields (pcm_read.h, PcmFrames); unused by the mono readers
    int16_t channel;
    float inv;
};
constexpr int WINDOW_LIST_ROWS = (int)wlist::ROWS_PER_LAUNCH;  // rows per launch: the descriptors travel as kernel arguments (3 KiB)
struct WindowListRows {
    WindowListRow r[WINDOW_LIST_ROWS];
};
static_assert(sizeof(WindowListRows) == 3072, "the descriptors and the other arguments stay within 4 KiB of kernel arguments");

// one row of a window-list launch as the host names it: the recording's bytes from the window's first frame on, with its layout
struct WindowListSrc {
    PcmSrc src;      // base: first byte of frame `start` of the recording
    uint32_t valid;  // as WindowListRow
    uint32_t dst;
};
// dst [.., S] f32 <- n <= WINDOW_LIST_ROWS rows; S % 4 == 0.  The reader is the one pcm_visit (pcm_read.h) picks for the rows' layouts,
// and its fields are a row's descriptor: rows of one launch must all take the same reader (window_list_plan.h groups them so).  A
// launch of more rows, of mixed readers or of a layout no reader knows is refused (kernels.h, launch_error) and launches nothing
void launch_window_list(hipStream_t s, float *dst, uint32_t S, const WindowListSrc *rows, uint32_t n);

}  // namespace bn
