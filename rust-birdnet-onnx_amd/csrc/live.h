// Kernels of the live ingest pool (live.hip), launched by live.cpp (bn_live_*, bn_step_live).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bn {

// one row of a gather launch: window w of a slot's ring
struct LiveRow {
    uint64_t base;   // element offset of the slot's ring in the slab (slot * ring_samples)
    uint32_t pos;    // ring index of the window's first sample (absolute start % ring_samples)
    uint32_t valid;  // samples of the window that were pushed (S before close; the rest reads as 0)
};
constexpr int LIVE_GATHER_ROWS = 128;  // rows per launch: the descriptors travel as kernel arguments (2 KiB)
struct LiveGatherRows {
    LiveRow r[LIVE_GATHER_ROWS];
};

// one tile of a scatter: len <= LIVE_TILE consecutive staged samples to consecutive ring elements (never across a wrap)
struct LiveTile {
    uint64_t dst;  // element offset in the slab
    uint32_t src;  // element offset in the staged data
    uint32_t len;
};
constexpr uint32_t LIVE_TILE = 4096;

// dst [n, S] f32 <- rows of the slab (i16 / 32768 or f32); S % 4 == 0, ring_samples >= S, n <= LIVE_GATHER_ROWS
void launch_live_gather(hipStream_t s, float *dst, const void *slab, int32_t is_i16, uint32_t ring_samples, uint32_t S, const LiveGatherRows &rows,
                        uint32_t n);
// slab <- staged chunks; tiles and data may live in pinned host memory or on the device
void launch_live_scatter(hipStream_t s, void *slab, int32_t is_i16, const LiveTile *tiles, uint32_t n_tiles, const void *data);

}  // namespace bn
