// Kernels of the live ingest pool (live.hip), launched by live.cpp (bn_live_*, bn_step_live).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm_layout.h"

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

// ---- resampling pools (bn_live_create_rates): the ring holds f32 at the model's rate, pushes are converted as they land ----
// one polyphase table of the pool
struct LiveRsTable {
    uint32_t L, M, T;
    uint32_t coef_off;   // element offset of [L][T] in the pool's coefficient buffer
    uint32_t lds_table;  // 1: the kernel copies the table into LDS behind the span
    uint32_t span_cap;   // floats of LDS the span may take (the host sizes tiles so that it does)
};
// one source touched by a push (or closed): its new source samples [p0, p0 + n_in) lie contiguously in the staged data
struct LiveRsJob {
    uint64_t p0;     // source samples of the stream before this call
    uint64_t hist;   // element offset of the source's history in the history buffer
    uint32_t src;    // element offset of its new samples in the staged data
    uint32_t n_in;   // new source samples (0: a close, everything past p0 reads as 0)
    uint32_t table;  // index into the pool's tables, LIVE_RS_PASS for a source at the model's rate (converting copy)
    uint32_t pad;
};
constexpr uint32_t LIVE_RS_PASS = 0xffffffffu;
// one tile: len consecutive outputs [n0, n0 + len) of a job to consecutive ring elements (never across a wrap); for a
// pass-through job the outputs are the source samples themselves
struct LiveRsTile {
    uint64_t dst;  // element offset in the slab
    uint64_t n0;   // index of the first output in the source's stream
    uint32_t len;
    uint32_t job;
};
constexpr uint32_t LIVE_RS_MAX_T = 512;          // taps per phase a resampling pool accepts (the history kernel holds T - 1 <= 2 * 256 - 1)
constexpr uint32_t LIVE_RS_LDS_FLOATS = 16384;  // LDS budget of the resampling scatter: span, and the table when it fits beside it

// dst [n, S] f32 <- rows of the slab (a ring is mono int16, read as v / 32768, or f32); S % 4 == 0, ring_samples >= S, n <= LIVE_GATHER_ROWS
void launch_live_gather(hipStream_t s, float *dst, const void *slab, int32_t is_i16, uint32_t ring_samples, uint32_t S, const LiveGatherRows &rows,
                        uint32_t n);
// slab <- staged chunks; tiles and data may live in pinned host memory or on the device.  Mono int16 / float data is copied into a
// ring of its own format; any other layout (pcm_layout.h) is converted frame by frame into an f32 ring, tiles counting frames
void launch_live_scatter(hipStream_t s, void *slab, const PcmSrc &data, const LiveTile *tiles, uint32_t n_tiles);
// slab (f32) <- the tiles' outputs: the T-tap fmaf chain of kernels.hip's resample_kernel over [history | staged chunk]; jobs,
// tiles and data may live in pinned host memory or on the device; lds_bytes: the pool's dynamic LDS size
void launch_live_resample(hipStream_t s, float *slab, const PcmSrc &data, const LiveRsTable *tables, const float *coef, const float *hist,
                          const LiveRsJob *jobs, const LiveRsTile *tiles, uint32_t n_tiles, uint32_t lds_bytes);
// history <- the last T - 1 source samples of every job's stream after its push; launched after launch_live_resample on the
// same stream (blocks of the resampling launch read the history, so it is not updated there)
void launch_live_history(hipStream_t s, float *hist, const PcmSrc &data, const LiveRsTable *tables, const LiveRsJob *jobs, uint32_t n_jobs);

}  // namespace bn
