// Device side of the live ingest pool (bn_live_*, host logic in live.cpp): a slab of per-source rings in the storage format.
//
//   * live_gather_kernel -- chunk_audio on the ring (the live twin of kernels.hip's windows_kernel): row b of the launch is a
//     window of one source, its descriptor a kernel argument.  One lane = 4 consecutive samples of the window (float4 store;
//     S % 4 == 0), ring index (pos + j) wrapped with one compare (pos < R and j < S <= R), samples at or past `valid` read as
//     0 (the zero-padded tail after close), i16 converts as v / 32768 exactly like windows_kernel.  grid (ceil(S/1024), rows)
//   * live_scatter_kernel -- one workgroup per tile of a push's staged chunks; the host splits chunks at ring wraps and every
//     LIVE_TILE samples, so a tile is one contiguous copy and lanes move consecutive samples.
//   * live_scatter_frames_kernel -- the scatter of a pool whose pushes are interleaved frames or a format the ring does not store
//     (bn_live_create_layout): the same tiles, counted in frames; lane i of a tile reads frame src + i through the layout's
//     reader (pcm_read.h) and stores its f32 sample, so the ring holds exactly what a mono f32 pool fed those samples holds.
//   * live_resample_kernel -- the scatter of a resampling pool (bn_live_create_rates): one workgroup per tile of consecutive
//     FINAL outputs of one source.  The source span the tile's taps touch, [(n0*M)/L - (T/2-1), (n1*M)/L + T/2], is read
//     ONCE into LDS as f32 -- from the source's history (the last T-1 samples before this push) and the staged chunk, 0
//     before sample 0 of the stream and past the staged end (the tail a close flushes) -- and the phase table too when it fits
//     behind the span.  One lane = one output: kernels.hip's resample_kernel chain, fmaf(table[phase][j], x, acc) for
//     j = 0..T-1 in that order, so the ring holds the bits bn_recording_create_resampled computes.  LDS reads: lanes of a wave
//     read span[(o*M + r0)/L + j], a stride of M/L between lanes -- upsampling repeats addresses (broadcast), integer M/L odd
//     is conflict-free, 3/2 puts 48 addresses on ds_read_b32's 32 banks (2-way on a third of them); table rows of one wave
//     are at most L distinct addresses.  A tile of a source at the model's rate is a converting copy.
//   * live_history_kernel -- one workgroup per job: the last T-1 source samples of the stream after the push, from the old
//     history (shifted) and the staged chunk, read into registers before any is written.
#include "live.h"
#include "pcm_read.h"

namespace bn {
namespace {

template <class T>
__global__ __launch_bounds__(256) void live_gather_kernel(float *__restrict__ dst, const T *__restrict__ slab, uint32_t R, uint32_t S,
                                                          LiveGatherRows rows) {
    const uint32_t i = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i >= S) return;
    const LiveRow d = rows.r[blockIdx.y];
    const T *ring = slab + d.base;
    uint32_t q = d.pos + i;
    if (q >= R) q -= R;
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (i + u < d.valid) {
            if constexpr (sizeof(T) == 2) v[u] = (float)ring[q] * (1.0f / 32768.0f);
            else v[u] = (float)ring[q];
        } else {
            v[u] = 0.0f;
        }
        if (++q == R) q = 0;
    }
    *reinterpret_cast<float4 *>(dst + (uint64_t)blockIdx.y * S + i) = make_float4(v[0], v[1], v[2], v[3]);
}

template <class T>
__global__ __launch_bounds__(256) void live_scatter_kernel(T *__restrict__ slab, const LiveTile *__restrict__ tiles, const T *__restrict__ data) {
    const LiveTile t = tiles[blockIdx.x];
    T *dst = slab + t.dst;
    const T *src = data + t.src;
    for (uint32_t i = threadIdx.x; i < t.len; i += 256u) dst[i] = src[i];
}

template <class R>
__global__ __launch_bounds__(256) void live_scatter_frames_kernel(float *__restrict__ slab, const LiveTile *__restrict__ tiles, const R data) {
    const LiveTile t = tiles[blockIdx.x];
    float *dst = slab + t.dst;
    for (uint32_t i = threadIdx.x; i < t.len; i += 256u) dst[i] = data((uint64_t)t.src + i);
}

// R: the reader of the staged pushes (pcm_read.h), indexed in frames
template <class R>
__global__ __launch_bounds__(256) void live_resample_kernel(float *__restrict__ slab, const LiveRsTable *__restrict__ tables,
                                                            const float *__restrict__ coef, const float *__restrict__ hist,
                                                            const LiveRsJob *__restrict__ jobs, const LiveRsTile *__restrict__ tiles,
                                                            const R data) {
    extern __shared__ float lds[];
    const LiveRsTile t = tiles[blockIdx.x];
    const LiveRsJob jb = jobs[t.job];
    float *dst = slab + t.dst;
    const R staged = data.from(jb.src);
    if (jb.table == LIVE_RS_PASS) {
        const uint32_t first = (uint32_t)(t.n0 - jb.p0);
        for (uint32_t i = threadIdx.x; i < t.len; i += 256u) dst[i] = staged(first + i);
        return;
    }
    const LiveRsTable tb = tables[jb.table];
    const uint32_t L = tb.L, M = tb.M, T = tb.T;
    const uint64_t pos0 = t.n0 * M;
    const uint64_t base0 = pos0 / L;
    const uint32_t r0 = (uint32_t)(pos0 - base0 * L);
    // span index i holds stream sample q_lo + i; output o's first tap is span index (o*M + r0) / L
    const int64_t q_lo = (int64_t)base0 - (int64_t)(T / 2 - 1);
    const uint32_t span_len = ((t.len - 1u) * M + r0) / L + T;
    if (span_len > tb.span_cap) return;  // the host sizes tiles so that this never happens
    const int64_t p0 = (int64_t)jb.p0;
    const int64_t h0 = p0 - (int64_t)(T - 1);  // stream sample in history slot 0
    const float *hs = hist + jb.hist;
    for (uint32_t i = threadIdx.x; i < span_len; i += 256u) {
        const int64_t q = q_lo + i;
        float v = 0.0f;
        if (q >= p0) {
            if (q - p0 < (int64_t)jb.n_in) v = staged((uint64_t)(q - p0));
        } else if (q >= 0 && q >= h0) {
            v = hs[q - h0];
        }
        lds[i] = v;
    }
    const float *tab = coef + tb.coef_off;
    if (tb.lds_table) {
        float *lt = lds + tb.span_cap;
        for (uint32_t i = threadIdx.x; i < L * T; i += 256u) lt[i] = tab[i];
        tab = lt;
    }
    __syncthreads();
    for (uint32_t o = threadIdx.x; o < t.len; o += 256u) {
        const uint32_t pos = o * M + r0;
        const uint32_t b = pos / L;
        const float *row = tab + (pos - b * L) * T;
        const float *x = lds + b;
        float acc = 0.0f;
        for (uint32_t j = 0; j < T; j++) acc = fmaf(row[j], x[j], acc);
        dst[o] = acc;
    }
}

template <class R>
__global__ __launch_bounds__(256) void live_history_kernel(float *__restrict__ hist, const LiveRsTable *__restrict__ tables,
                                                           const LiveRsJob *__restrict__ jobs, const R data) {
    const LiveRsJob jb = jobs[blockIdx.x];
    if (jb.table == LIVE_RS_PASS || jb.n_in == 0) return;
    const uint32_t H = tables[jb.table].T - 1u;  // <= LIVE_RS_MAX_T - 1 = 2 * 256 - 1
    float *hs = hist + jb.hist;
    const R staged = data.from(jb.src);
    // slot h of the new history holds stream sample p0 + n_in - H + h: staged sample n_in - H + h, or old slot h + n_in
    float v[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const uint32_t h = threadIdx.x + 256u * u;
        v[u] = 0.0f;
        if (h < H) {
            const int64_t k = (int64_t)jb.n_in - (int64_t)H + (int64_t)h;
            v[u] = k >= 0 ? staged((uint64_t)k) : hs[h + jb.n_in];
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const uint32_t h = threadIdx.x + 256u * u;
        if (h < H) hs[h] = v[u];
    }
}

}  // namespace

void launch_live_gather(hipStream_t s, float *dst, const void *slab, int32_t is_i16, uint32_t ring_samples, uint32_t S, const LiveGatherRows &rows,
                        uint32_t n) {
    if (n == 0 || S == 0) return;
    dim3 grid((S / 4 + 255) / 256, n);
    if (is_i16) hipLaunchKernelGGL(live_gather_kernel<int16_t>, grid, dim3(256), 0, s, dst, static_cast<const int16_t *>(slab), ring_samples, S, rows);
    else hipLaunchKernelGGL(live_gather_kernel<float>, grid, dim3(256), 0, s, dst, static_cast<const float *>(slab), ring_samples, S, rows);
}

void launch_live_scatter(hipStream_t s, void *slab, const PcmSrc &data, const LiveTile *tiles, uint32_t n_tiles) {
    if (n_tiles == 0) return;
    if (pcm_is_plain(data.layout)) {  // the ring stores what the pushes carry: a copy
        if (data.layout.format == BN_PCM_I16)
            hipLaunchKernelGGL(live_scatter_kernel<int16_t>, dim3(n_tiles), dim3(256), 0, s, static_cast<int16_t *>(slab), tiles,
                               static_cast<const int16_t *>(data.base));
        else
            hipLaunchKernelGGL(live_scatter_kernel<float>, dim3(n_tiles), dim3(256), 0, s, static_cast<float *>(slab), tiles,
                               static_cast<const float *>(data.base));
        return;
    }
    pcm_visit(data, [&](auto rd) {
        hipLaunchKernelGGL(live_scatter_frames_kernel<decltype(rd)>, dim3(n_tiles), dim3(256), 0, s, static_cast<float *>(slab), tiles, rd);
    });
}

void launch_live_resample(hipStream_t s, float *slab, const PcmSrc &data, const LiveRsTable *tables, const float *coef, const float *hist,
                          const LiveRsJob *jobs, const LiveRsTile *tiles, uint32_t n_tiles, uint32_t lds_bytes) {
    if (n_tiles == 0) return;
    pcm_visit(data, [&](auto rd) {
        hipLaunchKernelGGL(live_resample_kernel<decltype(rd)>, dim3(n_tiles), dim3(256), lds_bytes, s, slab, tables, coef, hist, jobs, tiles, rd);
    });
}

void launch_live_history(hipStream_t s, float *hist, const PcmSrc &data, const LiveRsTable *tables, const LiveRsJob *jobs, uint32_t n_jobs) {
    if (n_jobs == 0) return;
    pcm_visit(data, [&](auto rd) { hipLaunchKernelGGL(live_history_kernel<decltype(rd)>, dim3(n_jobs), dim3(256), 0, s, hist, tables, jobs, rd); });
}

}  // namespace bn
