// Device side of the live ingest pool (bn_live_*, host logic in live.cpp): a slab of per-source rings in the storage format.
//
//   * live_gather_kernel -- chunk_audio on the ring (the live twin of kernels.hip's windows_kernel): row b of the launch is a
//     window of one source, its descriptor a kernel argument.  One lane = 4 consecutive samples of the window (float4 store;
//     S % 4 == 0), ring index (pos + j) wrapped with one compare (pos < R and j < S <= R), samples at or past `valid` read as
//     0 (the zero-padded tail after close), i16 converts as v / 32768 exactly like windows_kernel.  grid (ceil(S/1024), rows)
//   * live_scatter_kernel -- one workgroup per tile of a push's staged chunks; the host splits chunks at ring wraps and every
//     LIVE_TILE samples, so a tile is one contiguous copy and lanes move consecutive samples.
#include "live.h"

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

}  // namespace

void launch_live_gather(hipStream_t s, float *dst, const void *slab, int32_t is_i16, uint32_t ring_samples, uint32_t S, const LiveGatherRows &rows,
                        uint32_t n) {
    if (n == 0 || S == 0) return;
    dim3 grid((S / 4 + 255) / 256, n);
    if (is_i16) hipLaunchKernelGGL(live_gather_kernel<int16_t>, grid, dim3(256), 0, s, dst, static_cast<const int16_t *>(slab), ring_samples, S, rows);
    else hipLaunchKernelGGL(live_gather_kernel<float>, grid, dim3(256), 0, s, dst, static_cast<const float *>(slab), ring_samples, S, rows);
}

void launch_live_scatter(hipStream_t s, void *slab, int32_t is_i16, const LiveTile *tiles, uint32_t n_tiles, const void *data) {
    if (n_tiles == 0) return;
    if (is_i16)
        hipLaunchKernelGGL(live_scatter_kernel<int16_t>, dim3(n_tiles), dim3(256), 0, s, static_cast<int16_t *>(slab), tiles, static_cast<const int16_t *>(data));
    else hipLaunchKernelGGL(live_scatter_kernel<float>, dim3(n_tiles), dim3(256), 0, s, static_cast<float *>(slab), tiles, static_cast<const float *>(data));
}

}  // namespace bn
