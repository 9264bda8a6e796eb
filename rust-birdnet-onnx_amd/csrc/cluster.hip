// bn_index_assign and bn_index_cluster behind the C ABI (include/birdnet_hip.h): the nearest centroid of every stored row of an
// index, and spherical k-means built on it, without the slab leaving the device.
//
// Kernels:
//   * cluster_scan_kernel -- each workgroup streams its contiguous range of 64-row tiles ONCE for all centroids of the pass (up
//     to 64), in rank_scan_kernel's form (rank.hip): row = A operand, centroid = B operand of v_mfma_f32_16x16x4_f32, k =
//     16 s + 4 (lane >> 4) + t of each 128-wide chunk, s then t ascending, ONE accumulator per (centroid, row), then + 0.0f: the
//     bits of bn_head_apply_host for a head with W = centroids, no bias and flags 0 on the stored row.  Each tile's
//     [64 centroids x 64 rows] scores go to LDS; there one wave takes, per row, the pass's centroids in ascending order against
//     the row's running (best score, best index), which it reads from and writes back to two planes in device memory: a later
//     centroid, and a later pass, replaces the running best only on a strictly larger score, a NaN never.
//   * cluster_stats_kernel -- rows moved against the previous assignment (which it then replaces) and the clusters' sizes
//     (integer atomics: exact in any order).
//   * cluster_offsets_kernel, cluster_members_kernel -- the member list: per cluster its rows' ids ascending, packed in cluster
//     order.  One workgroup per cluster walks the assignment plane; a wave's quarter is counted first, then compacted in place.
//   * cluster_segsum_kernel, cluster_fold_kernel, cluster_finish_kernel -- the update.  Segment j of a cluster is its members
//     [256 j, 256 j + 256) of the list, summed in list order in float64, one thread per component; the segments are added in
//     segment order in float64; a fixed number of segment slots per cluster is summed and folded per round, so the partial sums
//     take slots x k x dpad doubles however many rows there are.  The finish takes the float64 norm (components by a fixed
//     stride, then a fixed tree) and stores sum / norm as f32, or keeps the centroid.  The association is a function of a
//     member's rank in its cluster alone: never of the grid or the device.  No floating-point atomics anywhere.
//   * cluster_gather_kernel, cluster_argmin_kernel, cluster_pick_kernel -- the starts: stored rows become centroids; the max-min
//     start picks the row whose running best is smallest (ties by id: the order (score, id) is total, so the reduction's shape
//     cannot matter) and marks a picked row with a best score of +inf, which no honest score reaches and no pass replaces.
// Everything runs on the index's stream.  The buffers hang off the index (allocated on first use, freed with it).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "cluster_assign.h"
#include "device_common.h"
#include "hip_gate.h"
#include "topm_select.h"

namespace {

constexpr int KC = 128;   // k-step: the slab's and the centroids' rows are padded to a multiple of it
constexpr int TILE = 64;  // rows per workgroup tile: 4 waves x 16 rows
constexpr int CP = 64;    // centroids per scan pass
constexpr int WS_LD = KC + 4;
constexpr int S_LD = TILE + 1;
using bn::cluster::K_MAX;
constexpr uint32_t SEG = 256;         // members per segment of the update's sums
constexpr int ARG_BLOCKS = 256;       // blocks of cluster_argmin_kernel
constexpr uint32_t STATS_ROWS = 4096;  // rows per block of cluster_stats_kernel
constexpr size_t PART_BYTES = (size_t)32 << 20;  // what the segment slots of one round may take
constexpr uint32_t NONE = BN_CLUSTER_NONE;
constexpr uint32_t NEVER = 0xFEFEFEFEu;  // a previous assignment no row has (every byte 0xFE: set by a memset)

using bn::floatx4;
using bn::topm::lanes_below;

constexpr size_t SCAN_LDS = (size_t)CP * WS_LD * 4 + (size_t)CP * S_LD * 4;  // 50 432 bytes: below the 64 KB every kernel may use

// Scan of one pass (nc <= CP centroids c0 .. c0 + nc - 1, CB = ceil(nc / 16) blocks) over the tiles [tile_lo, tile_hi).  Workgroup g
// owns tiles [tile_lo + g * tiles_per_wg, ...).  The operand layout is rank_scan_kernel's.  W points at the pass's first centroid.
// first != 0: the running best starts empty (NaN, NONE); else it is read from the planes.  Rows outside [id_lo, id_hi) and rows
// the index holds invalid keep / get (NaN, NONE).  The planes are indexed by row id; a tile's 64 rows lie inside the padded slab.
template <int CB>
__global__ __launch_bounds__(256) void cluster_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t id_lo, uint32_t id_hi,
                                                           uint32_t dpad, const float *__restrict__ W, int nc, uint32_t c0, int first, uint32_t tile_lo,
                                                           uint32_t tile_hi, uint32_t tiles_per_wg, float *__restrict__ best_s, uint32_t *__restrict__ best_i) {
    extern __shared__ __align__(16) float cluster_lds[];
    float *Ws = cluster_lds;     // [CP][WS_LD]: the centroids' current k chunk
    float *S = Ws + CP * WS_LD;  // [CP][S_LD]: scores of the current tile

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const uint32_t t0 = min(tile_hi, tile_lo + blockIdx.x * tiles_per_wg);
    const uint32_t t1 = min(tile_hi, t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;

    // step u = (tile t0 + u / nkc, chunk u % nkc); the row chunk and the centroid chunk of step u + 1 are loaded during step u
    auto row_ptr = [&](uint32_t u) {
        const size_t row = (size_t)(t0 + u / nkc) * TILE + w * 16 + r16;  // < the slab's rows (padded to TILE)
        return slab + row * dpad + (u % nkc) * KC + 4 * h;
    };
    constexpr int WV = CB * 16 * (KC / 4) / 256;  // float4 of the centroid chunk per thread
    float4 a[8], wr[WV];
    auto load_w = [&](uint32_t u) {
        const uint32_t c = u % nkc;
#pragma unroll
        for (int j = 0; j < WV; j++) {
            const int e = tid + 256 * j, cc = e >> 5, kk = (e & 31) * 4;
            wr[j] = cc < nc ? *reinterpret_cast<const float4 *>(W + (size_t)cc * dpad + c * KC + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    if (steps) {
        const float *rp = row_ptr(0);
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
        load_w(0);
    }
    floatx4 acc[CB];
#pragma unroll
    for (int b = 0; b < CB; b++) acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (uint32_t u = 0; u < steps; u++) {
        __syncthreads();  // the previous chunk's Ws reads and the previous tile's S reads are done
#pragma unroll
        for (int j = 0; j < WV; j++) {
            const int e = tid + 256 * j, cc = e >> 5, kk = (e & 31) * 4;
            *reinterpret_cast<float4 *>(Ws + cc * WS_LD + kk) = wr[j];
        }
        __syncthreads();
        float4 an[8];
        if (u + 1 < steps) {
            const float *rp = row_ptr(u + 1);
#pragma unroll
            for (int s = 0; s < 8; s++) an[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
            load_w(u + 1);
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
#pragma unroll
            for (int b = 0; b < CB; b++) {
                const float4 bw = *reinterpret_cast<const float4 *>(Ws + (b * 16 + r16) * WS_LD + 16 * s + 4 * h);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, bw.x, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, bw.y, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, bw.z, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, bw.w, acc[b], 0, 0, 0);
            }
        }
        if (u + 1 < steps) {
#pragma unroll
            for (int s = 0; s < 8; s++) a[s] = an[s];
        }
        if ((u + 1) % nkc) continue;

        // ---- end of a tile: scores to LDS (the head's bias add, with a bias of +0.0), then wave 0 takes the argmax of each row
        const uint32_t t = t0 + u / nkc;
#pragma unroll
        for (int b = 0; b < CB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = acc[b][r] + 0.0f;
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        if (w == 0) {
            const uint32_t grow = t * TILE + lane;
            const bool row_ok = grow >= id_lo && grow < id_hi && valid[grow];
            float bs = __builtin_nanf("");
            uint32_t bi = NONE;
            if (!first && row_ok) {
                bs = best_s[grow];
                bi = best_i[grow];
            }
            if (row_ok) {
                for (int cc = 0; cc < nc; cc++) {
                    const float s = S[cc * S_LD + lane];
                    if (s == s && (bi == NONE || s > bs)) {
                        bs = s;
                        bi = c0 + cc;
                    }
                }
            }
            best_s[grow] = bs;
            best_i[grow] = bi;
        }
    }
}

const void *scan_of(int cb) {
    switch (cb) {
        case 1: return reinterpret_cast<const void *>(cluster_scan_kernel<1>);
        case 2: return reinterpret_cast<const void *>(cluster_scan_kernel<2>);
        case 3: return reinterpret_cast<const void *>(cluster_scan_kernel<3>);
        default: return reinterpret_cast<const void *>(cluster_scan_kernel<4>);
    }
}

// Block b: rows [id_lo + STATS_ROWS b, + STATS_ROWS) of the range.  scalars[0] += rows whose assignment differs from prev (which
// becomes the assignment), counts[c] += members of c (collected in LDS first).  counts and scalars[0] are zero on entry.
__global__ __launch_bounds__(256) void cluster_stats_kernel(const uint32_t *__restrict__ best_i, uint32_t *__restrict__ prev_i, uint32_t id_lo, uint32_t id_hi,
                                                            uint32_t k, uint32_t *__restrict__ counts, uint32_t *__restrict__ scalars) {
    __shared__ uint32_t hist[K_MAX];
    __shared__ uint32_t moved;
    for (uint32_t c = threadIdx.x; c < k; c += 256) hist[c] = 0;
    if (threadIdx.x == 0) moved = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)id_lo + (uint64_t)blockIdx.x * STATS_ROWS;
    uint32_t mine = 0;
    for (uint32_t j = threadIdx.x; j < STATS_ROWS; j += 256) {
        const uint64_t i = base + j;
        if (i >= id_hi) break;
        const uint32_t b = best_i[i];
        if (b != prev_i[i]) mine++;
        prev_i[i] = b;
        if (b < k) atomicAdd(&hist[b], 1u);
    }
    if (mine) atomicAdd(&moved, mine);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < k; c += 256)
        if (hist[c]) atomicAdd(&counts[c], hist[c]);
    if (threadIdx.x == 0 && moved) atomicAdd(&scalars[0], moved);
}

// offsets[c] = counts[0] + .. + counts[c - 1], offsets[k] = the assigned rows
__global__ __launch_bounds__(64) void cluster_offsets_kernel(const uint32_t *__restrict__ counts, uint32_t k, uint32_t *__restrict__ offsets) {
    if (threadIdx.x) return;
    uint32_t run = 0;
    for (uint32_t c = 0; c < k; c++) {
        offsets[c] = run;
        run += counts[c];
    }
    offsets[k] = run;
}

// Workgroup c: members[offsets[c] ..) = the ids of the range's rows assigned to c, ascending.  Wave w walks the quarter
// [id_lo + w * quarter, + quarter) of the range (quarter a multiple of 64) twice: counting, then writing behind the earlier waves'
// counts.  The writes stay below offsets[c] + counts[c]: both were taken from the plane this kernel reads.
__global__ __launch_bounds__(256) void cluster_members_kernel(const uint32_t *__restrict__ best_i, uint32_t id_lo, uint32_t id_hi, uint32_t quarter,
                                                              const uint32_t *__restrict__ offsets, uint32_t *__restrict__ members) {
    __shared__ uint32_t wcount[4];
    const uint32_t c = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t q0 = min((uint64_t)id_hi, (uint64_t)id_lo + (uint64_t)w * quarter), q1 = min((uint64_t)id_hi, q0 + quarter);
    uint32_t n = 0;
    for (uint64_t i0 = q0; i0 < q1; i0 += 64) {
        const uint64_t i = i0 + lane;
        n += __popcll(__ballot(i < q1 && best_i[i] == c));
    }
    if (lane == 0) wcount[w] = n;
    __syncthreads();
    uint32_t at = offsets[c];
    for (int j = 0; j < w; j++) at += wcount[j];
    for (uint64_t i0 = q0; i0 < q1; i0 += 64) {
        const uint64_t i = i0 + lane;
        const bool mine = i < q1 && best_i[i] == c;
        const uint64_t m = __ballot(mine);
        if (mine) members[at + lanes_below(m)] = (uint32_t)i;
        at += __popcll(m);
    }
}

// Block (slot, c, z): part[c][slot][col] = the sum over segment seg0 + slot of cluster c, in list order, of slab[member][col] in
// float64; col = 256 z + thread.  A segment past the cluster's end writes nothing (and is not read by the fold).
__global__ __launch_bounds__(256) void cluster_segsum_kernel(const float *__restrict__ slab, uint32_t dpad, const uint32_t *__restrict__ members,
                                                             const uint32_t *__restrict__ offsets, const uint32_t *__restrict__ counts, uint32_t seg0,
                                                             uint32_t slots, double *__restrict__ part) {
    const uint32_t c = blockIdx.y, col = blockIdx.z * 256 + threadIdx.x;
    const uint32_t m = counts[c];
    const uint64_t start = (uint64_t)(seg0 + blockIdx.x) * SEG;
    if (start >= m || col >= dpad) return;
    const uint32_t len = (uint32_t)min((uint64_t)SEG, m - start);
    const uint32_t *list = members + offsets[c] + start;
    double sum = 0.0;
    uint32_t j = 0;
    for (; j + 8 <= len; j += 8) {  // eight loads in flight, added in list order
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; e++) v[e] = slab[(size_t)list[j + e] * dpad + col];
#pragma unroll
        for (int e = 0; e < 8; e++) sum += (double)v[e];
    }
    for (; j < len; j++) sum += (double)slab[(size_t)list[j] * dpad + col];
    part[((size_t)c * slots + blockIdx.x) * dpad + col] = sum;
}

// Block (c, z): acc[c][col] (0 when seg0 == 0) += the round's segment sums of cluster c in slot order
__global__ __launch_bounds__(256) void cluster_fold_kernel(const double *__restrict__ part, uint32_t dpad, const uint32_t *__restrict__ counts, uint32_t seg0,
                                                           uint32_t slots, double *__restrict__ acc) {
    const uint32_t c = blockIdx.x, col = blockIdx.y * 256 + threadIdx.x;
    if (col >= dpad) return;
    const uint32_t m = counts[c];
    double a = seg0 ? acc[(size_t)c * dpad + col] : 0.0;
    for (uint32_t p = 0; p < slots && (uint64_t)(seg0 + p) * SEG < m; p++) a += part[((size_t)c * slots + p) * dpad + col];
    acc[(size_t)c * dpad + col] = a;
}

// Workgroup c: norm = sqrt(sum_col acc[c][col]^2) in float64 (thread t adds its columns t, t + 256, .. in order; the threads by a
// fixed tree); centroid = (float)(acc / norm), or unchanged (scalars[1] += 1) for no members or a zero / non-finite norm
__global__ __launch_bounds__(256) void cluster_finish_kernel(const double *__restrict__ acc, uint32_t dpad, const uint32_t *__restrict__ counts,
                                                             float *__restrict__ cent, uint32_t *__restrict__ scalars) {
    __shared__ double sh[256];
    const uint32_t c = blockIdx.x;
    const double *a = acc + (size_t)c * dpad;
    double ss = 0.0;
    for (uint32_t col = threadIdx.x; col < dpad; col += 256) ss += a[col] * a[col];
    sh[threadIdx.x] = ss;
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    const double norm = sqrt(sh[0]);
    const bool ok = counts[c] > 0 && norm > 0.0 && norm < (double)INFINITY;  // false for a NaN norm
    if (!ok) {
        if (threadIdx.x == 0) atomicAdd(&scalars[1], 1u);
        return;
    }
    for (uint32_t col = threadIdx.x; col < dpad; col += 256) cent[(size_t)c * dpad + col] = (float)(a[col] / norm);
}

// stored rows ids[c] -> centroids [k, dpad], as stored
__global__ __launch_bounds__(256) void cluster_gather_kernel(const float *__restrict__ slab, const uint32_t *__restrict__ ids, uint32_t dpad,
                                                             float *__restrict__ cent) {
    const size_t row = ids[blockIdx.x];
    for (uint32_t col = threadIdx.x; col < dpad; col += 256) cent[(size_t)blockIdx.x * dpad + col] = slab[row * dpad + col];
}

// a picked row: no later pass replaces its running best, no later pick takes it
__global__ void cluster_mark_kernel(float *__restrict__ best_s, uint32_t id) { best_s[id] = INFINITY; }

struct Pick {
    float s;
    uint32_t id;
};
__device__ inline bool pick_before(const Pick &a, const Pick &b) { return b.id == NONE || (a.id != NONE && (a.s < b.s || (a.s == b.s && a.id < b.id))); }

__device__ inline Pick block_min(Pick p, Pick *sh) {
    sh[threadIdx.x] = p;
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
        if ((int)threadIdx.x < off && pick_before(sh[threadIdx.x + off], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + off];
        __syncthreads();
    }
    return sh[0];
}

// part[b] = the block's smallest (running best, id) over the range's assigned, unpicked rows (ties: -0.0 == +0.0, then the id)
__global__ __launch_bounds__(256) void cluster_argmin_kernel(const float *__restrict__ best_s, const uint32_t *__restrict__ best_i, uint32_t id_lo,
                                                             uint32_t id_hi, Pick *__restrict__ part) {
    __shared__ Pick sh[256];
    Pick p{0.f, NONE};
    for (uint64_t i = (uint64_t)id_lo + blockIdx.x * 256 + threadIdx.x; i < id_hi; i += (uint64_t)ARG_BLOCKS * 256) {
        const float s = best_s[i];
        if (best_i[i] == NONE || !(s < INFINITY)) continue;  // invalid, NaN or picked
        const Pick q{s, (uint32_t)i};
        if (pick_before(q, p)) p = q;
    }
    p = block_min(p, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = p;
}

// the smallest of the blocks' picks becomes centroid j: its id to start_ids[j], its row to cent[j], its running best to +inf
__global__ __launch_bounds__(256) void cluster_pick_kernel(const Pick *__restrict__ part, const float *__restrict__ slab, uint32_t dpad, uint32_t j,
                                                           uint32_t *__restrict__ start_ids, float *__restrict__ cent, float *__restrict__ best_s) {
    __shared__ Pick sh[256];
    const Pick p = block_min(part[threadIdx.x], sh);  // ARG_BLOCKS == 256 entries
    if (threadIdx.x == 0) start_ids[j] = p.id;
    if (p.id == NONE) return;  // the host refuses a range with fewer valid rows than centroids, so this is not reached
    for (uint32_t col = threadIdx.x; col < dpad; col += 256) cent[(size_t)j * dpad + col] = slab[(size_t)p.id * dpad + col];
    if (threadIdx.x == 0) best_s[p.id] = INFINITY;
}

}  // namespace

// an index's clustering buffers: each allocated when a call first needs it, grown when a call needs more (the centroids [k, dpad]
// and the running best planes by row id are the base's)
struct bn::ClusterState : bn::cluster::AssignBufs {
    bn::DeviceBuf<uint32_t> d_prev_i, d_members;  // the previous assignment; the member lists
    size_t list_n = 0;
    bn::DeviceBuf<uint32_t> d_small;  // counts [K_MAX], offsets [K_MAX + 1], scalars [2] (moved, kept centroids), start ids [K_MAX]
    bn::DeviceBuf<Pick> d_pick;       // [ARG_BLOCKS]
    bn::DeviceBuf<double> d_acc;      // [k, dpad]
    size_t acc_n = 0;
    bn::DeviceBuf<double> d_part;  // [k, slots, dpad]
    size_t part_n = 0;
};

void bn::cluster_state_free(ClusterState *s) { delete s; }

namespace {

using bn::check_launch;
using bn::set_last_error;

constexpr size_t SMALL_COUNTS = 0, SMALL_OFFSETS = K_MAX, SMALL_SCALARS = 2 * K_MAX + 1, SMALL_START = 2 * K_MAX + 3, SMALL_N = 3 * K_MAX + 3;

// room for n elements; the stream is idle between calls, so the old block is free to go
template <class T>
hipError_t ensure(bn::DeviceBuf<T> &p, size_t &have, size_t n) {
    if (n <= have) return hipSuccess;
    have = 0;
    hipError_t e = p.alloc(n * sizeof(T));  // the old block goes first
    if (e == hipSuccess) have = n;
    return e;
}

bn_status check_common(const bn_index *x, size_t k, uint64_t first_id, uint64_t n_ids) {
    if (k < 1 || k > K_MAX) return set_last_error(BN_ERR_INVALID_ARG, "k must be in 1..1024, got " + std::to_string(k));
    const size_t size = bn_index_size(x);
    if (first_id > size || n_ids > size - first_id)
        return set_last_error(BN_ERR_INVALID_ARG, "rows [" + std::to_string(first_id) + ", +" + std::to_string(n_ids) + ") run past the index's " + std::to_string(size) + " rows");
    return BN_OK;
}

}  // namespace

// ---- what ivf.hip shares (cluster_assign.h)
namespace bn {
namespace cluster {

bn_status check_finite(const float *c, size_t n, const char *what) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(c[i])) return set_last_error(BN_ERR_INVALID_ARG, std::string(what) + " element " + std::to_string(i) + " is not finite");
    return BN_OK;
}

Range range_of(const bn::IndexScan &s, uint64_t first_id, uint64_t n_ids) {
    Range r;
    r.id_lo = (uint32_t)first_id;
    r.id_hi = (uint32_t)(n_ids ? first_id + n_ids : s.size);
    r.tile_lo = r.id_lo / TILE;
    r.tile_hi = (r.id_hi + TILE - 1) / TILE;
    // the grid rule: the range's tiles in contiguous runs, at most one workgroup per compute unit
    const uint32_t n_tiles = r.tile_hi - r.tile_lo;
    r.tpw = std::max<uint32_t>(1, (n_tiles + s.max_wg - 1) / s.max_wg);
    r.n_wg = (n_tiles + r.tpw - 1) / r.tpw;
    return r;
}

// the centroids and the running best planes (every row of the range's tiles is written by a pass)
bn_status reserve_assign(AssignBufs *cs, const bn::IndexScan &s, size_t k) {
    BN_HIP_TRY(ensure(cs->d_cent, cs->cent_n, k * s.dpad));
    const size_t rows = (s.size + TILE - 1) / TILE * TILE;
    if (rows > cs->best_n) {
        size_t a = cs->best_n, b = cs->best_n;
        BN_HIP_TRY(ensure(cs->d_best_s, a, rows));
        BN_HIP_TRY(ensure(cs->d_best_i, b, rows));
        cs->best_n = rows;
    }
    return BN_OK;
}

bn_status upload_centroids(AssignBufs *cs, const bn::IndexScan &s, const float *c, size_t k) {
    std::vector<float> pad(k * s.dpad, 0.f);
    for (size_t i = 0; i < k; i++) memcpy(pad.data() + i * s.dpad, c + i * s.dim, s.dim * sizeof(float));
    BN_HIP_TRY(bn::gated::Memcpy(cs->d_cent, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    return BN_OK;
}

// one pass of the scan: centroids [c0, c0 + nc) of d_cent against the range
bn_status enqueue_pass(AssignBufs *cs, const bn::IndexScan &s, const Range &r, size_t c0, int nc, bool first_pass) {
    const float *W = cs->d_cent + c0 * s.dpad;
    uint32_t lo = r.id_lo, hi = r.id_hi, d = (uint32_t)s.dpad, cc0 = (uint32_t)c0, tl = r.tile_lo, th = r.tile_hi, tpw = r.tpw;
    int first = first_pass ? 1 : 0;
    float *best_s = cs->d_best_s;
    uint32_t *best_i = cs->d_best_i;
    void *args[] = {(void *)&s.slab, (void *)&s.valid, &lo, &hi, &d, (void *)&W, &nc, &cc0, &first, &tl, &th, &tpw, &best_s, &best_i};
    BN_HIP_TRY(hipLaunchKernel(scan_of((nc + 15) / 16), dim3(r.n_wg), dim3(256), args, SCAN_LDS, s.stream));
    return BN_OK;
}

// the exact assignment of the range under d_cent[0 .. k): ascending passes of CP centroids
bn_status enqueue_assign(AssignBufs *cs, const bn::IndexScan &s, const Range &r, size_t k) {
    for (size_t c0 = 0; c0 < k; c0 += CP) {
        bn_status st = enqueue_pass(cs, s, r, c0, (int)std::min<size_t>(CP, k - c0), c0 == 0);
        if (st != BN_OK) return st;
    }
    return check_launch("cluster scan");
}

bn_status enqueue_member_lists(const uint32_t *d_best_i, uint32_t id_lo, uint32_t id_hi, const uint32_t *d_counts, uint32_t k, uint32_t *d_offsets,
                               uint32_t *d_members, hipStream_t stream) {
    const uint64_t n = id_hi - id_lo;
    const uint32_t quarter = (uint32_t)(((n + 3) / 4 + 63) / 64 * 64);
    hipLaunchKernelGGL(cluster_offsets_kernel, dim3(1), dim3(64), 0, stream, d_counts, k, d_offsets);
    hipLaunchKernelGGL(cluster_members_kernel, dim3(k), dim3(256), 0, stream, d_best_i, id_lo, id_hi, quarter, d_offsets, d_members);
    return check_launch("cluster member lists");
}

}  // namespace cluster
}  // namespace bn

namespace {

using bn::cluster::check_finite;
using bn::cluster::enqueue_assign;
using bn::cluster::enqueue_pass;
using bn::cluster::range_of;
using bn::cluster::Range;
using bn::cluster::reserve_assign;
using bn::cluster::upload_centroids;

bn_status planes_to_host(bn::ClusterState *cs, const bn::IndexScan &s, const Range &r, uint32_t *assign_out, float *score_out) {
    const size_t n = r.id_hi - r.id_lo;
    BN_HIP_TRY(hipStreamSynchronize(s.stream));
    if (assign_out) BN_HIP_TRY(bn::gated::Memcpy(assign_out, cs->d_best_i + r.id_lo, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (score_out) BN_HIP_TRY(bn::gated::Memcpy(score_out, cs->d_best_s + r.id_lo, n * sizeof(float), hipMemcpyDeviceToHost));
    return BN_OK;
}

// the winning scores summed in id order in float64 (a row without a winner carries NaN and is left out)
double objective_of(const float *score, size_t n) {
    double sum = 0.0;
    for (size_t i = 0; i < n; i++)
        if (score[i] == score[i]) sum += (double)score[i];
    return sum;
}

struct ClusterOpts {
    uint32_t max_iters = 50;
    const uint64_t *init_ids = nullptr;
    const float *init_centroids = nullptr;
    uint64_t *start_ids_out = nullptr;
    double *objective_history = nullptr;
    size_t history_capacity = 0;
};

}  // namespace

extern "C" bn_status bn_index_assign(bn_index *x, const float *centroids, size_t k, uint64_t first_id, uint64_t n_ids, uint32_t *assign_out,
                                     float *score_out) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (!centroids || !assign_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    bn_status st = check_common(x, k, first_id, n_ids);
    if (st != BN_OK) return st;
    if ((st = check_finite(centroids, k * bn_index_dim(x), "centroids")) != BN_OK) return st;
    bn::IndexScan s;
    if ((st = bn::index_scan_state(x, &s)) != BN_OK) return st;
    const Range r = range_of(s, first_id, n_ids);
    if (r.id_lo == r.id_hi) return BN_OK;  // an empty index or an empty range
    bn::ClusterState *&cs = *bn::index_cluster_state(x);
    if (!cs) cs = new bn::ClusterState;
    if ((st = reserve_assign(cs, s, k)) != BN_OK) return st;
    if ((st = upload_centroids(cs, s, centroids, k)) != BN_OK) return st;
    if ((st = enqueue_assign(cs, s, r, k)) != BN_OK) return st;
    return planes_to_host(cs, s, r, assign_out, score_out);
}

extern "C" bn_status bn_index_cluster(bn_index *x, size_t k, uint64_t first_id, uint64_t n_ids, const bn_cluster_opts *opts, size_t opts_size,
                                      float *centroids_out, uint32_t *assign_out, float *score_out, uint32_t *counts_out, bn_cluster_report *report,
                                      size_t report_size) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (!centroids_out || !assign_out || !counts_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    bn_status st = check_common(x, k, first_id, n_ids);
    if (st != BN_OK) return st;
    ClusterOpts o;
    {
        bn_cluster_opts in{};
        if (opts) memcpy(&in, opts, std::min(opts_size, sizeof(in)));  // a shorter (older) struct leaves the rest at its defaults
        if (in.max_iters) o.max_iters = in.max_iters;
        o.init_ids = in.init_ids;
        o.init_centroids = in.init_centroids;
        o.start_ids_out = in.start_ids_out;
        o.objective_history = in.objective_history;
        o.history_capacity = in.objective_history ? in.history_capacity : 0;
    }
    if (o.init_ids && o.init_centroids) return set_last_error(BN_ERR_INVALID_ARG, "both init_ids and init_centroids are given");
    const size_t dim = bn_index_dim(x);
    if (o.init_centroids && (st = check_finite(o.init_centroids, k * dim, "init_centroids")) != BN_OK) return st;
    bn::IndexScan s;
    if ((st = bn::index_scan_state(x, &s)) != BN_OK) return st;
    const Range r = range_of(s, first_id, n_ids);
    const size_t n = r.id_hi - r.id_lo;
    // the range's validity bytes: the refusals that depend on them, and the first row of the max-min start
    std::vector<uint8_t> valid(n);
    BN_HIP_TRY(hipStreamSynchronize(s.stream));
    if (n) BN_HIP_TRY(bn::gated::Memcpy(valid.data(), s.valid + r.id_lo, n, hipMemcpyDeviceToHost));
    const size_t n_valid = (size_t)std::count_if(valid.begin(), valid.end(), [](uint8_t v) { return v != 0; });
    if (n_valid < k)
        return set_last_error(BN_ERR_INVALID_ARG, "the range holds " + std::to_string(n_valid) + " valid rows, fewer than k = " + std::to_string(k));
    std::vector<uint32_t> start(k);
    if (o.init_ids) {
        for (size_t c = 0; c < k; c++) {
            const uint64_t id = o.init_ids[c];
            if (id < r.id_lo || id >= r.id_hi) return set_last_error(BN_ERR_INVALID_ARG, "init id " + std::to_string(id) + " is outside the range");
            if (!valid[id - r.id_lo]) return set_last_error(BN_ERR_INVALID_ARG, "row " + std::to_string(id) + " of the index is stored as zeros (it had no direction)");
            start[c] = (uint32_t)id;
        }
        std::vector<uint32_t> sorted(start);
        std::sort(sorted.begin(), sorted.end());
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return set_last_error(BN_ERR_INVALID_ARG, "init_ids holds a duplicate");
    }

    bn::ClusterState *&cs = *bn::index_cluster_state(x);
    if (!cs) cs = new bn::ClusterState;
    if ((st = reserve_assign(cs, s, k)) != BN_OK) return st;
    const size_t rows = (s.size + TILE - 1) / TILE * TILE;
    if (rows > cs->list_n) {
        size_t a = cs->list_n, b = cs->list_n;
        BN_HIP_TRY(ensure(cs->d_prev_i, a, rows));
        BN_HIP_TRY(ensure(cs->d_members, b, rows));
        cs->list_n = rows;
    }
    if (!cs->d_small) BN_HIP_TRY(cs->d_small.alloc(SMALL_N * sizeof(uint32_t)));
    if (!cs->d_pick) BN_HIP_TRY(cs->d_pick.alloc(ARG_BLOCKS * sizeof(Pick)));
    const size_t dpad = s.dpad;
    const uint32_t slots = (uint32_t)std::max<size_t>(1, std::min<size_t>(64, PART_BYTES / (k * dpad * sizeof(double))));
    BN_HIP_TRY(ensure(cs->d_acc, cs->acc_n, k * dpad));
    BN_HIP_TRY(ensure(cs->d_part, cs->part_n, k * slots * dpad));
    uint32_t *d_counts = cs->d_small + SMALL_COUNTS, *d_offsets = cs->d_small + SMALL_OFFSETS, *d_scalars = cs->d_small + SMALL_SCALARS,
             *d_start = cs->d_small + SMALL_START;
    const uint32_t kk = (uint32_t)k, dp = (uint32_t)dpad, zb = (uint32_t)((dpad + 255) / 256);

    // ---- the first centroids
    if (o.init_centroids) {
        if ((st = upload_centroids(cs, s, o.init_centroids, k)) != BN_OK) return st;
    } else if (o.init_ids) {
        BN_HIP_TRY(bn::gated::Memcpy(d_start, start.data(), k * sizeof(uint32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(cluster_gather_kernel, dim3(kk), dim3(256), 0, s.stream, s.slab, d_start, dp, cs->d_cent);
        if ((st = check_launch("cluster gather")) != BN_OK) return st;
    } else {
        // max-min: the lowest valid id, then k - 1 times the row farthest (smallest running best) from the centroids so far
        start[0] = r.id_lo + (uint32_t)(std::find_if(valid.begin(), valid.end(), [](uint8_t v) { return v != 0; }) - valid.begin());
        BN_HIP_TRY(bn::gated::Memcpy(d_start, start.data(), sizeof(uint32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(cluster_gather_kernel, dim3(1), dim3(256), 0, s.stream, s.slab, d_start, dp, cs->d_cent);
        for (uint32_t j = 1; j < kk; j++) {
            if ((st = enqueue_pass(cs, s, r, j - 1, 1, j == 1)) != BN_OK) return st;
            if (j == 1) hipLaunchKernelGGL(cluster_mark_kernel, dim3(1), dim3(1), 0, s.stream, cs->d_best_s, start[0]);
            hipLaunchKernelGGL(cluster_argmin_kernel, dim3(ARG_BLOCKS), dim3(256), 0, s.stream, cs->d_best_s, cs->d_best_i, r.id_lo, r.id_hi, cs->d_pick);
            hipLaunchKernelGGL(cluster_pick_kernel, dim3(1), dim3(256), 0, s.stream, cs->d_pick, s.slab, dp, j, d_start, cs->d_cent, cs->d_best_s);
        }
        if ((st = check_launch("cluster start")) != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(s.stream));
        BN_HIP_TRY(bn::gated::Memcpy(start.data(), d_start, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < k; c++)
            if (start[c] == NONE) return set_last_error(BN_ERR_BACKEND, "the max-min start found no row for centroid " + std::to_string(c));
    }

    // ---- Lloyd: assign, [stop], update
    BN_HIP_TRY(hipMemsetAsync(cs->d_prev_i + r.id_lo, (int)(NEVER & 0xFF), n * sizeof(uint32_t), s.stream));
    std::vector<uint32_t> h_small(K_MAX + 2);
    std::vector<float> h_score;
    bn_cluster_report rep{};
    uint32_t *h_counts = h_small.data();
    for (;;) {
        if ((st = enqueue_assign(cs, s, r, k)) != BN_OK) return st;
        BN_HIP_TRY(hipMemsetAsync(d_counts, 0, k * sizeof(uint32_t), s.stream));
        BN_HIP_TRY(hipMemsetAsync(d_scalars, 0, sizeof(uint32_t), s.stream));
        hipLaunchKernelGGL(cluster_stats_kernel, dim3((unsigned)((n + STATS_ROWS - 1) / STATS_ROWS)), dim3(256), 0, s.stream, cs->d_best_i, cs->d_prev_i, r.id_lo,
                           r.id_hi, kk, d_counts, d_scalars);
        if ((st = check_launch("cluster stats")) != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(s.stream));
        BN_HIP_TRY(bn::gated::Memcpy(h_counts, d_counts, k * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint32_t moved = 0;
        BN_HIP_TRY(bn::gated::Memcpy(&moved, d_scalars, sizeof(uint32_t), hipMemcpyDeviceToHost));
        rep.moved_last = moved;
        if (rep.history_len < o.history_capacity) {
            h_score.resize(n);
            BN_HIP_TRY(bn::gated::Memcpy(h_score.data(), cs->d_best_s + r.id_lo, n * sizeof(float), hipMemcpyDeviceToHost));
            o.objective_history[rep.history_len++] = objective_of(h_score.data(), n);
        }
        if (rep.iters > 0 && moved == 0) {
            rep.converged = 1;
            break;
        }
        if (rep.iters >= o.max_iters) break;

        // the update: member lists, segment sums folded in order, the norm
        if ((st = bn::cluster::enqueue_member_lists(cs->d_best_i, r.id_lo, r.id_hi, d_counts, kk, d_offsets, cs->d_members, s.stream)) != BN_OK) return st;
        const uint32_t max_count = *std::max_element(h_counts, h_counts + k);
        const uint32_t n_seg = std::max<uint32_t>(1, (max_count + SEG - 1) / SEG);  // one round even for empty clusters: it zeroes acc
        for (uint32_t seg0 = 0; seg0 < n_seg; seg0 += slots) {
            hipLaunchKernelGGL(cluster_segsum_kernel, dim3(slots, kk, zb), dim3(256), 0, s.stream, s.slab, dp, cs->d_members, d_offsets, d_counts, seg0, slots,
                               cs->d_part);
            hipLaunchKernelGGL(cluster_fold_kernel, dim3(kk, zb), dim3(256), 0, s.stream, cs->d_part, dp, d_counts, seg0, slots, cs->d_acc);
        }
        BN_HIP_TRY(hipMemsetAsync(d_scalars + 1, 0, sizeof(uint32_t), s.stream));
        hipLaunchKernelGGL(cluster_finish_kernel, dim3(kk), dim3(256), 0, s.stream, cs->d_acc, dp, d_counts, cs->d_cent, d_scalars);
        if ((st = check_launch("cluster update")) != BN_OK) return st;
        rep.iters++;
    }
    // the last pass's planes are the exact assignment under d_cent; d_scalars[1] still holds the last update's kept centroids
    BN_HIP_TRY(bn::gated::Memcpy(&rep.empty_clusters, d_scalars + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    h_score.resize(n);
    BN_HIP_TRY(bn::gated::Memcpy(h_score.data(), cs->d_best_s + r.id_lo, n * sizeof(float), hipMemcpyDeviceToHost));
    rep.objective = objective_of(h_score.data(), n);
    std::vector<float> pad(k * dpad);
    BN_HIP_TRY(bn::gated::Memcpy(pad.data(), cs->d_cent, pad.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < k; c++) memcpy(centroids_out + c * dim, pad.data() + c * dpad, dim * sizeof(float));
    BN_HIP_TRY(bn::gated::Memcpy(assign_out, cs->d_best_i + r.id_lo, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (score_out) memcpy(score_out, h_score.data(), n * sizeof(float));
    memcpy(counts_out, h_counts, k * sizeof(uint32_t));
    if (o.start_ids_out && !o.init_centroids)
        for (size_t c = 0; c < k; c++) o.start_ids_out[c] = start[c];
    if (report) memcpy(report, &rep, std::min(report_size, sizeof(rep)));
    return BN_OK;
}
