// bn_ivf_* behind the C ABI (include/birdnet_hip.h): an inverted-file view of an index.  Centroids, the exact assignment of the
// covered rows and one member list per centroid; a search scores the query against the centroids, takes the nprobe best lists and
// scans only their rows, with the score bits, the order and the tie rule of bn_index_search.
//
// Build and extend run cluster.hip's assignment pass and member-list kernels (cluster_assign.h) on the view's own planes.
// Kernels of this file:
//   * ivf_count_kernel -- the lists' sizes from the assignment plane (integer atomics: exact in any order).
//   * ivf_probe_score_kernel -- [queries x k] centroid scores.  One wave per block of 16 centroids and 16 queries: query = A
//     operand, centroid = B operand of v_mfma_f32_16x16x4_f32, k = 16 s + 4 (lane >> 4) + t ascending, ONE accumulator per
//     (query, centroid), then + 0.0f: cluster_scan_kernel's chain with the query in the row's place.
//   * ivf_probe_select_kernel -- one workgroup per query: the k scores in LDS, every centroid's rank under (score descending,
//     index ascending, NaN left out) counted directly; rank < nprobe is a probe.  Also the probed lists' sizes summed.
//   * ivf_scan_kernel -- the gathered scan.  A unit is (query, probe slot, segment of that list); it reads its list from the probe
//     output on the device.  index_scan_kernel's tile loop with one query block of which column 0 is the query: row = A operand,
//     query = B operand, the same k order and accumulator, so a (query, row) score has bn_index_search's bits.  A tile's 64 rows
//     are 64 consecutive members of the list; the ids are fetched two tiles ahead, the row chunk one step ahead.  Lanes past the
//     list's end read its last member (a valid row) and are masked by position.  Wave 0 selects into a pending list and merges it
//     into the unit's sorted candidates (topm_select.h).
//   * ivf_merge_kernel -- one workgroup of 8 waves per query.  Wave w walks units w, w + 8, .. (unit order = probe order, so the
//     best list comes first and the threshold rejects early), the next list's head loaded while the current one is taken; then
//     wave 0 takes the other waves' lists the same way.  The order is strict and total, so the result does not depend on the split.
// ivf_scan_kernel and ivf_merge_kernel are also sq8.hip's re-rank and merges, through ivf_enqueue_scan / ivf_enqueue_merge (capi_internal.h).
// LDS: the scan takes 4.3 KB (two 128-float query chunks, 64 scores, 128 pending and 256 scratch candidates), the merge 40 KB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "cluster_assign.h"
#include "device_common.h"
#include "hip_gate.h"
#include "topm_select.h"

namespace {

constexpr int KC = 128;   // k-step: the slab's and the centroids' rows are padded to a multiple of it
constexpr int TILE = 64;  // rows per tile: 4 waves x 16 rows
constexpr int MERGE_WAVES = 8;
constexpr size_t UNIT_MAX = 16384;     // units per scan launch: 32 MB of candidates
constexpr uint32_t COUNT_ROWS = 4096;  // rows per block of ivf_count_kernel
constexpr uint32_t NONE = BN_CLUSTER_NONE;

using bn::cluster::K_MAX;
using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;  // the search's order: score descending, ties by id ascending

// counts[c] += rows of [0, n) assigned to c; counts is zero on entry
__global__ __launch_bounds__(256) void ivf_count_kernel(const uint32_t *__restrict__ best_i, uint32_t n, uint32_t k, uint32_t *__restrict__ counts) {
    __shared__ uint32_t hist[K_MAX];
    for (uint32_t c = threadIdx.x; c < k; c += 256) hist[c] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * COUNT_ROWS;
    for (uint32_t j = threadIdx.x; j < COUNT_ROWS; j += 256) {
        const uint64_t i = base + j;
        if (i >= n) break;
        const uint32_t b = best_i[i];
        if (b < k) atomicAdd(&hist[b], 1u);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < k; c += 256)
        if (hist[c]) atomicAdd(&counts[c], hist[c]);
}

// Block (x, y), wave w: centroids 16 (4 x + w) .., queries 16 y ...  Lane l: A = query 16 y + (l & 15), B = centroid .. + (l & 15),
// both at k = 16 s + 4 (l >> 4) + t; D: query 16 y + 4 (l >> 4) + reg, centroid .. + (l & 15).  Rows past nq / k read the last one.
__global__ __launch_bounds__(256) void ivf_probe_score_kernel(const float *__restrict__ q, uint32_t nq, const float *__restrict__ cent, uint32_t k,
                                                              uint32_t dpad, float *__restrict__ scores) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r16 = lane & 15, h = lane >> 4;
    const uint32_t c0 = (blockIdx.x * 4 + w) * 16, q0 = blockIdx.y * 16;
    if (c0 >= k) return;
    const float *ap = q + (size_t)min(q0 + r16, nq - 1) * dpad + 4 * h;
    const float *bp = cent + (size_t)min(c0 + r16, k - 1) * dpad + 4 * h;
    floatx4 acc{0.f, 0.f, 0.f, 0.f};
    for (uint32_t c = 0; c < dpad; c += KC) {
        float4 a[8], b[8];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            a[s] = *reinterpret_cast<const float4 *>(ap + c + 16 * s);
            b[s] = *reinterpret_cast<const float4 *>(bp + c + 16 * s);
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, b[s].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, b[s].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, b[s].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, b[s].w, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t qq = q0 + 4 * h + r, cc = c0 + r16;
        if (qq < nq && cc < k) scores[(size_t)qq * k + cc] = acc[r] + 0.0f;  // the head's bias add, with a bias of +0.0
    }
}

// Workgroup q: probes[q][0 .. nprobe) = the centroids of rank 0 .. nprobe - 1 under (score descending, index ascending; -0.0 == +0.0;
// a NaN has no rank), NONE in the slots no centroid reaches and in every slot of an invalid query; scanned[q] = their lists' sizes
__global__ __launch_bounds__(256) void ivf_probe_select_kernel(const float *__restrict__ scores, const uint8_t *__restrict__ qvalid, uint32_t k,
                                                               uint32_t nprobe, const uint32_t *__restrict__ counts, uint32_t *__restrict__ probes,
                                                               unsigned long long *__restrict__ scanned) {
    __shared__ float sc[K_MAX];
    __shared__ uint32_t sel[K_MAX];
    __shared__ unsigned long long total;
    const uint32_t q = blockIdx.x;
    for (uint32_t c = threadIdx.x; c < k; c += 256) sc[c] = scores[(size_t)q * k + c];
    for (uint32_t i = threadIdx.x; i < nprobe; i += 256) sel[i] = NONE;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    if (qvalid[q]) {
        for (uint32_t c = threadIdx.x; c < k; c += 256) {
            const float s = sc[c];
            if (!(s == s)) continue;
            uint32_t rank = 0;
            for (uint32_t j = 0; j < k; j++) {
                const float t = sc[j];
                rank += (t > s || (t == s && j < c)) ? 1u : 0u;
            }
            if (rank < nprobe) sel[rank] = c;
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nprobe; i += 256) {
        const uint32_t c = sel[i];
        probes[(size_t)q * nprobe + i] = c;
        if (c != NONE) atomicAdd(&total, (unsigned long long)counts[c]);
    }
    __syncthreads();
    if (threadIdx.x == 0) scanned[q] = total;
}

// Block (seg, p, qq): unit (qq * nprobe + p) * segments + seg scans tiles [seg * seg_tiles, + seg_tiles) of the list probes[qq][p]
// for query qq.  Tile t of a list of n members holds members [64 t, 64 t + 64); wave w, lane l multiplies member 64 t + 16 w + (l & 15)
// (clamped to n - 1).  D: lanes with (l & 15) == 0 hold the query's scores of members 64 t + 16 w + 4 (l >> 4) + reg.
// Out: cand[unit][..] sorted, cand_len[unit].  A unit with no list (NONE), or whose segment starts past the list's end, has length 0.
__global__ __launch_bounds__(256) void ivf_scan_kernel(const float *__restrict__ slab, uint32_t dpad, const float *__restrict__ q,
                                                       const uint32_t *__restrict__ qid, int64_t radius, int M, const uint32_t *__restrict__ probes,
                                                       uint32_t nprobe, const uint32_t *__restrict__ counts, const uint32_t *__restrict__ offsets,
                                                       const uint32_t *__restrict__ members, uint32_t seg_tiles, Cand *__restrict__ cand,
                                                       int *__restrict__ cand_len) {
    // one query column: 16 lanes of a wave write S, each to its own four words, so S needs no padded stride
    __shared__ __align__(16) float Qs[2][KC];  // the query's k chunk of this step and of the next
    __shared__ float S[TILE];                  // the tile's scores
    __shared__ Cand pend[PEND], scratch[MMAX];
    __shared__ Cand thr;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const uint32_t qq = blockIdx.z, p = blockIdx.y;
    const size_t unit = ((size_t)qq * nprobe + p) * gridDim.x + blockIdx.x;
    const uint32_t c = probes[(size_t)qq * nprobe + p];
    uint32_t n = 0, off = 0;
    if (c != NONE) {
        n = counts[c];
        off = offsets[c];
    }
    const uint32_t n_tiles = (n + TILE - 1) / TILE;  // n < 2^32 - 64
    const uint32_t t0 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)blockIdx.x * seg_tiles);
    const uint32_t t1 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)t0 + seg_tiles);
    if (t0 >= t1) {  // the same for every thread of the block
        if (tid == 0) cand_len[unit] = 0;
        return;
    }
    const uint32_t *list = members + off;  // n >= 1 members, each the id of a stored row
    const float *qrow = q + (size_t)qq * dpad;
    Cand *my_cand = cand + unit * MMAX;
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;
    const uint32_t last = n - 1;
    // the member this lane multiplies in tile t, clamped into the list
    auto member_of = [&](uint64_t t) { return list[min((uint64_t)last, t * TILE + w * 16 + r16)]; };

    uint32_t id_cur = member_of(t0), id_nx = member_of((uint64_t)t0 + 1), id_nn = id_nx;
    float4 a[8], qr = make_float4(0.f, 0.f, 0.f, 0.f);
    {
        const float *rp = slab + (size_t)id_cur * dpad + 4 * h;
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
        if (tid < KC / 4) *reinterpret_cast<float4 *>(&Qs[0][tid * 4]) = *reinterpret_cast<const float4 *>(qrow + tid * 4);
    }
    __syncthreads();
    floatx4 acc{0.f, 0.f, 0.f, 0.f};
    int L = 0, np = 0;  // wave 0's: the unit's list length and the pending count

    // step u = (tile t0 + u / nkc, chunk u % nkc); the row chunk and the query chunk of step u + 1 are loaded during step u
    for (uint32_t u = 0; u < steps; u++) {
        const uint32_t tl = u / nkc, ck = u % nkc;
        if (ck == 0) id_nn = member_of((uint64_t)t0 + tl + 2);
        float4 an[8];
        if (u + 1 < steps) {
            const uint32_t ck1 = ck + 1 == nkc ? 0 : ck + 1;
            const float *rp = slab + (size_t)(ck1 ? id_cur : id_nx) * dpad + ck1 * KC + 4 * h;
#pragma unroll
            for (int s = 0; s < 8; s++) an[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
            if (tid < KC / 4) qr = *reinterpret_cast<const float4 *>(qrow + ck1 * KC + tid * 4);
        }
        const float *Qc = Qs[u & 1];
#pragma unroll
        for (int s = 0; s < 8; s++) {
            float4 bq = *reinterpret_cast<const float4 *>(Qc + 16 * s + 4 * h);
            if (r16) bq = make_float4(0.f, 0.f, 0.f, 0.f);  // columns 1 .. 15 of the query block are empty
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, bq.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, bq.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, bq.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, bq.w, acc, 0, 0, 0);
        }
        if (u + 1 < steps) {
#pragma unroll
            for (int s = 0; s < 8; s++) a[s] = an[s];
            if (tid < KC / 4) *reinterpret_cast<float4 *>(&Qs[(u + 1) & 1][tid * 4]) = qr;
        }
        __syncthreads();  // the next chunk is in place; this chunk's reads, and the previous tile's selection, are done
        if (ck + 1 != nkc) continue;

        // ---- end of a tile: the query's scores to LDS, then wave 0 selects
        if (r16 == 0) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[w * 16 + h * 4 + r] = acc[r];
        }
        acc = floatx4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        if (w == 0) {
            const uint64_t pos = (uint64_t)(t0 + tl) * TILE + lane;
            bool ok = pos <= last;
            const uint32_t id = list[ok ? pos : last];
            if (radius >= 0) {
                const int64_t d = (int64_t)id - (int64_t)qid[qq];
                ok = ok && (d > radius || d < -radius);
            }
            const Cand e{S[lane], id};
            const bool pass = ok && (L < M || Ord::ahead(e, thr));
            const uint64_t m = __ballot(pass);
            if (m) {
                if (np + 64 > PEND) {
                    L = merge_pending<Ord>(pend, np, my_cand, L, M, scratch, &thr);
                    np = 0;
                }
                if (pass) pend[np + lanes_below(m)] = e;
                np += __popcll(m);
                wave_sync();
            }
        }
        id_cur = id_nx;
        id_nx = id_nn;
    }
    if (w == 0) {
        if (np) L = merge_pending<Ord>(pend, np, my_cand, L, M, scratch, &thr);
        if (lane == 0) cand_len[unit] = L;
    }
}

// One wave: the sorted list src (lg entries, the first 64 already in `head`) into the wave's running list through its pending list
__device__ inline void absorb_sorted(const Cand *src, int lg, Cand head, Cand *list, int &len, Cand *pend, int &np, Cand *scratch, Cand *thr, int M) {
    const int lane = threadIdx.x & 63;
    for (int j = 0; j < lg; j += 64) {
        const bool in = j + lane < lg;
        const Cand e = j ? (in ? src[j + lane] : Cand{0.f, 0u}) : head;
        const bool pass = in && (len < M || Ord::ahead(e, *thr));
        const uint64_t m = __ballot(pass);
        if (!m) break;  // the list is sorted: nothing after a rejected entry can pass
        if (np + 64 > PEND) {
            len = merge_pending<Ord>(pend, np, list, len, M, scratch, thr);
            np = 0;
        }
        if (pass) pend[np + lanes_below(m)] = e;
        np += __popcll(m);
        wave_sync();
    }
}

// Workgroup q: the query's `units` sorted lists cand[q * units + u][MMAX] (lengths cand_len) -> out[q][M], count[q]
__global__ __launch_bounds__(64 * MERGE_WAVES) void ivf_merge_kernel(const Cand *__restrict__ cand, const int *__restrict__ cand_len, int units, int M,
                                                                     Cand *__restrict__ out, uint32_t *__restrict__ count) {
    __shared__ Cand list[MERGE_WAVES][MMAX], scratch[MERGE_WAVES][MMAX], pend[MERGE_WAVES][PEND];
    __shared__ Cand thr[MERGE_WAVES];
    __shared__ int lens[MERGE_WAVES];
    const int q = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const Cand *qc = cand + (size_t)q * units * MMAX;
    const int *ql = cand_len + (size_t)q * units;
    int len = 0, np = 0;
    // the next unit's length and first 64 entries are in flight while the current unit is taken
    int lg_n = w < units ? ql[w] : 0;
    Cand head_n = lane < lg_n ? qc[(size_t)w * MMAX + lane] : Cand{0.f, 0u};
    for (int u = w; u < units; u += MERGE_WAVES) {
        const int lg = lg_n;
        const Cand head = head_n;
        const int un = u + MERGE_WAVES;
        lg_n = un < units ? ql[un] : 0;
        head_n = lane < lg_n ? qc[(size_t)un * MMAX + lane] : Cand{0.f, 0u};
        absorb_sorted(qc + (size_t)u * MMAX, lg, head, list[w], len, pend[w], np, scratch[w], &thr[w], M);
    }
    if (np) len = merge_pending<Ord>(pend[w], np, list[w], len, M, scratch[w], &thr[w]);
    if (lane == 0) lens[w] = len;
    __syncthreads();
    if (w) return;
    np = 0;
    for (int j = 1; j < MERGE_WAVES; j++) {
        const int lg = lens[j];
        const Cand head = lane < lg ? list[j][lane] : Cand{0.f, 0u};
        absorb_sorted(list[j], lg, head, list[0], len, pend[0], np, scratch[0], &thr[0], M);
    }
    if (np) len = merge_pending<Ord>(pend[0], np, list[0], len, M, scratch[0], &thr[0]);
    for (int i = lane; i < len; i += 64) out[(size_t)q * M + i] = list[0][i];
    if (lane == 0) count[q] = (uint32_t)len;
}

}  // namespace

struct bn_ivf {
    bn_index *x = nullptr;
    int device = 0;
    size_t k = 0, dim = 0, dpad = 0, covered = 0, cap_pad = 0, out_lists = 0;
    bn::cluster::AssignBufs ab;     // the centroids [k, dpad]; the assignment planes [cap_pad]
    bn::DeviceBuf<uint32_t> d_small;    // counts [k], offsets [k + 1]
    bn::DeviceBuf<uint32_t> d_members;  // [cap_pad]
    std::vector<uint32_t> h_counts, h_offsets;
    uint32_t max_count = 0;
    bn::DeviceBuf<float> d_pscore;                // [out_lists, k] centroid scores
    bn::DeviceBuf<uint32_t> d_probes;             // [out_lists, k] (a call uses [queries, nprobe])
    bn::DeviceBuf<unsigned long long> d_scanned;  // [out_lists]
    bn::DeviceBuf<Cand> d_cand;                   // [UNIT_MAX, MMAX]
    bn::DeviceBuf<int> d_cand_len;                // [UNIT_MAX]
    ~bn_ivf() { (void)bn::use_device(device); }
};

namespace {

using bn::check_launch;
using bn::set_last_error;

// assigns ids [from, size) (from a multiple of the tile) under the view's centroids, then rebuilds sizes, offsets and lists of [0, size)
// The device lists are rebuilt in place and the host mirrors follow at the end: after a failure in between the two disagree, and the
// view is good for bn_ivf_free only (the header says so)
bn_status cover(bn_ivf *v, const bn::IndexScan &s, size_t from) {
    const uint32_t k = (uint32_t)v->k, size = (uint32_t)s.size;
    uint32_t *d_counts = v->d_small, *d_offsets = v->d_small + k;
    bn_status st;
    if (from < s.size) {
        const bn::cluster::Range r = bn::cluster::range_of(s, from, s.size - from);
        if ((st = bn::cluster::enqueue_assign(&v->ab, s, r, k)) != BN_OK) return st;
    }
    BN_HIP_TRY(hipMemsetAsync(v->d_small, 0, (2 * (size_t)k + 1) * sizeof(uint32_t), s.stream));
    if (size) {
        hipLaunchKernelGGL(ivf_count_kernel, dim3((size + COUNT_ROWS - 1) / COUNT_ROWS), dim3(256), 0, s.stream, v->ab.d_best_i, size, k, d_counts);
        if ((st = check_launch("ivf count")) != BN_OK) return st;
        if ((st = bn::cluster::enqueue_member_lists(v->ab.d_best_i, 0, size, d_counts, k, d_offsets, v->d_members, s.stream)) != BN_OK) return st;
    }
    BN_HIP_TRY(hipStreamSynchronize(s.stream));
    std::vector<uint32_t> small(2 * (size_t)k + 1);
    BN_HIP_TRY(bn::gated::Memcpy(small.data(), v->d_small, small.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    v->h_counts.assign(small.begin(), small.begin() + k);
    v->h_offsets.assign(small.begin() + k, small.end());
    v->max_count = *std::max_element(v->h_counts.begin(), v->h_counts.end());
    v->covered = s.size;
    return BN_OK;
}

}  // namespace

bn_status bn::ivf_enqueue_scan(hipStream_t stream, const IvfGather &g, size_t n_queries, int M, topm::Cand *cand, int *cand_len) {
    hipLaunchKernelGGL(ivf_scan_kernel, dim3(g.segments, g.nprobe, (unsigned)n_queries), dim3(256), 0, stream, g.slab, g.dpad, g.q, g.qid, g.radius, M, g.probes,
                       g.nprobe, g.counts, g.offsets, g.members, g.seg_tiles, cand, cand_len);
    return check_launch("ivf scan");
}

bn_status bn::ivf_enqueue_merge(hipStream_t stream, const topm::Cand *cand, const int *cand_len, size_t n_queries, size_t units, int M, topm::Cand *out,
                                uint32_t *count) {
    hipLaunchKernelGGL(ivf_merge_kernel, dim3((unsigned)n_queries), dim3(64 * MERGE_WAVES), 0, stream, cand, cand_len, (int)units, M, out, count);
    return check_launch("ivf merge");
}

namespace {

// probe, scan and merge for the nq staged queries (nq <= out_lists); results into the index's pinned mirrors; synchronous
bn_status run_search(bn_ivf *v, const bn::IndexScan &s, size_t nq, const bn::StagedQueries &staged, size_t nprobe, int M) {
    const uint32_t k = (uint32_t)v->k, dpad = (uint32_t)v->dpad, np32 = (uint32_t)nprobe;
    const uint32_t *d_counts = v->d_small, *d_offsets = v->d_small + k;
    hipLaunchKernelGGL(ivf_probe_score_kernel, dim3((k + 63) / 64, (unsigned)((nq + 15) / 16)), dim3(256), 0, s.stream, staged.d_q, (uint32_t)nq, v->ab.d_cent, k,
                       dpad, v->d_pscore);
    hipLaunchKernelGGL(ivf_probe_select_kernel, dim3((unsigned)nq), dim3(256), 0, s.stream, v->d_pscore, staged.d_qvalid, k, np32, d_counts, v->d_probes,
                       v->d_scanned);
    bn_status st = check_launch("ivf probe");
    if (st != BN_OK) return st;
    // The split: every (query, probe slot) gets the same number of segments, sized for the largest list, since which lists are probed
    // is known on the device only.  Segments are as long as leaves about two units per compute unit; a launch holds at most UNIT_MAX
    // units, so many queries take several launches.
    const uint64_t max_tiles = std::max<uint64_t>(1, ((uint64_t)v->max_count + TILE - 1) / TILE);
    const uint64_t target = 2 * (uint64_t)std::max(1, s.max_wg);
    const uint64_t seg_tiles = std::min<uint64_t>(max_tiles, std::max<uint64_t>(1, (nq * nprobe * max_tiles + target - 1) / target));
    const uint32_t segments = (uint32_t)((max_tiles + seg_tiles - 1) / seg_tiles);
    const size_t per_query = nprobe * segments;  // <= 1024 + target
    if (per_query > UNIT_MAX) return set_last_error(BN_ERR_BACKEND, "ivf split: " + std::to_string(per_query) + " units per query");
    const size_t q_pass = UNIT_MAX / per_query;
    for (size_t p0 = 0; p0 < nq; p0 += q_pass) {
        const size_t n = std::min(q_pass, nq - p0);
        const bn::StagedQueries q = staged.at(p0);
        bn::IvfGather g;
        g.slab = s.slab;
        g.dpad = dpad;
        g.q = q.d_q;
        g.qid = q.d_qid;
        g.radius = q.radius;
        g.probes = v->d_probes + p0 * nprobe;
        g.nprobe = np32;
        g.counts = d_counts;
        g.offsets = d_offsets;
        g.members = v->d_members;
        g.seg_tiles = (uint32_t)seg_tiles;
        g.segments = segments;
        if ((st = bn::ivf_enqueue_scan(s.stream, g, n, M, v->d_cand, v->d_cand_len)) != BN_OK) return st;
        if ((st = bn::ivf_enqueue_merge(s.stream, v->d_cand, v->d_cand_len, n, per_query, M, s.d_out + p0 * M, s.d_count + p0)) != BN_OK) return st;
    }
    return bn::copy_back_results(s, nq, M);
}

bn_status search(bn_ivf *v, const bn::QuerySource &src, size_t n_queries, size_t nprobe, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                 uint32_t *count_out, uint32_t *probes_out, uint64_t *scanned_out) {
    bn_status st = bn::check_top_m(top_m, m_stride);
    if (st != BN_OK) return st;
    if ((st = bn::check_search_buffers(src.data(), n_queries, id_out, score_out, count_out)) != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    if (nprobe < 1 || nprobe > v->k) return set_last_error(BN_ERR_INVALID_ARG, "nprobe must be in 1.." + std::to_string(v->k) + ", got " + std::to_string(nprobe));
    if ((st = bn::check_query_ids(src, n_queries, v->covered, bn::IdLimit::VIEW)) != BN_OK) return st;
    bn::IndexScan s;
    if ((st = bn::index_scan_state(v->x, &s)) != BN_OK) return st;
    return bn::for_each_round(v->x, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) -> bn_status {
        if (bn_status rs = run_search(v, s, nq, staged, nprobe, (int)top_m); rs != BN_OK) return rs;
        bn::scatter_results(s, q0, nq, top_m, m_stride, id_out, score_out, count_out);
        if (probes_out) BN_HIP_TRY(bn::gated::Memcpy(probes_out + q0 * nprobe, v->d_probes, nq * nprobe * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (scanned_out) BN_HIP_TRY(bn::gated::Memcpy(scanned_out + q0, v->d_scanned, nq * sizeof(uint64_t), hipMemcpyDeviceToHost));
        return BN_OK;
    });
}

}  // namespace

extern "C" {

bn_status bn_ivf_build(bn_index *x, const float *centroids, size_t k, bn_ivf **out) {
    if (!out || !centroids) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (k < 1 || k > K_MAX) return set_last_error(BN_ERR_INVALID_ARG, "k must be in 1..1024, got " + std::to_string(k));
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    bn_status st = bn::cluster::check_finite(centroids, k * bn_index_dim(x), "centroids");
    if (st != BN_OK) return st;
    bn::IndexScan s;
    if ((st = bn::index_scan_state(x, &s)) != BN_OK) return st;
    auto v = std::make_unique<bn_ivf>();
    v->x = x;
    v->device = s.device;
    v->k = k;
    v->dim = s.dim;
    v->dpad = s.dpad;
    v->cap_pad = s.cap_pad;
    v->out_lists = s.out_lists;
    BN_HIP_TRY(v->ab.d_cent.alloc(k * s.dpad * sizeof(float)));
    v->ab.cent_n = k * s.dpad;
    BN_HIP_TRY(v->ab.d_best_s.alloc(s.cap_pad * sizeof(float)));
    BN_HIP_TRY(v->ab.d_best_i.alloc(s.cap_pad * sizeof(uint32_t)));
    v->ab.best_n = s.cap_pad;
    BN_HIP_TRY(v->d_small.alloc((2 * k + 1) * sizeof(uint32_t)));
    BN_HIP_TRY(v->d_members.alloc(s.cap_pad * sizeof(uint32_t)));
    BN_HIP_TRY(v->d_pscore.alloc(s.out_lists * k * sizeof(float)));
    BN_HIP_TRY(v->d_probes.alloc(s.out_lists * k * sizeof(uint32_t)));
    BN_HIP_TRY(v->d_scanned.alloc(s.out_lists * sizeof(unsigned long long)));
    BN_HIP_TRY(v->d_cand.alloc(UNIT_MAX * MMAX * sizeof(Cand)));
    BN_HIP_TRY(v->d_cand_len.alloc(UNIT_MAX * sizeof(int)));
    if ((st = bn::cluster::upload_centroids(&v->ab, s, centroids, k)) != BN_OK) return st;
    if ((st = cover(v.get(), s, 0)) != BN_OK) return st;
    *out = v.release();
    return BN_OK;
}

void bn_ivf_free(bn_ivf *v) { delete v; }

size_t bn_ivf_lists(const bn_ivf *v) { return v ? v->k : 0; }
size_t bn_ivf_rows(const bn_ivf *v) { return v ? v->covered : 0; }

bn_status bn_ivf_extend(bn_ivf *v) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    bn::IndexScan s;
    bn_status st = bn::index_scan_state(v->x, &s);
    if (st != BN_OK) return st;
    if (s.size == v->covered) return BN_OK;
    // from the tile that holds the first new row: the pass writes whole tiles, and a covered row's assignment comes out the same
    return cover(v, s, v->covered / TILE * TILE);
}

bn_status bn_ivf_list_sizes(const bn_ivf *v, uint32_t *sizes_out) {
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    if (!sizes_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    memcpy(sizes_out, v->h_counts.data(), v->k * sizeof(uint32_t));
    return BN_OK;
}

bn_status bn_ivf_read_list(const bn_ivf *v, size_t list, uint64_t *ids_out, size_t cap, size_t *n_out) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    if (!n_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (list >= v->k) return set_last_error(BN_ERR_INVALID_ARG, "list " + std::to_string(list) + " of " + std::to_string(v->k));
    const size_t n = v->h_counts[list];
    *n_out = n;
    if (cap < n) return set_last_error(BN_ERR_INVALID_ARG, "the list holds " + std::to_string(n) + " ids, the buffer " + std::to_string(cap));
    if (!n) return BN_OK;
    if (!ids_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    BN_HIP_TRY(bn::use_device(v->device));
    std::vector<uint32_t> ids(n);
    BN_HIP_TRY(bn::gated::Memcpy(ids.data(), v->d_members + v->h_offsets[list], n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::copy(ids.begin(), ids.end(), ids_out);
    return BN_OK;
}

bn_status bn_ivf_search(bn_ivf *v, const float *queries, size_t n_queries, size_t nprobe, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                        uint32_t *count_out, uint32_t *probes_out, uint64_t *scanned_out) {
    if (n_queries && !queries) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return search(v, bn::QuerySource::host(queries), n_queries, nprobe, top_m, m_stride, id_out, score_out, count_out, probes_out, scanned_out);
}

bn_status bn_ivf_search_ids(bn_ivf *v, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t nprobe, size_t top_m, size_t m_stride,
                            uint64_t *id_out, float *score_out, uint32_t *count_out, uint32_t *probes_out, uint64_t *scanned_out) {
    if (n_queries && !query_ids) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return search(v, bn::QuerySource::stored(query_ids, exclude_radius), n_queries, nprobe, top_m, m_stride, id_out, score_out, count_out, probes_out,
                  scanned_out);
}

}  // extern "C"
