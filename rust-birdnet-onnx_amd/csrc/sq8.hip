// bn_sq8_* behind the C ABI (include/birdnet_hip.h): an int8 view of an index.  One code byte per slab element and one f32 scale per
// row; a search ranks every covered row by an exact integer key, keeps the `refine` best per query and re-scores those with the
// gathered scan of ivf.hip, so the returned scores, order and ties are bn_index_search's over the candidates.
//
// Kernels of this file:
//   * sq8_encode_kernel -- one wave per row: max |r[k]| by a wave reduction (a maximum has no order), inv = 127 / a, the codes
//     clamp(rint(r[k] * inv)) packed sixteen to a 16-byte store, pad columns and invalid rows zero, scale = a / 127.  Build, extend
//     (from the first uncovered row) and the staged queries of a search all go through it.
//   * sq8_scan_kernel -- the coarse scan on v_mfma_i32_16x16x64_i8.  Each workgroup streams its contiguous range of 64-row tiles once
//     for the pass's queries (up to 64): row = A operand, query = B operand, lane l holds bytes [64 s + 16 (l >> 4), + 16) of its row
//     and of its query for the s-th instruction of a row.  Which k a byte lands on inside the instruction does not matter: both
//     operands use the same map and an int32 sum has no order.  D is the dtype-independent map: query 16 qb + (l & 15), row
//     16 w + 4 (l >> 4) + reg.  A tile's keys (float)D * scale go to LDS (two buffers, one barrier per tile), ineligible rows are
//     masked there, and selection is index_scan_kernel's: pending lists merged into the workgroup's sorted running list
//     (topm_select.h).  Rows are loaded two 128-byte steps ahead and queries one step ahead, straight from global memory (the
//     queries' codes stay in cache), so the k loop has no barrier.  Out: cand[query][workgroup][256], the layout ivf_merge_kernel
//     takes, which merges them (8 waves per query).
//   * sq8_members_kernel -- the merged candidates' ids as one member list per query for the re-rank.
// LDS of the scan: 16 QB queries x (2 x 65 keys + 128 pending candidates) + 4 x 256 scratch candidates: 33 152 B at QB = 1, 108 032 B at
// QB = 4 (opted in per device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "topm_select.h"

namespace {

constexpr int KC = 128;        // bytes of a row per step: two MFMA instructions of k = 64
constexpr int TILE = 64;       // rows per tile: 4 waves x 16 rows
constexpr int QP = 64;         // queries per scan pass
constexpr int S_LD = TILE + 1;
constexpr int WG_PER_CU = 2;   // scan workgroups per compute unit
constexpr int RR_SEG = 4;      // re-rank units per query: one per tile of the 256 candidates at most
constexpr size_t DIM_MAX = 131072;  // 127^2 * dim < 2^31

using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;  // key descending, ties by id ascending

typedef int intx4 __attribute__((ext_vector_type(4)));

constexpr size_t scan_lds(int qb) {
    return (size_t)qb * 16 * (2 * S_LD * 4 + PEND * sizeof(Cand) + sizeof(Cand) + 2 * sizeof(int)) + 4 * MMAX * sizeof(Cand);
}

__device__ inline uint32_t code_of(float v, float inv, bool keep) {
    const float c = fminf(fmaxf(rintf(v * inv), -127.0f), 127.0f);
    return keep ? ((uint32_t)(int)c & 0xffu) : 0u;
}

// rows [n, dpad] (as the index stores them: pad columns zero) + valid [n] -> codes [n, dpad] + scales [n]
__global__ __launch_bounds__(256) void sq8_encode_kernel(const float *__restrict__ rows, const uint8_t *__restrict__ valid, uint32_t n, uint32_t dim,
                                                         uint32_t dpad, int8_t *__restrict__ codes, float *__restrict__ scales) {
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= n) return;
    const float *x = rows + (size_t)r * dpad;
    float a = 0.f;
    for (uint32_t k = lane * 4; k < dpad; k += 256) {
        const float4 v = *reinterpret_cast<const float4 *>(x + k);
        a = fmaxf(a, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
    }
    for (int off = 32; off; off >>= 1) a = fmaxf(a, __shfl_xor(a, off));
    const bool ok = valid[r] != 0 && a > 0.f;
    const float inv = ok ? __fdiv_rn(127.0f, a) : 0.f;
    for (uint32_t k0 = lane * 16; k0 < dpad; k0 += 1024) {
        uint32_t wd[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t k = k0 + 4 * j;
            const float4 v = *reinterpret_cast<const float4 *>(x + k);
            wd[j] = code_of(v.x, inv, ok && k < dim) | code_of(v.y, inv, ok && k + 1 < dim) << 8 | code_of(v.z, inv, ok && k + 2 < dim) << 16 |
                    code_of(v.w, inv, ok && k + 3 < dim) << 24;
        }
        *reinterpret_cast<uint4 *>(codes + (size_t)r * dpad + k0) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
    }
    if (lane == 0) scales[r] = ok ? __fdiv_rn(a, 127.0f) : 0.f;
}

// Scan of one pass (nq <= QP queries, QB = ceil(nq / 16) query blocks).  Workgroup g owns tiles [g * tiles_per_wg, ..) of the n_rows
// covered rows; the planes hold whole tiles.  Out: cand[(qq * gridDim.x + g)][..] sorted, the first M kept, cand_len[qq * gridDim.x + g].
template <int QB>
__global__ __launch_bounds__(256) void sq8_scan_kernel(const int8_t *__restrict__ codes, const float *__restrict__ scales, const uint8_t *__restrict__ valid,
                                                       uint32_t n_rows, uint32_t dpad, const int8_t *__restrict__ qcodes, const uint8_t *__restrict__ qvalid,
                                                       int nq, const uint32_t *__restrict__ qid, int64_t radius, int M, uint32_t tiles_per_wg,
                                                       Cand *__restrict__ cand, int *__restrict__ cand_len) {
    constexpr int NQ = QB * 16;
    extern __shared__ __align__(16) float sq8_lds[];
    float *S = sq8_lds;                                          // [2][NQ][S_LD]: the keys of this tile and of the previous one
    Cand *pend = reinterpret_cast<Cand *>(S + 2 * NQ * S_LD);    // [NQ][PEND]
    Cand *scratch = pend + NQ * PEND;                            // [4][MMAX]
    Cand *thr = scratch + 4 * MMAX;                              // [NQ]
    int *len = reinterpret_cast<int *>(thr + NQ);                // [NQ]
    int *pn = len + NQ;                                          // [NQ]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < NQ; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    const uint32_t n_tiles = (n_rows + TILE - 1) / TILE;
    const uint32_t t0 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)blockIdx.x * tiles_per_wg);
    const uint32_t t1 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;

    // in 16-byte units: a step is 8 of them, this lane's two are h and 4 + h
    const intx4 *rbase = reinterpret_cast<const intx4 *>(codes + ((size_t)t0 * TILE + w * 16 + r16) * dpad) + h;
    const size_t tile_stride = (size_t)TILE * dpad / 16;
    const intx4 *qbase[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) qbase[b] = reinterpret_cast<const intx4 *>(qcodes + (size_t)min(b * 16 + r16, nq - 1) * dpad) + h;

    uint32_t tlp = 0, ckp = 0;  // the step the row loads have reached
    auto load_a = [&](intx4 *a) {
        const intx4 *p = rbase + tlp * tile_stride + ckp * 8;
        a[0] = p[0];
        a[1] = p[4];
        if (++ckp == nkc) {
            ckp = 0;
            tlp++;
        }
    };
    auto load_q = [&](uint32_t ck, intx4(*q)[2]) {
#pragma unroll
        for (int b = 0; b < QB; b++) {
            q[b][0] = qbase[b][ck * 8];
            q[b][1] = qbase[b][ck * 8 + 4];
        }
    };
    const intx4 zero{0, 0, 0, 0};
    intx4 a0[2] = {zero, zero}, a1[2] = {zero, zero}, a2[2] = {zero, zero}, qc[QB][2], qn[QB][2];
#pragma unroll
    for (int b = 0; b < QB; b++) qc[b][0] = qc[b][1] = qn[b][0] = qn[b][1] = zero;
    if (steps) {
        load_a(a0);
        load_q(0, qc);
    }
    if (steps > 1) load_a(a1);
    intx4 acc[QB][2];
#pragma unroll
    for (int b = 0; b < QB; b++) acc[b][0] = acc[b][1] = zero;

    uint32_t tl = 0, ck = 0;
    for (uint32_t u = 0; u < steps; u++) {
        const uint32_t ck1 = ck + 1 == nkc ? 0 : ck + 1;
        if (u + 1 < steps) load_q(ck1, qn);  // before the row loads: its wait leaves them in flight
        if (u + 2 < steps) load_a(a2);
#pragma unroll
        for (int half = 0; half < 2; half++) {
#pragma unroll
            for (int b = 0; b < QB; b++) acc[b][half] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0[half], qc[b][half], acc[b][half], 0, 0, 0);
        }
#pragma unroll
        for (int half = 0; half < 2; half++) {
            a0[half] = a1[half];
            a1[half] = a2[half];
#pragma unroll
            for (int b = 0; b < QB; b++) qc[b][half] = qn[b][half];
        }
        ck = ck1;
        if (ck1) continue;

        // ---- end of a tile: keys to LDS, then selection (wave w owns queries w, w + 4, ...)
        const uint32_t t = t0 + tl;
        tl++;
        float *St = S + (t & 1) * NQ * S_LD;
        const float4 sc = *reinterpret_cast<const float4 *>(scales + (size_t)t * TILE + w * 16 + h * 4);
        const float scr[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
        for (int b = 0; b < QB; b++) {
            const intx4 d = acc[b][0] + acc[b][1];
#pragma unroll
            for (int r = 0; r < 4; r++) St[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = (float)d[r] * scr[r];
            acc[b][0] = acc[b][1] = zero;
        }
        __syncthreads();  // this tile's keys are in place; the buffer written next was read before the previous barrier
        const uint32_t grow = t * TILE + lane;
        const bool row_ok = grow < n_rows && valid[grow];
        for (int qq = w; qq < nq; qq += 4) {
            if (!qvalid[qq]) continue;
            bool ok = row_ok;
            if (radius >= 0) {
                const int64_t d = (int64_t)grow - (int64_t)qid[qq];
                ok = ok && (d > radius || d < -radius);
            }
            const Cand e{St[qq * S_LD + lane], grow};
            Cand *my_cand = cand + ((size_t)qq * gridDim.x + blockIdx.x) * MMAX;
            int L = len[qq];
            const bool pass = ok && (L < M || Ord::ahead(e, thr[qq]));
            const uint64_t m = __ballot(pass);
            if (!m) continue;
            int np = pn[qq];
            if (np + 64 > PEND) {
                L = merge_pending<Ord>(pend + qq * PEND, np, my_cand, L, M, scratch + w * MMAX, thr + qq);
                np = 0;
            }
            if (pass) pend[qq * PEND + np + lanes_below(m)] = e;
            wave_sync();
            if (lane == 0) {
                len[qq] = L;
                pn[qq] = np + __popcll(m);
            }
            wave_sync();
        }
    }
    __syncthreads();
    for (int qq = w; qq < nq; qq += 4) {
        Cand *my_cand = cand + ((size_t)qq * gridDim.x + blockIdx.x) * MMAX;
        int L = len[qq];
        const int np = pn[qq];
        if (np) L = merge_pending<Ord>(pend + qq * PEND, np, my_cand, L, M, scratch + w * MMAX, thr + qq);
        if (lane == 0) cand_len[(size_t)qq * gridDim.x + blockIdx.x] = L;
    }
}

// members[q][0 .. count[q]) = the ids of coarse[q][0 .. count[q]) (coarse rows of `refine`, member rows of MMAX)
__global__ __launch_bounds__(256) void sq8_members_kernel(const Cand *__restrict__ coarse, const uint32_t *__restrict__ count, uint32_t refine,
                                                          uint32_t *__restrict__ members) {
    const uint32_t q = blockIdx.x, n = count[q];
    for (uint32_t i = threadIdx.x; i < n; i += 256) members[(size_t)q * MMAX + i] = coarse[(size_t)q * refine + i].id;
}

bn::LdsOptIn g_scan_lds;

}  // namespace

struct bn_sq8 {
    bn_index *x = nullptr;
    int device = 0;
    size_t dim = 0, dpad = 0, covered = 0, cap_pad = 0, out_lists = 0, wg_max = 0;
    bn::DeviceBuf<int8_t> d_codes;    // [cap_pad, dpad]
    bn::DeviceBuf<float> d_scales;    // [cap_pad]
    bn::DeviceBuf<int8_t> d_qcodes;   // [out_lists, dpad]
    bn::DeviceBuf<float> d_qscales;   // [out_lists]: written, never read (the query's scale is left out of the key)
    bn::DeviceBuf<Cand> d_cand;       // the scan's [QP, wg_max, MMAX], then the re-rank's [out_lists * RR_SEG, MMAX]
    bn::DeviceBuf<int> d_cand_len;
    bn::DeviceBuf<Cand> d_coarse;     // [out_lists, refine]
    bn::DeviceBuf<uint32_t> d_ccount;   // [out_lists]
    bn::DeviceBuf<uint32_t> d_members;  // [out_lists, MMAX]
    bn::DeviceBuf<uint32_t> d_lists;    // [2, out_lists]: q -> q (the list a query "probes"), q -> q * MMAX (its offset)
    ~bn_sq8() { (void)bn::use_device(device); }
};

namespace {

using bn::check_launch;
using bn::set_last_error;

// codes and scales of rows [from, size) on the index's stream, then waits: the view covers [0, size)
bn_status cover(bn_sq8 *v, const bn::IndexScan &s, size_t from) {
    if (from < s.size) {
        const size_t n = s.size - from;
        hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s.stream, s.slab + from * s.dpad, s.valid + from, (uint32_t)n,
                           (uint32_t)s.dim, (uint32_t)s.dpad, v->d_codes + from * s.dpad, v->d_scales + from);
        if (bn_status st = check_launch("sq8 encode"); st != BN_OK) return st;
    }
    BN_HIP_TRY(hipStreamSynchronize(s.stream));
    v->covered = s.size;
    return BN_OK;
}

bn_status check_search_args(size_t n_queries, size_t refine, size_t top_m, size_t m_stride, const void *queries, const uint64_t *id_out,
                            const float *score_out, const uint32_t *count_out) {
    if (refine < 1 || refine > (size_t)MMAX) return set_last_error(BN_ERR_INVALID_ARG, "refine must be in 1..256, got " + std::to_string(refine));
    if (top_m < 1 || top_m > refine)
        return set_last_error(BN_ERR_INVALID_ARG, "top_m must be in 1..refine (" + std::to_string(refine) + "), got " + std::to_string(top_m));
    if (bn_status st = bn::check_top_m(top_m, m_stride); st != BN_OK) return st;  // top_m <= refine <= 256: the stride's refusal
    return bn::check_search_buffers(queries, n_queries, id_out, score_out, count_out);
}

template <int QB>
void launch_scan(const bn_sq8 *v, const bn::IndexScan &s, uint32_t n_wg, uint32_t tpw, size_t p0, int np, const bn::StagedQueries &q, int R) {
    hipLaunchKernelGGL(sq8_scan_kernel<QB>, dim3(n_wg), dim3(256), scan_lds(QB), s.stream, v->d_codes, v->d_scales, s.valid, (uint32_t)v->covered,
                       (uint32_t)v->dpad, v->d_qcodes + p0 * v->dpad, q.d_qvalid, np, q.d_qid, q.radius, R, tpw, v->d_cand, v->d_cand_len);
}

// encode, coarse scan + merge, re-rank + merge for the nq staged queries (nq <= out_lists, covered > 0); results into the index's pinned
// mirrors, candidates left in d_members / d_ccount; synchronous
bn_status run_search(bn_sq8 *v, const bn::IndexScan &s, size_t nq, const bn::StagedQueries &staged, int R, int M) {
    hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s.stream, staged.d_q, staged.d_qvalid, (uint32_t)nq, (uint32_t)v->dim,
                       (uint32_t)v->dpad, v->d_qcodes, v->d_qscales);
    bn_status st = check_launch("sq8 encode");
    if (st != BN_OK) return st;
    const bn::WgSplit sp = bn::split_tiles((uint32_t)((v->covered + TILE - 1) / TILE), v->wg_max);
    const uint32_t tpw = sp.tiles_per_wg, n_wg = sp.n_wg;
    for (size_t p0 = 0; p0 < nq; p0 += QP) {
        const int np = (int)std::min<size_t>(QP, nq - p0);
        bn::by_blocks(np, [&](auto qb) { launch_scan<decltype(qb)::value>(v, s, n_wg, tpw, p0, np, staged.at(p0), R); });
        if ((st = check_launch("sq8 scan")) != BN_OK) return st;
        if ((st = bn::ivf_enqueue_merge(s.stream, v->d_cand, v->d_cand_len, (size_t)np, n_wg, R, v->d_coarse + p0 * R, v->d_ccount + p0)) != BN_OK) return st;
    }
    hipLaunchKernelGGL(sq8_members_kernel, dim3((unsigned)nq), dim3(256), 0, s.stream, v->d_coarse, v->d_ccount, (uint32_t)R, v->d_members);
    if ((st = check_launch("sq8 members")) != BN_OK) return st;
    // the re-rank: IVF's gathered scan with one list per query, the candidates in coarse order, one unit per tile of 64
    bn::IvfGather g;
    g.slab = s.slab;
    g.dpad = (uint32_t)v->dpad;
    g.q = staged.d_q;
    g.probes = v->d_lists;
    g.nprobe = 1;
    g.counts = v->d_ccount;
    g.offsets = v->d_lists + v->out_lists;
    g.members = v->d_members;
    g.seg_tiles = 1;
    g.segments = (uint32_t)((R + TILE - 1) / TILE);
    if ((st = bn::ivf_enqueue_scan(s.stream, g, nq, M, v->d_cand, v->d_cand_len)) != BN_OK) return st;
    if ((st = bn::ivf_enqueue_merge(s.stream, v->d_cand, v->d_cand_len, nq, g.segments, M, s.d_out, s.d_count)) != BN_OK) return st;
    return bn::copy_back_results(s, nq, M);
}

bn_status search(bn_sq8 *v, const bn::QuerySource &src, size_t n_queries, size_t refine, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                 uint32_t *count_out, uint64_t *cand_out, uint32_t *cand_count_out) {
    bn_status st = check_search_args(n_queries, refine, top_m, m_stride, src.data(), id_out, score_out, count_out);
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    if ((st = bn::check_query_ids(src, n_queries, v->covered, bn::IdLimit::VIEW)) != BN_OK) return st;
    bn::IndexScan s;
    if ((st = bn::index_scan_state(v->x, &s)) != BN_OK) return st;
    if (v->covered == 0) {  // no launch
        std::fill(count_out, count_out + n_queries, 0u);
        if (cand_count_out) std::fill(cand_count_out, cand_count_out + n_queries, 0u);
        return BN_OK;
    }
    std::vector<uint32_t> members, ccount;
    return bn::for_each_round(v->x, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) -> bn_status {
        if (bn_status rs = run_search(v, s, nq, staged, (int)refine, (int)top_m); rs != BN_OK) return rs;
        bn::scatter_results(s, q0, nq, top_m, m_stride, id_out, score_out, count_out);
        if (!cand_out && !cand_count_out) return BN_OK;
        ccount.resize(nq);
        BN_HIP_TRY(bn::gated::Memcpy(ccount.data(), v->d_ccount, nq * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (cand_count_out) std::copy(ccount.begin(), ccount.end(), cand_count_out + q0);
        if (cand_out) {
            members.resize(nq * MMAX);
            BN_HIP_TRY(bn::gated::Memcpy(members.data(), v->d_members, nq * MMAX * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < nq; i++)
                for (uint32_t j = 0; j < ccount[i]; j++) cand_out[(q0 + i) * refine + j] = members[i * MMAX + j];
        }
        return BN_OK;
    });
}

}  // namespace

extern "C" {

bn_status bn_sq8_build(bn_index *x, bn_sq8 **out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (bn_index_dim(x) > DIM_MAX)
        return set_last_error(BN_ERR_INVALID_ARG, "dim " + std::to_string(bn_index_dim(x)) + " is above 131072: the int32 key could overflow");
    bn::IndexScan s;
    bn_status st = bn::index_scan_state(x, &s);
    if (st != BN_OK) return st;
    BN_HIP_TRY(g_scan_lds.prepare(s.device, {{(const void *)sq8_scan_kernel<1>, scan_lds(1)}, {(const void *)sq8_scan_kernel<2>, scan_lds(2)},
                                             {(const void *)sq8_scan_kernel<3>, scan_lds(3)}, {(const void *)sq8_scan_kernel<4>, scan_lds(4)}}));
    auto v = std::make_unique<bn_sq8>();
    v->x = x;
    v->device = s.device;
    v->dim = s.dim;
    v->dpad = s.dpad;
    v->cap_pad = s.cap_pad;
    v->out_lists = s.out_lists;
    v->wg_max = (size_t)WG_PER_CU * std::max(1, s.max_wg);
    const size_t units = std::max((size_t)QP * v->wg_max, s.out_lists * RR_SEG);
    BN_HIP_TRY(v->d_codes.alloc(s.cap_pad * s.dpad));
    BN_HIP_TRY(v->d_scales.alloc(s.cap_pad * sizeof(float)));
    BN_HIP_TRY(v->d_qcodes.alloc(s.out_lists * s.dpad));
    BN_HIP_TRY(v->d_qscales.alloc(s.out_lists * sizeof(float)));
    BN_HIP_TRY(v->d_cand.alloc(units * MMAX * sizeof(Cand)));
    BN_HIP_TRY(v->d_cand_len.alloc(units * sizeof(int)));
    BN_HIP_TRY(v->d_coarse.alloc(s.out_lists * MMAX * sizeof(Cand)));
    BN_HIP_TRY(v->d_ccount.alloc(s.out_lists * sizeof(uint32_t)));
    BN_HIP_TRY(v->d_members.alloc(s.out_lists * MMAX * sizeof(uint32_t)));
    BN_HIP_TRY(v->d_lists.alloc(2 * s.out_lists * sizeof(uint32_t)));
    // rows past the covered ones are read by the scan a whole tile at a time and masked by position: they hold zeros
    BN_HIP_TRY(bn::gated::Memset(v->d_codes, 0, s.cap_pad * s.dpad));
    BN_HIP_TRY(bn::gated::Memset(v->d_scales, 0, s.cap_pad * sizeof(float)));
    std::vector<uint32_t> lists(2 * s.out_lists);
    for (size_t q = 0; q < s.out_lists; q++) {
        lists[q] = (uint32_t)q;
        lists[s.out_lists + q] = (uint32_t)(q * MMAX);
    }
    BN_HIP_TRY(bn::gated::Memcpy(v->d_lists, lists.data(), lists.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    if ((st = cover(v.get(), s, 0)) != BN_OK) return st;
    *out = v.release();
    return BN_OK;
}

void bn_sq8_free(bn_sq8 *v) { delete v; }

size_t bn_sq8_rows(const bn_sq8 *v) { return v ? v->covered : 0; }

bn_status bn_sq8_extend(bn_sq8 *v) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    bn::IndexScan s;
    bn_status st = bn::index_scan_state(v->x, &s);
    if (st != BN_OK) return st;
    if (s.size == v->covered) return BN_OK;
    return cover(v, s, v->covered);
}

bn_status bn_sq8_read(const bn_sq8 *v, uint64_t first, size_t count, int8_t *codes_out, float *scales_out) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!v) return set_last_error(BN_ERR_INVALID_ARG, "null view");
    if (first > v->covered || count > v->covered - first) return set_last_error(BN_ERR_INVALID_ARG, "rows out of range");
    if (!count) return BN_OK;
    BN_HIP_TRY(bn::use_device(v->device));
    if (scales_out) BN_HIP_TRY(bn::gated::Memcpy(scales_out, v->d_scales + first, count * sizeof(float), hipMemcpyDeviceToHost));
    if (codes_out) {
        constexpr size_t CHUNK = 1024;
        std::vector<int8_t> tmp;
        for (size_t r0 = 0; r0 < count; r0 += CHUNK) {
            const size_t k = std::min(CHUNK, count - r0);
            tmp.resize(k * v->dpad);
            BN_HIP_TRY(bn::gated::Memcpy(tmp.data(), v->d_codes + (first + r0) * v->dpad, k * v->dpad, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < k; i++) memcpy(codes_out + (r0 + i) * v->dim, tmp.data() + i * v->dpad, v->dim);
        }
    }
    return BN_OK;
}

bn_status bn_sq8_search(bn_sq8 *v, const float *queries, size_t n_queries, size_t refine, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                        uint32_t *count_out, uint64_t *cand_out, uint32_t *cand_count_out) {
    if (n_queries && !queries) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return search(v, bn::QuerySource::host(queries), n_queries, refine, top_m, m_stride, id_out, score_out, count_out, cand_out, cand_count_out);
}

bn_status bn_sq8_search_ids(bn_sq8 *v, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t refine, size_t top_m, size_t m_stride,
                            uint64_t *id_out, float *score_out, uint32_t *count_out, uint64_t *cand_out, uint32_t *cand_count_out) {
    if (n_queries && !query_ids) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return search(v, bn::QuerySource::stored(query_ids, exclude_radius), n_queries, refine, top_m, m_stride, id_out, score_out, count_out, cand_out,
                  cand_count_out);
}

}  // extern "C"
