// bn_index_search_above / bn_index_search_above_ids behind the C ABI (include/birdnet_hip.h): every row of an id range that scores at
// least min_score against a query, in id ascending order, with the total count.  Scores have bn_index_search's bits.
//
// Kernels of this file:
//   * above_scan_kernel<QB> -- index_scan_kernel's tile loop written out once more (index_scan.h says why every scan keeps its own):
//     64 queries per pass in LDS, the exact-f32 MFMA v_mfma_f32_16x16x4_f32 with row = A operand and query = B operand, one accumulator
//     per (query, row) over k ascending.  Each workgroup owns a contiguous run of the 64-row tiles that cover the id range.  What differs
//     is the tail of a tile, which selects nothing: wave w takes queries w, w + 4, ...; lane = row; ONE ballot of the hit predicate gives
//     every hit its slot cnt[q] + (hits in lower lanes) in the workgroup's own staging list of that query, in id order because tiles,
//     and lanes within one, are visited in id order.  A slot is stored only while it is below cap_wg = min(rows of a workgroup,
//     max_hits); the count runs on uncapped.  A workgroup can therefore never drop an entry of the final first-max_hits: its count
//     exceeds cap_wg only when cap_wg == max_hits, and then it alone supplies max_hits entries and no later workgroup's are kept.
//     Out: stage[g][q][cap_wg], cnt[g][q].  No pending lists, no merge, no candidate buffer: 50 944 B of LDS (index_scan.h,
//     AboveLayout), below the size from which a kernel must opt in.
//   * above_offsets_kernel -- one thread per query: the exclusive prefix of the workgroups' uncapped counts in workgroup order is each
//     workgroup's offset into the query's list, their sum is count_out; the exclusive prefix over the queries of min(count, max_hits)
//     is where the query's list starts in the packed results.
//   * above_gather_kernel -- block (g, q) copies staged entry j to position offset + j of query q's packed list while that is below
//     max_hits, and looks the tag up in the plane (0 without one).
// No atomics anywhere: every slot is a function of counts taken in a fixed order.  A count (max_hits == 0) runs the first two kernels
// with a null staging pointer.
//
// Host side: index.hip's for_each_round stages the queries of either source in rounds of out_lists; a round is one
// run_threshold_passes (shared with group.hip): the round's thresholds go up, then passes of Plan::width queries (above_plan.h: the
// width shrinks until staging plus results fit a fixed budget), and what comes back per pass is the counts, then exactly the packed
// entries.  The buffers belong to the index (AboveState), allocated on first need and only ever grown.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <string>

#include "above_plan.h"
#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "index_scan.h"
#include "topm_select.h"

namespace bn {
struct AboveState {
    DeviceBuf<float> d_thr;      // [out_lists]: min_score of the round's queries
    DeviceBuf<uint32_t> d_cnt;   // [max_wg][QP]: uncapped hits per workgroup and query
    DeviceBuf<uint32_t> d_off;   // [max_wg][QP]: their exclusive prefix over the workgroups
    DeviceBuf<uint32_t> d_head;  // [2][QP]: count per query; start of the query's list in d_res
    PinnedBuf<uint32_t> h_head;
    DeviceBuf<topm::Cand> d_stage;  // [n_wg][width][cap_wg], stage_cap entries
    DeviceBuf<topm::Cand> d_res;    // [width x max_hits] packed, res_cap entries
    DeviceBuf<uint32_t> d_tag;      // likewise
    PinnedBuf<topm::Cand> h_res;    // the entries a pass returned, host_cap entries
    PinnedBuf<uint32_t> h_tag;      // host_tag_cap entries
    size_t stage_cap = 0, res_cap = 0, host_cap = 0, host_tag_cap = 0;
};
}  // namespace bn

namespace {

using bn::scan::KC;
using bn::scan::QS_LD;
using bn::scan::S_LD;
using bn::scan::TILE;
constexpr int QP = bn::scan::LP;  // queries per scan pass at most
static_assert(bn::above::TILE == TILE && bn::above::LISTS == QP, "above_plan.h restates index_scan.h");
static_assert(bn::above::ENTRY == sizeof(bn::topm::Cand) && bn::above::RESULT == sizeof(bn::topm::Cand) + sizeof(uint32_t), "above_plan.h's entry sizes");

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;

constexpr size_t ABOVE_LDS = bn::scan::AboveLayout::BYTES;

// Scan of one pass (nq <= QP queries, QB = ceil(nq / 16) query blocks) over rows [id_lo, id_hi).  Workgroup g owns tiles
// [tile_lo + g * tiles_per_wg, ...) below tile_hi.  Operands as in index_scan_kernel: lane l of wave w: A = row (tile row 16w + (l & 15)),
// k = 16s + 4(l >> 4) + c of each KC chunk; B = query 16qb + (l & 15) at the same k.  D: query 16qb + (l & 15), row 16w + 4(l >> 4) + reg.
// Out: stage[(g * lists + q) * cap_wg + slot] for slot < cap_wg (stage may be NULL with cap_wg == 0), cnt[g * QP + q].
template <int QB>
__global__ __launch_bounds__(256) void above_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t id_lo, uint32_t id_hi,
                                                         uint32_t dpad, const float *__restrict__ q, const uint8_t *__restrict__ qvalid, int nq,
                                                         const uint32_t *__restrict__ qid, int64_t radius, const float *__restrict__ min_score,
                                                         uint32_t tile_lo, uint32_t tile_hi, uint32_t tiles_per_wg, uint32_t cap_wg, int lists,
                                                         Cand *__restrict__ stage, uint32_t *__restrict__ cnt_out) {
    extern __shared__ __align__(16) char ab_lds[];
    using L = bn::scan::AboveLayout;
    float *Qs = reinterpret_cast<float *>(ab_lds + L::B);          // [QP][QS_LD]: the queries' current k chunk
    float *S = reinterpret_cast<float *>(ab_lds + L::S);           // [QP][S_LD]: scores of the current tile
    float *thr = reinterpret_cast<float *>(ab_lds + L::THR);       // [QP]
    uint32_t *cnt = reinterpret_cast<uint32_t *>(ab_lds + L::CNT);  // [QP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < QP; i += 256) {
        cnt[i] = 0;
        thr[i] = i < nq ? min_score[i] : __builtin_inff();
    }
    const uint32_t t0 = (uint32_t)min((uint64_t)tile_hi, (uint64_t)tile_lo + (uint64_t)blockIdx.x * tiles_per_wg);
    const uint32_t t1 = (uint32_t)min((uint64_t)tile_hi, (uint64_t)t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;
    Cand *my_stage = stage + (size_t)blockIdx.x * lists * cap_wg;

    // step u = (tile t0 + u / nkc, chunk u % nkc); the row chunk and the query chunk of step u + 1 are loaded during step u
    auto row_ptr = [&](uint32_t u) {
        const size_t row = (size_t)(t0 + u / nkc) * TILE + w * 16 + r16;  // < the slab's rows (padded to TILE)
        return slab + row * dpad + (u % nkc) * KC + 4 * h;
    };
    constexpr int QV = QB * 16 * (KC / 4) / 256;  // float4 of the query chunk per thread
    auto load_q = [&](uint32_t u, float4 *qr) {
        const uint32_t c = u % nkc;
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            qr[j] = qq < nq ? *reinterpret_cast<const float4 *>(q + (size_t)qq * dpad + c * KC + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float4 a[8], qr[QV];
    if (steps) {
        const float *rp = row_ptr(0);
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
        load_q(0, qr);
    }
    floatx4 acc[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (uint32_t u = 0; u < steps; u++) {
        __syncthreads();  // the previous chunk's Qs reads are done
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            *reinterpret_cast<float4 *>(Qs + qq * QS_LD + kk) = qr[j];
        }
        __syncthreads();
        float4 an[8];
        if (u + 1 < steps) {
            const float *rp = row_ptr(u + 1);
#pragma unroll
            for (int s = 0; s < 8; s++) an[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
            load_q(u + 1, qr);
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
#pragma unroll
            for (int b = 0; b < QB; b++) {
                const float4 bq = *reinterpret_cast<const float4 *>(Qs + (b * 16 + r16) * QS_LD + 16 * s + 4 * h);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, bq.x, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, bq.y, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, bq.z, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, bq.w, acc[b], 0, 0, 0);
            }
        }
        if (u + 1 < steps) {
#pragma unroll
            for (int s = 0; s < 8; s++) a[s] = an[s];
        }
        if ((u + 1) % nkc) continue;

        // ---- end of a tile: scores to LDS, then the hits of each query take their slots (wave w owns queries w, w + 4, ...)
        const uint32_t t = t0 + u / nkc;
#pragma unroll
        for (int b = 0; b < QB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = acc[b][r];
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const uint32_t grow = t * TILE + lane;
        const bool row_ok = grow >= id_lo && grow < id_hi && valid[grow];
        for (int qq = w; qq < nq; qq += 4) {
            if (!qvalid[qq]) continue;
            bool ok = row_ok;
            if (radius >= 0) {
                const int64_t d = (int64_t)grow - (int64_t)qid[qq];
                ok = ok && (d > radius || d < -radius);
            }
            const float s = S[qq * S_LD + lane];
            const bool hit = ok && s >= thr[qq];
            const uint64_t m = __ballot(hit);
            if (!m) continue;
            const uint32_t c = cnt[qq];
            const uint32_t slot = c + (uint32_t)lanes_below(m);
            if (hit && slot < cap_wg) my_stage[(size_t)qq * cap_wg + slot] = Cand{s, grow};
            if (lane == 0) cnt[qq] = c + (uint32_t)__popcll(m);  // read again only by this wave, after the next tile's barriers
        }
    }
    __syncthreads();
    for (int i = tid; i < nq; i += 256) cnt_out[blockIdx.x * QP + i] = cnt[i];
}

// One block of QP threads, thread = query.  off[g][q] = hits of query q in workgroups before g; head[q] = their total;
// head[QP + q] = sum over the queries before q of min(total, max_hits): where q's list starts in the packed results
__global__ __launch_bounds__(64) void above_offsets_kernel(const uint32_t *__restrict__ cnt, int n_wg, int nq, uint32_t max_hits,
                                                           uint32_t *__restrict__ off, uint32_t *__restrict__ head) {
    __shared__ uint32_t kept[QP];
    const int qq = threadIdx.x;
    uint32_t run = 0;  // below 2^32: the hits of a query are distinct rows, and an index holds fewer than 2^32 - 64
    if (qq < nq)
        for (int g = 0; g < n_wg; g++) {
            off[g * QP + qq] = run;
            run += cnt[g * QP + qq];
        }
    kept[qq] = min(run, max_hits);
    __syncthreads();
    uint32_t base = 0;
    for (int i = 0; i < qq; i++) base += kept[i];
    head[qq] = run;
    head[QP + qq] = base;
}

// block (g, q): workgroup g's staged entries of query q -> positions [off, off + n) of the query's packed list, while below max_hits
__global__ __launch_bounds__(256) void above_gather_kernel(const Cand *__restrict__ stage, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                           const uint32_t *__restrict__ head, uint32_t cap_wg, int lists, uint32_t max_hits,
                                                           const uint16_t *__restrict__ tags, Cand *__restrict__ res, uint32_t *__restrict__ tag) {
    const uint32_t g = blockIdx.x, qq = blockIdx.y;
    const uint32_t o = off[g * QP + qq];
    if (o >= max_hits) return;
    const uint32_t n = min(min(cnt[g * QP + qq], cap_wg), max_hits - o);
    const Cand *src = stage + ((size_t)g * lists + qq) * cap_wg;
    const size_t dst = (size_t)head[QP + qq] + o;  // + j < (queries before qq + 1) * max_hits
    for (uint32_t j = threadIdx.x; j < n; j += 256) {
        const Cand e = src[j];
        res[dst + j] = e;
        tag[dst + j] = tags ? tags[e.id] : 0u;
    }
}

using bn::check_launch;
using bn::set_last_error;

// room for `entries` elements of `elem` bytes, at least doubled up to `limit` when it grows; what was there is dropped (nothing of
// an earlier pass is kept)
template <class Buf>
hipError_t grow(Buf &b, size_t *cap, size_t entries, size_t limit, size_t elem) {
    if (entries <= *cap) return hipSuccess;
    const size_t want = std::max(entries, std::min(limit, 2 * *cap));
    *cap = 0;
    hipError_t e = b.alloc(want * elem);
    if (e == hipSuccess) *cap = want;
    return e;
}

// the state of an index, with the small buffers every call needs; the stream must be idle when a buffer is replaced
bn_status state_of(bn_index *ix, const bn::IndexScan &x, bn::AboveState **out) {
    bn::AboveState **slot = bn::index_above_state(ix);
    if (!*slot) {
        auto s = std::make_unique<bn::AboveState>();
        BN_HIP_TRY(s->d_thr.alloc(x.out_lists * sizeof(float)));
        BN_HIP_TRY(s->d_cnt.alloc((size_t)x.max_wg * QP * sizeof(uint32_t)));
        BN_HIP_TRY(s->d_off.alloc((size_t)x.max_wg * QP * sizeof(uint32_t)));
        BN_HIP_TRY(s->d_head.alloc(2 * QP * sizeof(uint32_t)));
        BN_HIP_TRY(s->h_head.alloc(2 * QP * sizeof(uint32_t)));
        *slot = s.release();
    }
    *out = *slot;
    return BN_OK;
}

// One pass: the np <= pl.width queries `q` of the staged round, which are queries p0 .. of the round and i0 .. of the call.  Scan,
// offsets, gather; the counts come back, then exactly the packed entries; both into the caller's arrays at query index i0.  Synchronous
bn_status run_pass(const bn::IndexScan &x, bn::AboveState &a, const bn::above::Plan &pl, uint32_t lo, uint32_t hi, const bn::StagedQueries &q, size_t p0, int np,
                   size_t i0, size_t max_hits, size_t h_stride, uint64_t *id_out, float *score_out, uint32_t *tag_out, uint32_t *count_out) {
    Cand *stage = max_hits ? a.d_stage.get() : nullptr;
    bn::by_blocks(np, [&](auto qb) {
        hipLaunchKernelGGL(above_scan_kernel<decltype(qb)::value>, dim3(pl.n_wg), dim3(256), ABOVE_LDS, x.stream, x.slab, x.valid, lo, hi, (uint32_t)x.dpad,
                           q.d_q, q.d_qvalid, np, q.d_qid, q.radius, a.d_thr + p0, pl.tile_lo, pl.tile_hi, pl.tiles_per_wg, pl.cap_wg, pl.width, stage,
                           a.d_cnt.get());
    });
    if (bn_status st = check_launch("above scan"); st != BN_OK) return st;
    hipLaunchKernelGGL(above_offsets_kernel, dim3(1), dim3(QP), 0, x.stream, a.d_cnt, (int)pl.n_wg, np, (uint32_t)max_hits, a.d_off.get(), a.d_head.get());
    if (bn_status st = check_launch("above offsets"); st != BN_OK) return st;
    if (max_hits) {
        hipLaunchKernelGGL(above_gather_kernel, dim3(pl.n_wg, (unsigned)np), dim3(256), 0, x.stream, a.d_stage, a.d_cnt, a.d_off, a.d_head, pl.cap_wg, pl.width,
                           (uint32_t)max_hits, x.tags, a.d_res.get(), a.d_tag.get());
        if (bn_status st = check_launch("above gather"); st != BN_OK) return st;
    }
    BN_HIP_TRY(hipMemcpyAsync(a.h_head, a.d_head, 2 * QP * sizeof(uint32_t), hipMemcpyDeviceToHost, x.stream));
    BN_HIP_TRY(hipStreamSynchronize(x.stream));
    const uint32_t *count = a.h_head, *base = a.h_head + QP;
    const size_t total = max_hits ? base[np - 1] + std::min<size_t>(count[np - 1], max_hits) : 0;
    if (total) {
        BN_HIP_TRY(grow(a.h_res, &a.host_cap, total, a.res_cap, sizeof(Cand)));
        BN_HIP_TRY(hipMemcpyAsync(a.h_res, a.d_res, total * sizeof(Cand), hipMemcpyDeviceToHost, x.stream));
        if (tag_out) {
            BN_HIP_TRY(grow(a.h_tag, &a.host_tag_cap, total, a.res_cap, sizeof(uint32_t)));
            BN_HIP_TRY(hipMemcpyAsync(a.h_tag, a.d_tag, total * sizeof(uint32_t), hipMemcpyDeviceToHost, x.stream));
        }
        BN_HIP_TRY(hipStreamSynchronize(x.stream));
    }
    for (int i = 0; i < np; i++) {
        count_out[i0 + i] = count[i];
        const size_t k = std::min<size_t>(count[i], max_hits), at = (i0 + i) * h_stride;
        for (size_t j = 0; j < k; j++) {
            id_out[at + j] = a.h_res[base[i] + j].id;
            score_out[at + j] = a.h_res[base[i] + j].s;
            if (tag_out) tag_out[at + j] = a.h_tag[base[i] + j];
        }
    }
    return BN_OK;
}

bn_status search(bn_index *ix, const bn::QuerySource &src, size_t n_queries, const float *min_score, uint64_t first_id, uint64_t n_ids, size_t max_hits,
                 size_t h_stride, uint64_t *id_out, float *score_out, uint32_t *tag_out, uint32_t *count_out) {
    bn_status st = bn::above::check_args(src.data(), n_queries, min_score, max_hits, h_stride, id_out, score_out, count_out);
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!ix) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    const size_t size = bn_index_size(ix);
    uint32_t lo = 0, hi = 0;
    if ((st = bn::above::check_range(first_id, n_ids, size, &lo, &hi)) != BN_OK) return st;
    if ((st = bn::check_query_ids(src, n_queries, size)) != BN_OK) return st;
    if (lo == hi || n_queries == 0) {  // an empty index, an empty range, no query: no launch
        std::fill(count_out, count_out + n_queries, 0u);
        return BN_OK;
    }
    bn::IndexScan x;
    if ((st = bn::index_scan_state(ix, &x)) != BN_OK) return st;
    bn::AboveState *a = nullptr;
    if ((st = state_of(ix, x, &a)) != BN_OK) return st;
    const bn::above::Plan pl = bn::above::plan(lo, hi, (size_t)x.max_wg, max_hits);
    if (max_hits && (pl.stage_entries > a->stage_cap || pl.result_entries > a->res_cap)) {
        BN_HIP_TRY(hipStreamSynchronize(x.stream));  // nothing reads a buffer that is replaced
        BN_HIP_TRY(grow(a->d_stage, &a->stage_cap, pl.stage_entries, pl.stage_entries, sizeof(Cand)));
        if (pl.result_entries > a->res_cap) {
            a->res_cap = 0;
            BN_HIP_TRY(a->d_res.alloc(pl.result_entries * sizeof(Cand)));
            BN_HIP_TRY(a->d_tag.alloc(pl.result_entries * sizeof(uint32_t)));
            a->res_cap = pl.result_entries;
        }
    }
    return bn::for_each_round(ix, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) {
        return bn::run_threshold_passes(x.stream, a->d_thr, min_score + q0, nq, (size_t)pl.width, [&](size_t p0, int np) {
            return run_pass(x, *a, pl, lo, hi, staged.at(p0), p0, np, q0 + p0, max_hits, h_stride, id_out, score_out, tag_out, count_out);
        });
    });
}

}  // namespace

void bn::above_state_free(AboveState *s) { delete s; }

extern "C" {

bn_status bn_index_search_above(bn_index *x, const float *queries, size_t n_queries, const float *min_score, uint64_t first_id, uint64_t n_ids,
                                size_t max_hits, size_t h_stride, uint64_t *id_out, float *score_out, uint32_t *tag_out, uint32_t *count_out) {
    return search(x, bn::QuerySource::host(queries), n_queries, min_score, first_id, n_ids, max_hits, h_stride, id_out, score_out, tag_out, count_out);
}

bn_status bn_index_search_above_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, const float *min_score,
                                    uint64_t first_id, uint64_t n_ids, size_t max_hits, size_t h_stride, uint64_t *id_out, float *score_out,
                                    uint32_t *tag_out, uint32_t *count_out) {
    return search(x, bn::QuerySource::stored(query_ids, exclude_radius), n_queries, min_score, first_id, n_ids, max_hits, h_stride, id_out, score_out,
                  tag_out, count_out);
}

}  // extern "C"
