// Embedding index behind the C ABI (include/birdnet_hip.h, bn_index_*): a device-resident slab of L2-normalised f32 rows and
// an exact top-M cosine search over it.
//
// Kernels:
//   * index_normalise_kernel -- one wave per row: sum of squares in a fixed order (lane-strided chains, then a fixed xor
//     butterfly), a validity flag, and the row x / sqrt(sum) stored with its stride padded with zeros to a multiple of KC, so
//     the scan has no k tail.  Appends (host rows or a context's embedding output) and host queries go through it.
//   * index_scan_kernel -- each workgroup streams its contiguous range of 64-row tiles ONCE for all queries of the pass (up to
//     64).  The products run on the exact-f32 MFMA v_mfma_f32_16x16x4_f32, which is bit for bit a k-ordered fmaf chain: the
//     k order of a (query, row) pair is fixed by the padded dim alone, never by the tile, the pass or the query count.  Each
//     tile's [64 queries x 64 rows] scores go to LDS, rows are masked there (invalid, excluded id, past the end), and a row
//     that beats the query's running M-th candidate joins a pending list; pending lists are merged into the workgroup's
//     running top-M (kept in its slice of the candidate buffer) when they fill.  Out: [workgroups x queries x M] candidates.
//   * index_merge_kernel -- one wave per query merges the workgroups' sorted lists into the final top-M, reading each list
//     only while its entries still beat the running M-th.
// Order everywhere: score descending, ties by id ascending (-0.0 == +0.0 through the float compare).  The candidate, the order and
// the two merges live in topm_select.h; the scan's constants and LDS layout in index_scan.h, which the subset, peaks and rank scans
// carve theirs from too.  Other files borrow this index's stream and buffers: rank.hip, subset.hip, peaks.hip, ivf.hip
// and sq8.hip through index_scan_state, cluster.hip through index_cluster_state, above.hip through both index_scan_state and
// index_above_state, group.hip likewise through index_group_state.  The host side those searches share is defined
// here once (declared in capi_internal.h): the LDS opt-in (LdsOptIn), the argument refusals (check_top_m, check_search_buffers),
// the round loop that stages a round's queries from either source (for_each_round over query_source.h's QuerySource), the pass loop
// with its merge and copy-back (run_scan_passes, index_enqueue_merge, copy_back_results), the threshold searches' round
// (run_threshold_passes) and the copy into the caller's arrays (scatter_results); subset.hip also reads the tag plane below.
//
// Row tags (bn_index_set_tags / fill_tags / read_tags): one u16 per row of capacity, allocated zeroed by the first call that sets one.
// No kernel of this file reads it.
//
// An index is reference counted: bn_index_free drops the caller's reference, and every attachment of match.hip (bn_ctx_attach_index)
// holds one, so the slab lives until the last of them.  match.hip reads the slab, the valid bytes and the tag plane on a context's
// stream, with buffers of its own; what it needs of an index is index_rows, index_tags and index_enqueue_normalise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "index_scan.h"
#include "topm_select.h"

namespace {

using bn::scan::KC;
using bn::scan::QS_LD;
using bn::scan::S_LD;
using bn::scan::TILE;
constexpr int QP = bn::scan::LP;  // queries per scan pass
constexpr size_t QCHUNK = 1024;  // queries normalised / searched per round of a call
constexpr size_t STAGE_ROWS = 1024;

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;  // the search's order: score descending, ties by id ascending

constexpr size_t SCAN_LDS = bn::scan::Layout<1>::BYTES;

// rows [n, dim] at src (row stride src_stride) -> normalised rows [n, dpad] at dst + validity flags
__global__ __launch_bounds__(256) void index_normalise_kernel(const float *__restrict__ src, size_t src_stride, uint32_t n, uint32_t dim,
                                                              float *__restrict__ dst, uint32_t dpad, uint8_t *__restrict__ valid) {
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= n) return;
    const float *x = src + (size_t)r * src_stride;
    float ss = 0.f;
    bool fin = true;
    for (uint32_t k = lane; k < dim; k += 64) {
        const float v = x[k];
        fin = fin && isfinite(v);
        ss = fmaf(v, v, ss);
    }
    for (int off = 32; off; off >>= 1) ss += __shfl_xor(ss, off);
    const bool ok = __ballot(!fin) == 0 && ss > 0.f && isfinite(ss);
    const float nrm = __fsqrt_rn(ss);
    float *y = dst + (size_t)r * dpad;
    for (uint32_t k = lane; k < dpad; k += 64) y[k] = (ok && k < dim) ? x[k] / nrm : 0.f;
    if (lane == 0) valid[r] = ok ? 1 : 0;
}

// stored rows ids[q] -> query rows (as stored) + their validity
__global__ __launch_bounds__(256) void index_gather_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid,
                                                           const uint32_t *__restrict__ ids, uint32_t dpad, float *__restrict__ dst,
                                                           uint8_t *__restrict__ dvalid) {
    const uint32_t q = blockIdx.x;
    const size_t row = ids[q];
    for (uint32_t k = threadIdx.x; k < dpad; k += 256) dst[(size_t)q * dpad + k] = slab[row * dpad + k];
    if (threadIdx.x == 0) dvalid[q] = valid[row];
}

// Scan of one pass (nq <= QP queries, QB = ceil(nq / 16) query blocks).  Workgroup g owns tiles [g * tiles_per_wg, ...).
// Lane l of wave w: A operand = row (tile row 16w + (l & 15)), k = 16s + 4(l >> 4) + t of each KC chunk (t = component of the
// float4); B operand = query 16qb + (l & 15) at the same k.  D: query 16qb + (l & 15), row 16w + 4(l >> 4) + reg.
template <int QB>
__global__ __launch_bounds__(256) void index_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t n_rows,
                                                         uint32_t dpad, const float *__restrict__ q, const uint8_t *__restrict__ qvalid, int nq,
                                                         const uint32_t *__restrict__ qid, int64_t radius, int M, uint32_t tiles_per_wg,
                                                         Cand *__restrict__ cand, int *__restrict__ cand_len) {
    extern __shared__ __align__(16) char idx_lds[];
    using L = bn::scan::Layout<1>;
    float *Qs = reinterpret_cast<float *>(idx_lds + L::B);             // [QP][QS_LD]: the queries' current k chunk
    float *S = reinterpret_cast<float *>(idx_lds + L::S);              // [QP][S_LD]: scores of the current tile
    Cand *pend = reinterpret_cast<Cand *>(idx_lds + L::PENDING);       // [QP][PEND]
    Cand *scratch = reinterpret_cast<Cand *>(idx_lds + L::SCRATCH);    // [4][MMAX]
    Cand *thr = reinterpret_cast<Cand *>(idx_lds + L::THR);            // [QP]
    int *len = reinterpret_cast<int *>(idx_lds + L::LEN);              // [QP]
    int *pn = reinterpret_cast<int *>(idx_lds + L::PN);                // [QP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < QP; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    const uint32_t n_tiles = (n_rows + TILE - 1) / TILE;
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = min(n_tiles, t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = t0 < t1 ? (t1 - t0) * nkc : 0;
    Cand *my_cand = cand + (size_t)blockIdx.x * QP * MMAX;

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

        // ---- end of a tile: scores to LDS, then selection (wave w owns queries w, w + 4, ...)
        const uint32_t t = t0 + u / nkc;
#pragma unroll
        for (int b = 0; b < QB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = acc[b][r];
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const uint32_t grow = t * TILE + lane;
        const bool row_ok = grow < n_rows && valid[grow];
        for (int qq = w; qq < nq; qq += 4) {
            if (!qvalid[qq]) continue;
            bool ok = row_ok;
            if (radius >= 0) {
                const int64_t d = (int64_t)grow - (int64_t)qid[qq];
                ok = ok && (d > radius || d < -radius);
            }
            const Cand e{S[qq * S_LD + lane], grow};
            int L = len[qq];
            const bool pass = ok && (L < M || Ord::ahead(e, thr[qq]));
            const uint64_t m = __ballot(pass);
            if (!m) continue;
            int np = pn[qq];
            if (np + 64 > PEND) {
                L = merge_pending<Ord>(pend + qq * PEND, np, my_cand + qq * MMAX, L, M, scratch + w * MMAX, thr + qq);
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
        int L = len[qq];
        const int np = pn[qq];
        if (np) L = merge_pending<Ord>(pend + qq * PEND, np, my_cand + qq * MMAX, L, M, scratch + w * MMAX, thr + qq);
        if (lane == 0) cand_len[blockIdx.x * QP + qq] = L;
    }
}

// one wave per query: the workgroups' sorted lists -> the final top-M (out [nq][M], count [nq])
__global__ __launch_bounds__(64) void index_merge_kernel(const Cand *__restrict__ cand, const int *__restrict__ cand_len, int n_wg, int M,
                                                         Cand *__restrict__ out, uint32_t *__restrict__ count) {
    bn::topm::merge_lists<Ord>(cand, cand_len, QP, n_wg, M, out, count);
}

bn::LdsOptIn g_scan_lds;

}  // namespace

struct bn_index {
    std::atomic<int> refs{1};  // the caller's handle + one per attachment that matches against it (match.hip)
    int device = 0;
    size_t dim = 0, dpad = 0, cap = 0, cap_pad = 0, size = 0;
    int max_wg = 0;
    bn::Stream stream;  // stream and event before the buffers: they go last (device_mem.h)
    bn::Event ev;       // recorded after the last bn_index_add_ctx on the context's stream
    bool pending = false;
    bn::DeviceBuf<float> slab;      // [cap_pad, dpad]
    bn::DeviceBuf<uint8_t> valid;   // [cap_pad]
    bn::DeviceBuf<float> d_stage;   // [STAGE_ROWS, dim]: host rows / queries on their way in
    bn::DeviceBuf<float> d_q;       // [QCHUNK, dpad]
    bn::DeviceBuf<uint8_t> d_qvalid;
    bn::DeviceBuf<uint32_t> d_qid;  // [QCHUNK]
    bn::DeviceBuf<Cand> d_cand;     // [max_wg, QP, MMAX]
    bn::DeviceBuf<int> d_cand_len;  // [max_wg, QP]
    bn::DeviceBuf<Cand> d_out;      // [QCHUNK, MMAX]
    bn::DeviceBuf<uint32_t> d_count;
    bn::PinnedBuf<Cand> h_out;  // pinned mirrors of d_out / d_count
    bn::PinnedBuf<uint32_t> h_count;
    bn::ClusterState *cluster = nullptr;  // cluster.hip's buffers, allocated by the first bn_index_assign / bn_index_cluster
    bn::DeviceBuf<uint16_t> tags;  // [cap_pad], allocated by the first bn_index_set_tags / bn_index_fill_tags; absent: every tag is 0
    bn::AboveState *above = nullptr;  // above.hip's buffers, allocated by the first bn_index_search_above / _ids
    bn::GroupState *group = nullptr;  // group.hip's buffers, allocated by the first bn_index_group_above / _ids
    ~bn_index() {
        (void)bn::use_device(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (ev) (void)hipEventSynchronize(ev);
        bn::cluster_state_free(cluster);
        bn::above_state_free(above);
        bn::group_state_free(group);
    }
};

namespace {

using bn::set_last_error;

using bn::check_launch;

void unref(bn_index *x) {
    if (x && x->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete x;
}

// device and stream of the index current, and the index's stream ordered after the last bn_index_add_ctx
bn_status begin(const bn_index *x) {
    BN_HIP_TRY(bn::use_device(x->device));
    if (x->pending) BN_HIP_TRY(hipStreamWaitEvent(x->stream, x->ev, 0));
    return BN_OK;
}

bn_status check_search_args(const bn_index *x, const void *queries, size_t n_queries, size_t top_m, size_t m_stride, const uint64_t *id_out,
                            const float *score_out, const uint32_t *count_out) {
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (bn_status st = bn::check_top_m(top_m, m_stride); st != BN_OK) return st;
    return bn::check_search_buffers(queries, n_queries, id_out, score_out, count_out);
}

// what a scan on the index's own stream and buffers needs (capi_internal.h)
bn::IndexScan scan_state_of(const bn_index *x) {
    bn::IndexScan s;
    s.device = x->device;
    s.stream = x->stream;
    s.slab = x->slab;
    s.valid = x->valid;
    s.dim = x->dim;
    s.dpad = x->dpad;
    s.size = x->size;
    s.cap_pad = x->cap_pad;
    s.max_wg = x->max_wg;
    s.lists = QP;
    s.out_lists = QCHUNK;
    s.d_cand = x->d_cand;
    s.d_cand_len = x->d_cand_len;
    s.d_out = x->d_out;
    s.d_count = x->d_count;
    s.h_out = x->h_out;
    s.h_count = x->h_count;
    s.tags = x->tags;
    return s;
}

// The round's nq queries of `unit` rows from query `first` on (nq * unit <= QCHUNK, every id in the index) -> d_q / d_qvalid, and
// d_qid for stored rows.  Host rows are normalised as appended rows are; a stored id stands for the `unit` rows from it on, gathered
// as they are.  Every copy waits for the stream first: the round before has read the buffer it overwrites
bn_status stage(bn_index *x, const bn::QuerySource &src, size_t first, size_t nq, size_t unit, bn::StagedQueries *out) {
    const size_t rows = nq * unit;
    if (src.ids) {
        std::vector<uint32_t> ids(rows);
        for (size_t i = 0; i < nq; i++)
            for (size_t j = 0; j < unit; j++) ids[i * unit + j] = (uint32_t)(src.ids[first + i] + j);
        BN_HIP_TRY(hipStreamSynchronize(x->stream));
        BN_HIP_TRY(bn::gated::Memcpy(x->d_qid, ids.data(), rows * sizeof(uint32_t), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(index_gather_kernel, dim3((unsigned)rows), dim3(256), 0, x->stream, x->slab, x->valid, x->d_qid, (uint32_t)x->dpad, x->d_q,
                           x->d_qvalid);
        if (bn_status st = check_launch("index gather"); st != BN_OK) return st;
    } else {
        for (size_t s0 = 0; s0 < rows; s0 += STAGE_ROWS) {
            const size_t k = std::min(STAGE_ROWS, rows - s0);
            BN_HIP_TRY(hipStreamSynchronize(x->stream));
            BN_HIP_TRY(bn::gated::Memcpy(x->d_stage, src.rows + (first * unit + s0) * x->dim, k * x->dim * sizeof(float), hipMemcpyHostToDevice));
            hipLaunchKernelGGL(index_normalise_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, x->stream, x->d_stage, x->dim, (uint32_t)k,
                               (uint32_t)x->dim, x->d_q + s0 * x->dpad, (uint32_t)x->dpad, x->d_qvalid + s0);
            if (bn_status st = check_launch("index normalise"); st != BN_OK) return st;
        }
    }
    *out = {x->d_q, x->d_qvalid, src.ids ? x->d_qid.get() : nullptr, src.radius, x->dpad};
    return BN_OK;
}

// bn_index_search and bn_index_search_ids behind their refusals (the index not empty): per round the scan + merge passes over the
// staged queries, results through the pinned mirrors into the caller's arrays
bn_status search_rounds(bn_index *x, const bn::QuerySource &src, size_t n_queries, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                        uint32_t *count_out) {
    const uint32_t n_rows = (uint32_t)x->size;
    const int M = (int)top_m;
    const bn::WgSplit sp = bn::split_tiles((n_rows + TILE - 1) / TILE, x->max_wg);
    return bn::for_each_round(x, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) -> bn_status {
        const bn::IndexScan s = scan_state_of(x);
        bn_status st = bn::run_scan_passes(s, nq, sp.n_wg, M, "index scan", [&](size_t p0, int np) {
            const bn::StagedQueries q = staged.at(p0);
            bn::by_blocks(np, [&](auto qb) {
                hipLaunchKernelGGL(index_scan_kernel<decltype(qb)::value>, dim3(sp.n_wg), dim3(256), SCAN_LDS, x->stream, x->slab, x->valid, n_rows,
                                   (uint32_t)x->dpad, q.d_q, q.d_qvalid, np, q.d_qid, q.radius, M, sp.tiles_per_wg, x->d_cand, x->d_cand_len);
            });
        });
        if (st == BN_OK) bn::scatter_results(s, q0, nq, top_m, m_stride, id_out, score_out, count_out);
        return st;
    });
}

// the refusals of the tag calls that write; then the plane, zeroed, if this is the first of them
bn_status prepare_tags(bn_index *x, uint64_t first_id, size_t n, const uint32_t *tags, size_t n_tags) {
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (n && n_tags && !tags) return set_last_error(BN_ERR_INVALID_ARG, "null tags");
    if (first_id > x->size || n > x->size - first_id)
        return set_last_error(BN_ERR_INVALID_ARG, "rows [" + std::to_string(first_id) + ", +" + std::to_string(n) + ") are not in the index (" +
                                                      std::to_string(x->size) + " rows)");
    for (size_t i = 0; i < n_tags; i++)
        if (tags[i] >= BN_INDEX_TAG_LIMIT)
            return set_last_error(BN_ERR_INVALID_ARG, "tag " + std::to_string(tags[i]) + " is not below " + std::to_string(BN_INDEX_TAG_LIMIT));
    if (!n) return BN_OK;
    bn_status st = begin(x);
    if (st != BN_OK) return st;
    BN_HIP_TRY(hipStreamSynchronize(x->stream));
    if (!x->tags) {
        bn::DeviceBuf<uint16_t> p;
        BN_HIP_TRY(p.alloc(x->cap_pad * sizeof(uint16_t)));
        if (hipError_t e = bn::gated::Memset(p, 0, x->cap_pad * sizeof(uint16_t)); e != hipSuccess)
            return set_last_error(BN_ERR_BACKEND, std::string("hipMemset of the tag plane failed: ") + hipGetErrorString(e));
        x->tags = std::move(p);
    }
    return BN_OK;
}

bn_status reserve_rows(const bn_index *x, size_t n) {
    if (n > x->cap - x->size)
        return set_last_error(BN_ERR_INVALID_ARG, "append of " + std::to_string(n) + " rows exceeds the index capacity (" + std::to_string(x->size) + " of " +
                                                      std::to_string(x->cap) + " rows used)");
    return BN_OK;
}

}  // namespace

bn_status bn::index_rows(bn_index *x, IndexRows *out) {
    if (!x || !out) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    bn_status st = begin(x);
    if (st != BN_OK) return st;
    BN_HIP_TRY(hipStreamSynchronize(x->stream));
    out->device = x->device;
    out->slab = x->slab;
    out->valid = x->valid;
    out->dim = x->dim;
    out->dpad = x->dpad;
    out->size = x->size;
    return BN_OK;
}

bn_status bn::for_each_round(bn_index *x, const QuerySource &src, size_t n, size_t unit, const RoundFn &fn) {
    if (!x || (n && !src.data())) return set_last_error(BN_ERR_INVALID_ARG, "for_each_round: bad argument");
    return each_round(n, QCHUNK, unit, [&](size_t first, size_t count) -> bn_status {
        StagedQueries q;
        bn_status st = begin(x);
        if (st == BN_OK) st = stage(x, src, first, count, unit, &q);
        return st == BN_OK ? fn(first, count, q) : st;
    });
}

bn::ClusterState **bn::index_cluster_state(bn_index *x) { return &x->cluster; }
bn::AboveState **bn::index_above_state(bn_index *x) { return &x->above; }
bn::GroupState **bn::index_group_state(bn_index *x) { return &x->group; }

void bn::index_ref(bn_index *x) { x->refs.fetch_add(1, std::memory_order_relaxed); }
void bn::index_unref(bn_index *x) { unref(x); }
int bn::index_device(const bn_index *x) { return x->device; }
hipStream_t bn::index_stream(const bn_index *x) { return x->stream; }
const uint16_t *bn::index_tags(const bn_index *x) { return x->tags; }

bn_status bn::index_enqueue_normalise(hipStream_t stream, const float *d_src, size_t src_stride, size_t n, size_t dim, float *d_dst, size_t dpad,
                                      uint8_t *d_valid) {
    hipLaunchKernelGGL(index_normalise_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, stream, d_src, src_stride, (uint32_t)n, (uint32_t)dim, d_dst,
                       (uint32_t)dpad, d_valid);
    return check_launch("index normalise");
}

bn_status bn::index_scan_state(bn_index *x, IndexScan *out) {
    if (!x || !out) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    bn_status st = begin(x);
    if (st != BN_OK) return st;
    *out = scan_state_of(x);
    return BN_OK;
}

bn_status bn::index_enqueue_merge(hipStream_t stream, const topm::Cand *cand, const int *cand_len, size_t n_queries, int n_wg, int M, topm::Cand *out,
                                  uint32_t *count) {
    hipLaunchKernelGGL(index_merge_kernel, dim3((unsigned)n_queries), dim3(64), 0, stream, cand, cand_len, n_wg, M, out, count);
    return check_launch("index merge");
}

hipError_t bn::LdsOptIn::prepare(int dev, std::initializer_list<Kernel> kernels) {
    std::lock_guard<std::mutex> lk(mu);
    if (dev < 64 && ((ready >> dev) & 1)) return hipSuccess;
    bn::gated::Shared g;
    for (const Kernel &k : kernels) {
        hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes);
        if (e != hipSuccess) return e;
    }
    if (dev < 64) ready |= 1ull << dev;
    return hipSuccess;
}

bn_status bn::check_top_m(size_t top_m, size_t m_stride) {
    if (top_m < 1 || top_m > (size_t)MMAX) return set_last_error(BN_ERR_INVALID_ARG, "top_m must be in 1..256, got " + std::to_string(top_m));
    if (m_stride < top_m) return set_last_error(BN_ERR_INVALID_ARG, "m_stride < top_m");
    return BN_OK;
}

bn_status bn::check_search_buffers(const void *queries, size_t n_queries, const uint64_t *id_out, const float *score_out, const uint32_t *count_out) {
    if (n_queries && (!queries || !id_out || !score_out || !count_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return BN_OK;
}

bn_status bn::run_scan_passes(const IndexScan &s, size_t n_lists, uint32_t n_wg, int M, const char *what,
                              const std::function<void(size_t p0, int np)> &launch_scan, MergeEnqueue merge) {
    for (size_t p0 = 0; p0 < n_lists; p0 += s.lists) {
        const int np = (int)std::min(s.lists, n_lists - p0);
        launch_scan(p0, np);
        bn_status st = check_launch(what);
        if (st != BN_OK) return st;
        if ((st = merge(s.stream, s.d_cand, s.d_cand_len, (size_t)np, (int)n_wg, M, s.d_out + p0 * M, s.d_count + p0)) != BN_OK) return st;
    }
    return copy_back_results(s, n_lists, M);
}

bn_status bn::copy_back_results(const IndexScan &s, size_t n, int M) {
    BN_HIP_TRY(hipMemcpyAsync(s.h_out, s.d_out, n * M * sizeof(Cand), hipMemcpyDeviceToHost, s.stream));
    BN_HIP_TRY(hipMemcpyAsync(s.h_count, s.d_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream));
    BN_HIP_TRY(hipStreamSynchronize(s.stream));
    return BN_OK;
}

void bn::scatter_results(const IndexScan &s, size_t first, size_t n, size_t M, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out) {
    for (size_t i = 0; i < n; i++) {
        const uint32_t c = s.h_count[i];
        const size_t at = (first + i) * m_stride;
        count_out[first + i] = c;
        for (uint32_t j = 0; j < c; j++) {
            id_out[at + j] = s.h_out[i * M + j].id;
            score_out[at + j] = s.h_out[i * M + j].s;
        }
    }
}

bn_status bn::run_threshold_passes(hipStream_t stream, float *d_thr, const float *min_score, size_t nq, size_t width,
                                   const std::function<bn_status(size_t p0, int np)> &pass) {
    BN_HIP_TRY(hipStreamSynchronize(stream));  // the last pass of the round before has read d_thr
    BN_HIP_TRY(bn::gated::Memcpy(d_thr, min_score, nq * sizeof(float), hipMemcpyHostToDevice));
    for (size_t p0 = 0; p0 < nq; p0 += width)
        if (bn_status st = pass(p0, (int)std::min(width, nq - p0)); st != BN_OK) return st;
    return BN_OK;
}

bn_status bn::index_io_state(bn_index *x, IndexIo *out) {
    if (!x || !out) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    bn_status st = begin(x);
    if (st != BN_OK) return st;
    out->device = x->device;
    out->stream = x->stream;
    out->slab = x->slab;
    out->valid = x->valid;
    out->dim = x->dim;
    out->dpad = x->dpad;
    out->size = x->size;
    out->cap = x->cap;
    return BN_OK;
}

bn_status bn::index_adopt_rows(bn_index *x, size_t n) {
    if (!x || x->size != 0 || n > x->cap) return set_last_error(BN_ERR_INVALID_ARG, "index_adopt_rows: bad argument");
    x->size = n;
    return BN_OK;
}

bn_status bn::index_copy_shape(const bn_index *dst, size_t n, size_t *dpad, int *max_wg) {
    if (!dst || !dpad || !max_wg) return set_last_error(BN_ERR_INVALID_ARG, "index_copy_shape: bad argument");
    if (bn_status st = reserve_rows(dst, n); st != BN_OK) return st;
    *dpad = dst->dpad;
    *max_wg = dst->max_wg;
    return BN_OK;
}

bn_status bn::index_copy_begin(bn_index *dst, const bn_index *src, size_t n, IndexCopy *out) {
    if (!dst || !src || !out || dst == src || dst->dim != src->dim || dst->device != src->device)
        return set_last_error(BN_ERR_INVALID_ARG, "index_copy_begin: bad argument");
    bn_status st = reserve_rows(dst, n);
    if (st != BN_OK) return st;
    if ((st = begin(dst)) != BN_OK) return st;
    // src's own stream is idle between calls; what may still be writing its rows is the context stream behind its event
    if (src->pending) BN_HIP_TRY(hipStreamWaitEvent(dst->stream, src->ev, 0));
    if (src->tags && !dst->tags) {
        bn::DeviceBuf<uint16_t> p;
        BN_HIP_TRY(p.alloc(dst->cap_pad * sizeof(uint16_t)));
        BN_HIP_TRY(hipMemsetAsync(p, 0, dst->cap_pad * sizeof(uint16_t), dst->stream));  // on the stream that writes the new tags: ordered before them
        dst->tags = std::move(p);
    }
    out->device = dst->device;
    out->stream = dst->stream;
    out->dpad = dst->dpad;
    out->first = dst->size;
    out->max_wg = dst->max_wg;
    out->src_slab = src->slab;
    out->src_valid = src->valid;
    out->src_tags = src->tags;
    out->dst_slab = dst->slab + dst->size * dst->dpad;
    out->dst_valid = dst->valid + dst->size;
    out->dst_tags = dst->tags ? dst->tags + dst->size : nullptr;
    return BN_OK;
}

void bn::index_copy_commit(bn_index *dst, size_t n) { dst->size += n; }

extern "C" {

bn_status bn_index_create(int32_t device, size_t dim, size_t capacity_rows, bn_index **out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (dim == 0) return set_last_error(BN_ERR_INVALID_ARG, "dim must be at least 1");
    if (dim > (1u << 20)) return set_last_error(BN_ERR_INVALID_ARG, "dim above 2^20");
    if (capacity_rows == 0) return set_last_error(BN_ERR_INVALID_ARG, "capacity_rows must be at least 1");
    if (capacity_rows >= 0xffffffffull - TILE) return set_last_error(BN_ERR_INVALID_ARG, "capacity_rows must be below 2^32 - 64");
    if (bn_status dst = bn::require_device(device); dst != BN_OK) return dst;
    BN_HIP_TRY(bn::use_device(device));
    BN_HIP_TRY(g_scan_lds.prepare(device, {{(const void *)index_scan_kernel<1>, SCAN_LDS}, {(const void *)index_scan_kernel<2>, SCAN_LDS},
                                            {(const void *)index_scan_kernel<3>, SCAN_LDS}, {(const void *)index_scan_kernel<4>, SCAN_LDS}}));
    auto x = std::make_unique<bn_index>();
    x->device = device;
    x->dim = dim;
    x->dpad = (dim + KC - 1) / KC * KC;
    x->cap = capacity_rows;
    x->cap_pad = (capacity_rows + TILE - 1) / TILE * TILE;
    int cus = 0;
    BN_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    x->max_wg = std::max(1, cus);
    BN_HIP_TRY(x->stream.create(hipStreamNonBlocking));
    BN_HIP_TRY(x->ev.create(hipEventDisableTiming));
    // zeroed on the index's own stream and waited for below: a hipMemset of device memory may return before it has run, and nothing
    // orders the null stream before a kernel that the first call after this one puts on a non-blocking stream
    BN_HIP_TRY(x->slab.alloc(x->cap_pad * x->dpad * sizeof(float)));
    BN_HIP_TRY(hipMemsetAsync(x->slab, 0, x->cap_pad * x->dpad * sizeof(float), x->stream));
    BN_HIP_TRY(x->valid.alloc(x->cap_pad));
    BN_HIP_TRY(hipMemsetAsync(x->valid, 0, x->cap_pad, x->stream));
    BN_HIP_TRY(x->d_stage.alloc(STAGE_ROWS * dim * sizeof(float)));
    BN_HIP_TRY(x->d_q.alloc(QCHUNK * x->dpad * sizeof(float)));
    BN_HIP_TRY(x->d_qvalid.alloc(QCHUNK));
    BN_HIP_TRY(x->d_qid.alloc(QCHUNK * sizeof(uint32_t)));
    BN_HIP_TRY(x->d_cand.alloc((size_t)x->max_wg * QP * MMAX * sizeof(Cand)));
    BN_HIP_TRY(x->d_cand_len.alloc((size_t)x->max_wg * QP * sizeof(int)));
    BN_HIP_TRY(x->d_out.alloc(QCHUNK * MMAX * sizeof(Cand)));
    BN_HIP_TRY(x->d_count.alloc(QCHUNK * sizeof(uint32_t)));
    BN_HIP_TRY(x->h_out.alloc(QCHUNK * MMAX * sizeof(Cand)));
    BN_HIP_TRY(x->h_count.alloc(QCHUNK * sizeof(uint32_t)));
    BN_HIP_TRY(hipStreamSynchronize(x->stream));
    *out = x.release();
    return BN_OK;
}

void bn_index_free(bn_index *x) { unref(x); }

size_t bn_index_size(const bn_index *x) { return x ? x->size : 0; }
size_t bn_index_dim(const bn_index *x) { return x ? x->dim : 0; }

bn_status bn_index_add_host(bn_index *x, const float *rows, size_t n, uint64_t *first_id) {
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (n && !rows) return set_last_error(BN_ERR_INVALID_ARG, "null rows");
    bn_status st = reserve_rows(x, n);
    if (st != BN_OK) return st;
    if ((st = begin(x)) != BN_OK) return st;
    const size_t first = x->size;
    for (size_t r0 = 0; r0 < n; r0 += STAGE_ROWS) {
        const size_t k = std::min(STAGE_ROWS, n - r0);
        BN_HIP_TRY(hipStreamSynchronize(x->stream));  // the previous chunk's kernel has read the staging buffer
        BN_HIP_TRY(bn::gated::Memcpy(x->d_stage, rows + r0 * x->dim, k * x->dim * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(index_normalise_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, x->stream, x->d_stage, x->dim, (uint32_t)k,
                           (uint32_t)x->dim, x->slab + (first + r0) * x->dpad, (uint32_t)x->dpad, x->valid + first + r0);
        if ((st = check_launch("index normalise")) != BN_OK) return st;
    }
    BN_HIP_TRY(hipStreamSynchronize(x->stream));
    x->size = first + n;
    if (first_id) *first_id = first;
    return BN_OK;
}

bn_status bn_index_add_ctx(bn_index *x, bn_ctx *c, size_t batch_size, uint64_t *first_id) {
    if (!x || !c) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    bn::CtxEmbedding e;
    bn_status st = bn::ctx_embedding(c, &e);
    if (st != BN_OK) return st;
    if (e.row_elems != x->dim)
        return set_last_error(BN_ERR_INVALID_ARG, "embedding dimension " + std::to_string(e.row_elems) + " differs from the index's " + std::to_string(x->dim));
    if (e.device != x->device) return set_last_error(BN_ERR_INVALID_ARG, "the context lives on device " + std::to_string(e.device) + ", the index on " + std::to_string(x->device));
    if (batch_size > e.last_batch)
        return set_last_error(BN_ERR_INVALID_ARG, "batch_size " + std::to_string(batch_size) + " exceeds the context's last run (" + std::to_string(e.last_batch) + " rows)");
    if ((st = reserve_rows(x, batch_size)) != BN_OK) return st;
    const size_t first = x->size;
    if (batch_size) {
        BN_HIP_TRY(bn::use_device(x->device));
        // the index's own stream is idle between calls; appends from several contexts stay in call order
        if (x->pending) BN_HIP_TRY(hipStreamWaitEvent(e.stream, x->ev, 0));
        hipLaunchKernelGGL(index_normalise_kernel, dim3((unsigned)((batch_size + 3) / 4)), dim3(256), 0, e.stream, e.d_rows, e.row_elems,
                           (uint32_t)batch_size, (uint32_t)x->dim, x->slab + first * x->dpad, (uint32_t)x->dpad, x->valid + first);
        if ((st = check_launch("index normalise")) != BN_OK) return st;
        BN_HIP_TRY(hipEventRecord(x->ev, e.stream));
        x->pending = true;
        x->size = first + batch_size;
    }
    if (first_id) *first_id = first;
    return BN_OK;
}

bn_status bn_index_read(const bn_index *x, uint64_t first, size_t count, float *host_out) {
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (first > x->size || count > x->size - first) return set_last_error(BN_ERR_INVALID_ARG, "rows out of range");
    if (count && !host_out) return set_last_error(BN_ERR_INVALID_ARG, "null host buffer");
    bn_status st = begin(x);
    if (st != BN_OK) return st;
    BN_HIP_TRY(hipStreamSynchronize(x->stream));
    std::vector<float> tmp;
    for (size_t r0 = 0; r0 < count; r0 += STAGE_ROWS) {
        const size_t k = std::min(STAGE_ROWS, count - r0);
        tmp.resize(k * x->dpad);
        BN_HIP_TRY(bn::gated::Memcpy(tmp.data(), x->slab + (first + r0) * x->dpad, k * x->dpad * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < k; i++) memcpy(host_out + (r0 + i) * x->dim, tmp.data() + i * x->dpad, x->dim * sizeof(float));
    }
    return BN_OK;
}

bn_status bn_index_set_tags(bn_index *x, uint64_t first_id, size_t n, const uint32_t *tags) {
    bn_status st = prepare_tags(x, first_id, n, tags, n);
    if (st != BN_OK || !n) return st;
    const std::vector<uint16_t> t(tags, tags + n);
    BN_HIP_TRY(bn::gated::Memcpy(x->tags + first_id, t.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    return BN_OK;
}

bn_status bn_index_fill_tags(bn_index *x, uint64_t first_id, size_t n, uint32_t tag) {
    bn_status st = prepare_tags(x, first_id, n, &tag, 1);
    if (st != BN_OK || !n) return st;
    const std::vector<uint16_t> t(n, (uint16_t)tag);
    BN_HIP_TRY(bn::gated::Memcpy(x->tags + first_id, t.data(), n * sizeof(uint16_t), hipMemcpyHostToDevice));
    return BN_OK;
}

bn_status bn_index_read_tags(const bn_index *x, uint64_t first, size_t count, uint32_t *tags_out) {
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (first > x->size || count > x->size - first) return set_last_error(BN_ERR_INVALID_ARG, "rows out of range");
    if (count && !tags_out) return set_last_error(BN_ERR_INVALID_ARG, "null host buffer");
    if (!count) return BN_OK;
    if (!x->tags) {
        std::fill(tags_out, tags_out + count, 0u);
        return BN_OK;
    }
    bn_status st = begin(x);
    if (st != BN_OK) return st;
    BN_HIP_TRY(hipStreamSynchronize(x->stream));
    std::vector<uint16_t> t(count);
    BN_HIP_TRY(bn::gated::Memcpy(t.data(), x->tags + first, count * sizeof(uint16_t), hipMemcpyDeviceToHost));
    std::copy(t.begin(), t.end(), tags_out);
    return BN_OK;
}

bn_status bn_index_search(bn_index *x, const float *queries, size_t n_queries, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                          uint32_t *count_out) {
    bn_status st = check_search_args(x, queries, n_queries, top_m, m_stride, id_out, score_out, count_out);
    if (st != BN_OK) return st;
    if (x->size == 0) {  // no launch
        std::fill(count_out, count_out + n_queries, 0u);
        return BN_OK;
    }
    return search_rounds(x, bn::QuerySource::host(queries), n_queries, top_m, m_stride, id_out, score_out, count_out);
}

bn_status bn_index_search_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t top_m, size_t m_stride,
                              uint64_t *id_out, float *score_out, uint32_t *count_out) {
    bn_status st = check_search_args(x, query_ids, n_queries, top_m, m_stride, id_out, score_out, count_out);
    if (st != BN_OK) return st;
    const bn::QuerySource src = bn::QuerySource::stored(query_ids, exclude_radius);
    if ((st = bn::check_query_ids(src, n_queries, x->size)) != BN_OK) return st;
    return search_rounds(x, src, n_queries, top_m, m_stride, id_out, score_out, count_out);
}

}  // extern "C"
