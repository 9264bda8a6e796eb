// Matching a step's embeddings against an attached index (include/birdnet_hip.h: bn_ctx_attach_index, bn_step_index_results,
// bn_index_match): the watch list.  A snapshot of an index -- rows [0, n), n the size at the attach -- is searched for every row of
// every step, on the context's stream behind the plan, with scratch that belongs to the attachment: the index's own stream and
// buffers are not touched, so any number of contexts match against one index while other threads append to it and search it.
//
// Kernels (three launches per step, whatever the batch; DESIGN.md 7b, "Matching a step against an attached index"):
//   * the query rows are normalised by index.hip's index_normalise_kernel (index_enqueue_normalise): the index's rule, the index's bits.
//   * match_scan_kernel -- index_scan_kernel's tile loop (the same k-ordered chain on v_mfma_f32_16x16x4_f32, so the same score
//     bits), one launch for the whole batch: grid (row ranges x passes of 64 queries).  Rows are masked by id against the snapshot
//     (the last tile may hold rows an append is writing: their valid bytes are not looked at), then by their valid byte; with a
//     threshold a candidate below min_score never enters a pending list.  Out: [ranges][passes][64][256] candidates + lengths.
//   * match_merge_kernel -- one wave per query walks its `ranges` sorted lists into the final top-M, gathers the tags of the rows
//     it kept and writes the packed result rows (id widened to u64, score, tag, count) that one copy takes to pinned memory.
// The number of row ranges comes from the snapshot's tile count (match_ranges), not from the index's max_wg: the merge walks one
// list per range and the whole step has 0.45 ms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>

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
constexpr int QP = bn::scan::LP;     // queries per pass
constexpr size_t ROUND = 256;        // rows per round of bn_index_match: four passes in one launch
constexpr uint32_t MAX_RANGES = 256;

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;

constexpr size_t SCAN_LDS = bn::scan::Layout<1>::BYTES;

// Pass blockIdx.y (queries [64 * pass, ..) of nq_all, QB blocks of 16 of them) over the tiles [blockIdx.x * tiles_per_wg, ..) of
// rows [0, n_rows).  Operand and result lanes as in index_scan_kernel.
template <int QB>
__global__ __launch_bounds__(256) void match_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t n_rows,
                                                         uint32_t dpad, const float *__restrict__ q_all, const uint8_t *__restrict__ qvalid_all,
                                                         int nq_all, int M, int has_min, float min_score, uint32_t tiles_per_wg,
                                                         Cand *__restrict__ cand, int *__restrict__ cand_len) {
    extern __shared__ __align__(16) char match_lds[];
    using L = bn::scan::Layout<1>;
    float *Qs = reinterpret_cast<float *>(match_lds + L::B);           // [QP][QS_LD]: the queries' current k chunk
    float *S = reinterpret_cast<float *>(match_lds + L::S);            // [QP][S_LD]: scores of the current tile
    Cand *pend = reinterpret_cast<Cand *>(match_lds + L::PENDING);     // [QP][PEND]
    Cand *scratch = reinterpret_cast<Cand *>(match_lds + L::SCRATCH);  // [4][MMAX]
    Cand *thr = reinterpret_cast<Cand *>(match_lds + L::THR);          // [QP]
    int *len = reinterpret_cast<int *>(match_lds + L::LEN);            // [QP]
    int *pn = reinterpret_cast<int *>(match_lds + L::PN);              // [QP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < QP; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    const int q0 = (int)blockIdx.y * QP;
    const int nq = min(QP, nq_all - q0);
    const float *q = q_all + (size_t)q0 * dpad;
    const uint8_t *qvalid = qvalid_all + q0;
    const uint32_t n_tiles = (n_rows + TILE - 1) / TILE;
    const uint32_t t0 = blockIdx.x * tiles_per_wg;
    const uint32_t t1 = min(n_tiles, t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = t0 < t1 ? (t1 - t0) * nkc : 0;
    const size_t unit = ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * QP;  // this workgroup's first list
    Cand *my_cand = cand + unit * MMAX;

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
        const bool row_ok = grow < n_rows && valid[grow];  // by id first: a row past the snapshot may be half written
        for (int qq = w; qq < nq; qq += 4) {
            if (!qvalid[qq]) continue;
            const Cand e{S[qq * S_LD + lane], grow};
            int L = len[qq];
            const bool pass = row_ok && (!has_min || e.s >= min_score) && (L < M || Ord::ahead(e, thr[qq]));
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
        if (lane == 0) cand_len[unit + qq] = L;
    }
}

// One wave per query q: its n_ranges sorted lists cand[g][q][MMAX] (lengths cand_len[g][q], `lists` = passes * 64 lists per range)
// -> the first M of their union as packed result rows at stride M: id (u64), score, tag (tags == NULL: 0), and count[q].  Each list
// is read only while its entries still beat the running M-th.
__global__ __launch_bounds__(64) void match_merge_kernel(const Cand *__restrict__ cand, const int *__restrict__ cand_len, int lists, int n_ranges,
                                                         int M, const uint16_t *__restrict__ tags, uint64_t *__restrict__ id_out,
                                                         float *__restrict__ score_out, uint32_t *__restrict__ tag_out,
                                                         uint32_t *__restrict__ count_out) {
    __shared__ Cand list[MMAX], scratch[MMAX], pend[PEND];
    __shared__ Cand thr;
    __shared__ int lens[MAX_RANGES];
    const int q = blockIdx.x, lane = threadIdx.x;
    for (int g = lane; g < n_ranges; g += 64) lens[g] = cand_len[(size_t)g * lists + q];
    wave_sync();
    int len = 0, np = 0;
    for (int g = 0; g < n_ranges; g++) {
        const Cand *src = cand + ((size_t)g * lists + q) * MMAX;
        const int lg = lens[g];
        for (int j = 0; j < lg; j += 64) {
            const bool in = j + lane < lg;
            const Cand e = in ? src[j + lane] : Cand{0.f, 0u};
            const bool pass = in && (len < M || Ord::ahead(e, thr));
            const uint64_t m = __ballot(pass);
            if (!m) break;  // the list is sorted: nothing after a rejected entry can pass
            if (np + 64 > PEND) {
                len = merge_pending<Ord>(pend, np, list, len, M, scratch, &thr);
                np = 0;
            }
            if (pass) pend[np + lanes_below(m)] = e;
            np += __popcll(m);
            wave_sync();
        }
    }
    if (np) len = merge_pending<Ord>(pend, np, list, len, M, scratch, &thr);
    for (int i = lane; i < len; i += 64) {
        const Cand e = list[i];
        const size_t o = (size_t)q * M + i;
        id_out[o] = e.id;
        score_out[o] = e.s;
        tag_out[o] = tags ? (uint32_t)tags[e.id] : 0u;
    }
    if (lane == 0) count_out[q] = (uint32_t)len;
}

bn::LdsOptIn g_match_lds;

using bn::check_launch;
using bn::set_last_error;

// The packed result rows of `batch` queries at stride m: [id: batch * m u64][score: batch * m][tag: batch * m][count: batch], one
// region on its way to pinned memory
struct Rows {
    uint64_t *id;
    float *score;
    uint32_t *tag, *count;
    static size_t bytes(size_t batch, size_t m) { return batch * m * 16 + batch * 4; }
    static Rows view(void *base, size_t batch, size_t m) {
        Rows r;
        r.id = static_cast<uint64_t *>(base);
        r.score = reinterpret_cast<float *>(r.id + batch * m);
        r.tag = reinterpret_cast<uint32_t *>(r.score + batch * m);
        r.count = r.tag + batch * m;
        return r;
    }
};

}  // namespace

// The row ranges of a snapshot of n_tiles tiles: the smallest R with R^2 >= 64 * n_tiles, at most MAX_RANGES and n_tiles.  The scan's
// time falls as n_tiles / R, the merge's grows as R (one list per range and query, walked by one wave); their sum is least where
// R^2 = n_tiles * (time of a tile) / (time of a list).  Measured beside three other stepping contexts a tile costs 45-150 us and a
// list 1-3 us: the ratio is about 64, so up to 64 tiles every tile has a workgroup of its own
bn::WgSplit bn::match_ranges(uint32_t n_tiles) {
    if (n_tiles == 0) return {1, 0};
    uint32_t r = 1;
    while (r < MAX_RANGES && r < n_tiles && (uint64_t)r * r < 64ull * n_tiles) r++;
    return bn::split_tiles(n_tiles, r);
}

struct bn::MatchAttach {
    bn_index *index = nullptr;  // holds a reference
    int device = 0;
    const float *slab = nullptr;
    const uint8_t *valid = nullptr;
    size_t dim = 0, dpad = 0, n = 0;  // the snapshot: rows [0, n)
    bn::WgSplit split{1, 0};
    size_t max_batch = 0, M = 0;
    int32_t has_min = 0;
    float min_score = 0.f;
    bn::DeviceBuf<float> d_q;          // [max_batch, dpad]
    bn::DeviceBuf<uint8_t> d_qvalid;   // [max_batch]
    bn::DeviceBuf<Cand> d_cand;        // [ranges][passes][64][256]
    bn::DeviceBuf<int> d_cand_len;     // [ranges][passes][64]
    bn::DeviceBuf<void> d_rows;        // Rows of max_batch
    bn::PinnedBuf<void> h_rows;        // and the pinned mirror
    size_t last_batch = 0;
    bool stepped = false;
    ~MatchAttach() { bn::index_unref(index); }
};

namespace {

bn_status check_threshold(int32_t has_min, float min_score) {
    if (has_min && !std::isfinite(min_score)) return set_last_error(BN_ERR_INVALID_ARG, "min_score must be finite");
    return BN_OK;
}

// the snapshot and the scratch of an attachment for up to max_batch rows per step; takes a reference on the index
bn_status make_attach(bn_index *x, const bn::IndexRows &v, size_t max_batch, size_t top_m, int32_t has_min, float min_score, bn::MatchAttach **out) {
    BN_HIP_TRY(bn::use_device(v.device));
    BN_HIP_TRY(g_match_lds.prepare(v.device, {{(const void *)match_scan_kernel<1>, SCAN_LDS}, {(const void *)match_scan_kernel<2>, SCAN_LDS},
                                              {(const void *)match_scan_kernel<3>, SCAN_LDS}, {(const void *)match_scan_kernel<4>, SCAN_LDS}}));
    auto a = std::make_unique<bn::MatchAttach>();
    a->device = v.device;
    a->slab = v.slab;
    a->valid = v.valid;
    a->dim = v.dim;
    a->dpad = v.dpad;
    a->n = v.size;
    a->split = bn::match_ranges((uint32_t)((v.size + TILE - 1) / TILE));
    a->max_batch = max_batch;
    a->M = top_m;
    a->has_min = has_min;
    a->min_score = min_score;
    const size_t passes = (max_batch + QP - 1) / QP, units = std::max<size_t>(1, (size_t)a->split.n_wg * passes);
    BN_HIP_TRY(a->d_q.alloc(std::max<size_t>(1, max_batch) * v.dpad * sizeof(float)));
    BN_HIP_TRY(a->d_qvalid.alloc(std::max<size_t>(1, max_batch)));
    BN_HIP_TRY(a->d_cand.alloc(units * QP * MMAX * sizeof(Cand)));
    BN_HIP_TRY(a->d_cand_len.alloc(units * QP * sizeof(int)));
    BN_HIP_TRY(a->d_rows.alloc(std::max<size_t>(16, Rows::bytes(max_batch, top_m))));
    BN_HIP_TRY(a->h_rows.alloc(std::max<size_t>(16, Rows::bytes(max_batch, top_m))));
    bn::index_ref(x);
    a->index = x;
    *out = a.release();
    return BN_OK;
}

// normalise + scan + merge-and-pack + the rows to pinned memory for `batch` raw rows at d_src (row stride src_stride), on `stream`
bn_status enqueue_match(bn::MatchAttach *a, hipStream_t stream, const float *d_src, size_t src_stride, size_t batch) {
    bn_status st = bn::index_enqueue_normalise(stream, d_src, src_stride, batch, a->dim, a->d_q, a->dpad, a->d_qvalid);
    if (st != BN_OK) return st;
    const int passes = (int)((batch + QP - 1) / QP), M = (int)a->M;
    const uint32_t n_wg = a->split.n_wg;
    if (n_wg) {
        bn::by_blocks(passes > 1 ? QP : (int)batch, [&](auto qb) {
            hipLaunchKernelGGL(match_scan_kernel<decltype(qb)::value>, dim3(n_wg, (unsigned)passes), dim3(256), SCAN_LDS, stream, a->slab, a->valid,
                               (uint32_t)a->n, (uint32_t)a->dpad, a->d_q, a->d_qvalid, (int)batch, M, (int)a->has_min, a->min_score,
                               a->split.tiles_per_wg, a->d_cand, a->d_cand_len);
        });
        if ((st = check_launch("match scan")) != BN_OK) return st;
    }
    const Rows r = Rows::view(a->d_rows, batch, a->M);
    hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)batch), dim3(64), 0, stream, a->d_cand, a->d_cand_len, passes * QP, (int)n_wg, M,
                       bn::index_tags(a->index), r.id, r.score, r.tag, r.count);
    if ((st = check_launch("match merge")) != BN_OK) return st;
    const bn::OutRegion reg{a->h_rows, a->d_rows, Rows::bytes(batch, a->M)};
    return bn::results_to_host(stream, &reg, 1);
}

}  // namespace

bn_status bn::match_attach(bn_index *x, int device, bool has_embedding, size_t embedding_dim, size_t max_batch, size_t top_m, int32_t has_min,
                           float min_score, MatchAttach **out) {
    if (!x || !out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (!has_embedding) return set_last_error(BN_ERR_INVALID_ARG, "the context's model has no embedding output");
    const size_t dim = bn_index_dim(x);
    if (embedding_dim != dim)
        return set_last_error(BN_ERR_INVALID_ARG, "the index's dim " + std::to_string(dim) + " differs from the model's embedding_dim " + std::to_string(embedding_dim));
    const int xdev = bn::index_device(x);
    if (device != xdev) return set_last_error(BN_ERR_INVALID_ARG, "the context lives on device " + std::to_string(device) + ", the index on " + std::to_string(xdev));
    bn_status st = bn::check_top_m(top_m, top_m);
    if (st != BN_OK) return st;
    if ((st = check_threshold(has_min, min_score)) != BN_OK) return st;
    bn::IndexRows v;
    if ((st = bn::index_rows(x, &v)) != BN_OK) return st;  // waits for a pending bn_index_add_ctx: the snapshot's rows are complete
    return make_attach(x, v, max_batch, top_m, has_min, min_score, out);
}

void bn::match_detach(MatchAttach *a) { delete a; }

bn_status bn::match_step(MatchAttach *a, hipStream_t stream, const float *d_emb, size_t batch) {
    if (batch > a->max_batch) return set_last_error(BN_ERR_INVALID_ARG, "batch exceeds the context's max_batch");
    bn_status st = enqueue_match(a, stream, d_emb, a->dim, batch);
    if (st != BN_OK) return st;
    a->last_batch = batch;
    a->stepped = true;
    return BN_OK;
}

bn_status bn::match_step_results(const MatchAttach *a, const uint64_t **id, const float **score, const uint32_t **tag, const uint32_t **count,
                                 size_t *m_stride, size_t *rows_searched) {
    if (!a || !a->stepped) return set_last_error(BN_ERR_INVALID_ARG, "no step has run on this context since an index was attached");
    const Rows r = Rows::view(a->h_rows, a->last_batch, a->M);
    if (id) *id = r.id;
    if (score) *score = r.score;
    if (tag) *tag = r.tag;
    if (count) *count = r.count;
    if (m_stride) *m_stride = a->M;
    if (rows_searched) *rows_searched = a->n;
    return BN_OK;
}

extern "C" {

bn_status bn_index_match(bn_index *x, const float *rows, size_t n, size_t top_m, int32_t has_min, float min_score, size_t m_stride, uint64_t *id_out,
                         float *score_out, uint32_t *tag_out, uint32_t *count_out) {
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    bn_status st = bn::check_top_m(top_m, m_stride);
    if (st != BN_OK) return st;
    if ((st = check_threshold(has_min, min_score)) != BN_OK) return st;
    if (n && (!rows || !id_out || !score_out || !tag_out || !count_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!n) return BN_OK;
    bn::IndexRows v;
    if ((st = bn::index_rows(x, &v)) != BN_OK) return st;
    // an attachment of one call, on the index's stream: the same snapshot, scratch and kernels as a step's
    bn::MatchAttach *raw = nullptr;
    if ((st = make_attach(x, v, std::min(n, ROUND), top_m, has_min, min_score, &raw)) != BN_OK) return st;
    std::unique_ptr<bn::MatchAttach> a(raw);
    hipStream_t stream = bn::index_stream(x);
    bn::Scratch stage;  // waits for the stream before the attachment goes
    stage.stream = stream;
    float *d_stage = nullptr;
    BN_HIP_TRY(stage.alloc(&d_stage, a->max_batch * v.dim * sizeof(float)));
    for (size_t r0 = 0; r0 < n; r0 += ROUND) {
        const size_t k = std::min(ROUND, n - r0);
        BN_HIP_TRY(bn::gated::Memcpy(d_stage, rows + r0 * v.dim, k * v.dim * sizeof(float), hipMemcpyHostToDevice));
        if ((st = enqueue_match(a.get(), stream, d_stage, v.dim, k)) != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(stream));
        const Rows r = Rows::view(a->h_rows, k, top_m);
        for (size_t i = 0; i < k; i++) {
            const uint32_t c = r.count[i];
            count_out[r0 + i] = c;
            for (uint32_t j = 0; j < c; j++) {
                id_out[(r0 + i) * m_stride + j] = r.id[i * top_m + j];
                score_out[(r0 + i) * m_stride + j] = r.score[i * top_m + j];
                tag_out[(r0 + i) * m_stride + j] = r.tag[i * top_m + j];
            }
        }
    }
    return BN_OK;
}

}  // extern "C"
