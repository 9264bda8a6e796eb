// bn_subset_* behind the C ABI (include/birdnet_hip.h): a fixed, ascending list of row ids of one index, chosen by id range and row
// tag (bn_subset_select) or given by the caller (bn_subset_from_ids), and an exact top-M cosine search that reads only those rows,
// once for all queries of a pass.  A search returns what bn_index_search would return if only the list's rows existed, with the same
// score bits, order and tie rule.
//
// Kernels of this file:
//   * subset_select_kernel<SCATTER> -- selection in two launches of one body.  A block evaluates SEL_ROWS consecutive ids of the
//     range: wave w takes four groups of 64 ids in ascending order, one id per lane, and a ballot per group says which pass (in the
//     range, tag admitted by the 65536-bit map; a missing tag plane reads as tag 0).  SCATTER = false stores the block's count.
//     SCATTER = true stores each passing id at the block's offset + the counts of the groups before its own + lanes_below(ballot): a
//     position is a function of the data alone, never of an atomic or of timing, so the ids come out ascending and two selections
//     of the same state give the same bytes.
//   * subset_offsets_kernel -- one workgroup: the exclusive prefix sums of the blocks' counts (integers: exact), the total last.
//   * subset_scan_kernel<QB> -- index_scan_kernel's tile loop written out again over the list: 64 queries per pass in
//     LDS, the exact-f32 MFMA v_mfma_f32_16x16x4_f32 with row = A operand and query = B operand, one accumulator per (query, row) over k
//     ascending, so a score has bn_index_search's bits.  The constants and the LDS layout are index_scan.h's; the loop is this file's
//     own (as an instantiation of one templated body it measured slower: DESIGN.md).  A tile's 64 rows are 64 consecutive list entries;
//     the ids are fetched two tiles ahead of the rows they name, the row chunk one step ahead, and the id and validity a lane judges in
//     the selection at the start of its tile.  Lanes past the list's end read its last member and are masked by position.  Workgroup g
//     owns a contiguous run of list tiles and leaves its sorted candidates in the index's own buffers; index_merge_kernel
//     (run_scan_passes) finishes the query.  LDS: index_scan_kernel's 125 184 B (opted in per device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
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
constexpr int QP = bn::scan::LP;     // queries per scan pass
constexpr uint32_t SEL_ROWS = 1024;  // ids per block of the selection: 4 waves x 4 groups of 64
constexpr uint32_t MAP_WORDS = BN_INDEX_TAG_LIMIT / 32;

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;  // the search's order: score descending, ties by id ascending

constexpr size_t SCAN_LDS = bn::scan::Layout<1>::BYTES;  // index_scan_kernel's

// Block b: ids [first + b * SEL_ROWS, + SEL_ROWS) cut at `end`.  tags NULL: every tag is 0; admit NULL: tags are not tested.
// SCATTER false: block_count[b] = the ids that pass.  SCATTER true: those ids, ascending, to ids_out[block_off[b] ..).
template <bool SCATTER>
__global__ __launch_bounds__(256) void subset_select_kernel(const uint16_t *__restrict__ tags, const uint32_t *__restrict__ admit, uint64_t first,
                                                            uint64_t end, uint32_t *__restrict__ block_count,
                                                            const uint32_t *__restrict__ block_off, uint32_t *__restrict__ ids_out) {
    __shared__ uint32_t wave_n[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t base = first + (uint64_t)blockIdx.x * SEL_ROWS + (uint64_t)w * 256;
    uint64_t m[4];
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint64_t id = base + 64 * j + lane;
        bool pass = id < end;
        if (pass && admit) {
            const uint32_t t = tags ? tags[id] : 0u;
            pass = (admit[t >> 5] >> (t & 31)) & 1u;
        }
        m[j] = __ballot(pass);
        n += (uint32_t)__popcll(m[j]);
    }
    if (lane == 0) wave_n[w] = n;
    __syncthreads();
    if (!SCATTER) {
        if (threadIdx.x == 0) block_count[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        return;
    }
    uint32_t pos = block_off[blockIdx.x];
    for (int i = 0; i < w; i++) pos += wave_n[i];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if ((m[j] >> lane) & 1) ids_out[pos + lanes_below(m[j])] = (uint32_t)(base + 64 * j + lane);
        pos += (uint32_t)__popcll(m[j]);
    }
}

// one workgroup: off[b] = count[0] + .. + count[b - 1] for b in [0, nb]; thread t owns the contiguous blocks [t * per, + per)
__global__ __launch_bounds__(256) void subset_offsets_kernel(const uint32_t *__restrict__ count, uint32_t nb, uint32_t *__restrict__ off) {
    __shared__ uint32_t part[256];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nb + 255) / 256;
    const uint32_t b0 = min(nb, t * per), b1 = min(nb, b0 + per);
    uint32_t s = 0;
    for (uint32_t b = b0; b < b1; b++) s += count[b];
    part[t] = s;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t i = 0; i < t; i++) run += part[i];
    for (uint32_t b = b0; b < b1; b++) {
        off[b] = run;
        run += count[b];
    }
    if (t == 255) off[nb] = run;  // b1 == nb for the last thread
}

// Scan of one pass (nq <= QP queries, QB = ceil(nq / 16) query blocks) over the list ids[0 .. n), n >= 1, every entry the id of a
// stored row.  Tile t of the list holds entries [64 t, 64 t + 64); workgroup g owns tiles [g * tiles_per_wg, ...).  Lane l of wave w:
// A operand = the row named by entry 64 t + 16 w + (l & 15) (clamped to n - 1), k = 16 s + 4 (l >> 4) + c of each KC chunk; B operand =
// query 16 qb + (l & 15) at the same k.  D: query 16 qb + (l & 15), entry 64 t + 16 w + 4 (l >> 4) + reg.
// Out: cand[g][query][..] sorted, the first M kept; cand_len[g][query].
template <int QB>
__global__ __launch_bounds__(256) void subset_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, const uint32_t *__restrict__ ids,
                                                          uint32_t n, uint32_t dpad, const float *__restrict__ q, const uint8_t *__restrict__ qvalid, int nq,
                                                          const uint32_t *__restrict__ qid, int64_t radius, int M, uint32_t tiles_per_wg,
                                                          Cand *__restrict__ cand, int *__restrict__ cand_len) {
    extern __shared__ __align__(16) char sub_lds[];
    using L = bn::scan::Layout<1>;                                  // index_scan_kernel's layout
    float *Qs = reinterpret_cast<float *>(sub_lds + L::B);          // [QP][QS_LD]: the queries' current k chunk
    float *S = reinterpret_cast<float *>(sub_lds + L::S);           // [QP][S_LD]: scores of the current tile
    Cand *pend = reinterpret_cast<Cand *>(sub_lds + L::PENDING);    // [QP][PEND]
    Cand *scratch = reinterpret_cast<Cand *>(sub_lds + L::SCRATCH);  // [4][MMAX]
    Cand *thr = reinterpret_cast<Cand *>(sub_lds + L::THR);         // [QP]
    int *len = reinterpret_cast<int *>(sub_lds + L::LEN);           // [QP]
    int *pn = reinterpret_cast<int *>(sub_lds + L::PN);             // [QP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < QP; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    const uint32_t n_tiles = (n + TILE - 1) / TILE;  // n < 2^32 - 64
    const uint32_t t0 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)blockIdx.x * tiles_per_wg);
    const uint32_t t1 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;
    const uint32_t last = n - 1;
    Cand *my_cand = cand + (size_t)blockIdx.x * QP * MMAX;

    // the entry this lane multiplies in tile t, clamped into the list
    auto member_of = [&](uint64_t t) { return ids[min((uint64_t)last, t * TILE + w * 16 + r16)]; };
    constexpr int QV = QB * 16 * (KC / 4) / 256;  // float4 of the query chunk per thread
    auto load_q = [&](uint32_t c, float4 *qr) {
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            qr[j] = qq < nq ? *reinterpret_cast<const float4 *>(q + (size_t)qq * dpad + c * KC + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // the entry this lane judges in the selection of tile t (entry 64 t + lane), clamped likewise
    auto judged_of = [&](uint64_t t) { return ids[min((uint64_t)last, t * TILE + lane)]; };
    uint32_t id_cur = 0, id_nx = 0, id_nn = 0, sel_cur = 0, sel_nx = 0;
    uint8_t sel_valid = 0;
    float4 a[8], qr[QV];
    if (steps) {
        id_cur = member_of(t0);
        id_nx = member_of((uint64_t)t0 + 1);
        id_nn = id_nx;
        sel_cur = judged_of(t0);
        const float *rp = slab + (size_t)id_cur * dpad + 4 * h;
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
        load_q(0, qr);
    }
    floatx4 acc[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};

    // step u = (tile t0 + tl, chunk ck); the row chunk and the query chunk of step u + 1 are loaded during step u
    uint32_t tl = 0, ck = 0;
    for (uint32_t u = 0; u < steps; u++) {
        __syncthreads();  // the previous chunk's Qs reads are done
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            *reinterpret_cast<float4 *>(Qs + qq * QS_LD + kk) = qr[j];
        }
        __syncthreads();
        if (ck == 0) {  // ids ahead of the rows they name; the judged row's validity ahead of the selection
            id_nn = member_of((uint64_t)t0 + tl + 2);
            sel_nx = judged_of((uint64_t)t0 + tl + 1);
            sel_valid = valid[sel_cur];
        }
        const uint32_t ck1 = ck + 1 == nkc ? 0 : ck + 1;
        float4 an[8];
        if (u + 1 < steps) {
            const float *rp = slab + (size_t)(ck1 ? id_cur : id_nx) * dpad + ck1 * KC + 4 * h;
#pragma unroll
            for (int s = 0; s < 8; s++) an[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
            load_q(ck1, qr);
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
        ck = ck1;
        if (ck1) continue;

        // ---- end of a tile: scores to LDS, then selection (wave w owns queries w, w + 4, ...)
        const uint64_t pos = (uint64_t)(t0 + tl) * TILE + lane;
        tl++;
        id_cur = id_nx;
        id_nx = id_nn;
#pragma unroll
        for (int b = 0; b < QB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = acc[b][r];
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const uint32_t grow = sel_cur;
        const bool row_ok = pos <= last && sel_valid;
        sel_cur = sel_nx;
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

bn::LdsOptIn g_scan_lds;
hipError_t opt_in_scan(int dev) {
    return g_scan_lds.prepare(dev, {{(const void *)subset_scan_kernel<1>, SCAN_LDS}, {(const void *)subset_scan_kernel<2>, SCAN_LDS},
                                    {(const void *)subset_scan_kernel<3>, SCAN_LDS}, {(const void *)subset_scan_kernel<4>, SCAN_LDS}});
}

}  // namespace

struct bn_subset {
    bn_index *x = nullptr;
    int device = 0;
    size_t n = 0;
    bn::DeviceBuf<uint32_t> d_ids;  // [n] ascending ids of stored rows; NULL for an empty subset
    ~bn_subset() {
        if (d_ids) (void)bn::use_device(device);
    }
};

namespace {

using bn::check_launch;
using bn::set_last_error;

// Per round the scan + merge passes over the staged queries, results through the index's pinned mirrors.  The list's tiles are split
// among the workgroups as bn_index_search splits the slab's
bn_status search(bn_subset *s, const bn::QuerySource &src, size_t n_queries, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                 uint32_t *count_out) {
    bn_status st = bn::check_top_m(top_m, m_stride);  // bn_index_search's refusals, in its order, without the index
    if (st != BN_OK) return st;
    if ((st = bn::check_search_buffers(src.data(), n_queries, id_out, score_out, count_out)) != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!s) return set_last_error(BN_ERR_INVALID_ARG, "null subset");
    if ((st = bn::check_query_ids(src, n_queries, bn_index_size(s->x))) != BN_OK) return st;
    if (s->n == 0) {  // no launch
        std::fill(count_out, count_out + n_queries, 0u);
        return BN_OK;
    }
    bn::IndexScan x;
    if ((st = bn::index_scan_state(s->x, &x)) != BN_OK) return st;
    const int M = (int)top_m;
    const bn::WgSplit sp = bn::split_tiles((uint32_t)((s->n + TILE - 1) / TILE), x.max_wg);
    return bn::for_each_round(s->x, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) -> bn_status {
        bn_status rs = bn::run_scan_passes(x, nq, sp.n_wg, M, "subset scan", [&](size_t p0, int np) {
            const bn::StagedQueries q = staged.at(p0);
            bn::by_blocks(np, [&](auto qb) {
                hipLaunchKernelGGL(subset_scan_kernel<decltype(qb)::value>, dim3(sp.n_wg), dim3(256), SCAN_LDS, x.stream, x.slab, x.valid, s->d_ids,
                                   (uint32_t)s->n, (uint32_t)x.dpad, q.d_q, q.d_qvalid, np, q.d_qid, q.radius, M, sp.tiles_per_wg, x.d_cand, x.d_cand_len);
            });
        });
        if (rs == BN_OK) bn::scatter_results(x, q0, nq, top_m, m_stride, id_out, score_out, count_out);
        return rs;
    });
}

// a subset of n ids for index x, the list allocated (n > 0) and not yet written
bn_status make_subset(bn_index *x, int device, size_t n, std::unique_ptr<bn_subset> &s) {
    s.reset(new bn_subset);
    s->x = x;
    s->device = device;
    s->n = n;
    if (n) BN_HIP_TRY(s->d_ids.alloc(n * sizeof(uint32_t)));
    return BN_OK;
}

}  // namespace

bn::SubsetList bn::subset_list(const bn_subset *s) {
    SubsetList l;
    l.x = s->x;
    l.n = s->n;
    l.d_ids = s->d_ids;
    return l;
}

extern "C" {

bn_status bn_subset_select(bn_index *x, const bn_index_filter *f, size_t struct_size, bn_subset **out) {
    if (!out || !f) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (struct_size < sizeof(bn_index_filter))
        return set_last_error(BN_ERR_INVALID_ARG, "struct_size " + std::to_string(struct_size) + " is smaller than bn_index_filter (" +
                                                      std::to_string(sizeof(bn_index_filter)) + " bytes)");
    if (f->flags & ~BN_FILTER_EXCLUDE_TAGS) return set_last_error(BN_ERR_INVALID_ARG, "unknown filter flags " + std::to_string(f->flags));
    const size_t n_tags = f->tags ? f->n_tags : 0;
    for (size_t i = 0; i < n_tags; i++)
        if (f->tags[i] >= BN_INDEX_TAG_LIMIT)
            return set_last_error(BN_ERR_INVALID_ARG, "listed tag " + std::to_string(f->tags[i]) + " is not below " + std::to_string(BN_INDEX_TAG_LIMIT));
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    const size_t size = bn_index_size(x);
    if (f->first_id > size || f->n_ids > size - f->first_id)
        return set_last_error(BN_ERR_INVALID_ARG, "the id range [" + std::to_string(f->first_id) + ", +" + std::to_string(f->n_ids) + ") is not in the index (" +
                                                      std::to_string(size) + " rows)");
    const uint64_t first = f->first_id, end = f->n_ids ? first + f->n_ids : size;
    bn::IndexScan xs;
    bn_status st = bn::index_scan_state(x, &xs);
    if (st != BN_OK) return st;
    BN_HIP_TRY(opt_in_scan(xs.device));
    std::unique_ptr<bn_subset> s;
    if (first == end) {
        if ((st = make_subset(x, xs.device, 0, s)) != BN_OK) return st;
        *out = s.release();
        return BN_OK;
    }
    const uint32_t nb = (uint32_t)((end - first + SEL_ROWS - 1) / SEL_ROWS);
    bn::Scratch tmp;
    tmp.stream = xs.stream;
    uint32_t *d_admit = nullptr, *d_count = nullptr, *d_off = nullptr;
    BN_HIP_TRY(tmp.alloc(&d_count, (size_t)nb * sizeof(uint32_t)));
    BN_HIP_TRY(tmp.alloc(&d_off, ((size_t)nb + 1) * sizeof(uint32_t)));
    if (n_tags) {
        // the admit map: bit t set when a row of tag t is a member
        std::vector<uint32_t> map(MAP_WORDS, 0u);
        for (size_t i = 0; i < n_tags; i++) map[f->tags[i] >> 5] |= 1u << (f->tags[i] & 31);
        if (f->flags & BN_FILTER_EXCLUDE_TAGS)
            for (uint32_t &wd : map) wd = ~wd;
        BN_HIP_TRY(tmp.alloc(&d_admit, MAP_WORDS * sizeof(uint32_t)));
        BN_HIP_TRY(hipStreamSynchronize(xs.stream));
        BN_HIP_TRY(bn::gated::Memcpy(d_admit, map.data(), MAP_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(subset_select_kernel<false>, dim3(nb), dim3(256), 0, xs.stream, xs.tags, d_admit, first, end, d_count, d_off, (uint32_t *)nullptr);
    if ((st = check_launch("subset count")) != BN_OK) return st;
    hipLaunchKernelGGL(subset_offsets_kernel, dim3(1), dim3(256), 0, xs.stream, d_count, nb, d_off);
    if ((st = check_launch("subset offsets")) != BN_OK) return st;
    uint32_t n = 0;
    BN_HIP_TRY(hipMemcpyAsync(&n, d_off + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, xs.stream));
    BN_HIP_TRY(hipStreamSynchronize(xs.stream));
    if ((st = make_subset(x, xs.device, n, s)) != BN_OK) return st;
    if (n) {
        hipLaunchKernelGGL(subset_select_kernel<true>, dim3(nb), dim3(256), 0, xs.stream, xs.tags, d_admit, first, end, d_count, d_off, s->d_ids);
        if ((st = check_launch("subset scatter")) != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(xs.stream));
    }
    *out = s.release();
    return BN_OK;
}

bn_status bn_subset_from_ids(bn_index *x, const uint64_t *ids, size_t n, bn_subset **out) {
    if (!out || (n && !ids)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    for (size_t i = 1; i < n; i++)
        if (ids[i] <= ids[i - 1])
            return set_last_error(BN_ERR_INVALID_ARG, "ids are not strictly ascending at position " + std::to_string(i) + " (" + std::to_string(ids[i - 1]) +
                                                          " then " + std::to_string(ids[i]) + ")");
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    const size_t size = bn_index_size(x);
    if (n && ids[n - 1] >= size)  // ascending: the last is the largest
        return set_last_error(BN_ERR_INVALID_ARG, "id " + std::to_string(ids[n - 1]) + " is not in the index (" + std::to_string(size) + " rows)");
    bn::IndexScan xs;
    bn_status st = bn::index_scan_state(x, &xs);
    if (st != BN_OK) return st;
    BN_HIP_TRY(opt_in_scan(xs.device));
    std::unique_ptr<bn_subset> s;
    if ((st = make_subset(x, xs.device, n, s)) != BN_OK) return st;
    if (n) {
        const std::vector<uint32_t> v(ids, ids + n);
        BN_HIP_TRY(bn::gated::Memcpy(s->d_ids, v.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    *out = s.release();
    return BN_OK;
}

void bn_subset_free(bn_subset *s) { delete s; }

size_t bn_subset_size(const bn_subset *s) { return s ? s->n : 0; }

bn_status bn_subset_read(const bn_subset *s, size_t first, size_t count, uint64_t *ids_out) {
    if (count && !ids_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!s) return set_last_error(BN_ERR_INVALID_ARG, "null subset");
    if (first > s->n || count > s->n - first) return set_last_error(BN_ERR_INVALID_ARG, "entries out of range");
    if (!count) return BN_OK;
    BN_HIP_TRY(bn::use_device(s->device));
    std::vector<uint32_t> v(count);
    BN_HIP_TRY(bn::gated::Memcpy(v.data(), s->d_ids + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::copy(v.begin(), v.end(), ids_out);
    return BN_OK;
}

bn_status bn_subset_search(bn_subset *s, const float *queries, size_t n_queries, size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out,
                           uint32_t *count_out) {
    if (n_queries && !queries) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return search(s, bn::QuerySource::host(queries), n_queries, top_m, m_stride, id_out, score_out, count_out);
}

bn_status bn_subset_search_ids(bn_subset *s, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t top_m, size_t m_stride,
                               uint64_t *id_out, float *score_out, uint32_t *count_out) {
    if (n_queries && !query_ids) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return search(s, bn::QuerySource::stored(query_ids, exclude_radius), n_queries, top_m, m_stride, id_out, score_out, count_out);
}

}  // extern "C"
