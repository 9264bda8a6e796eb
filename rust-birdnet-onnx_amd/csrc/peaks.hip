// bn_index_search_peaks / bn_index_search_peaks_ids behind the C ABI (include/birdnet_hip.h): the exact top-M cosine search of index.hip
// restricted to the LOCAL PEAKS over row ids.  A row is a peak of a query when no other eligible row within peak_radius ids of it comes
// before it in the search's order (score descending, ties by id ascending); the result is the first top_m peaks in that order.  Scores
// have bn_index_search's bits, and peak_radius == 0 is bn_index_search itself.
//
// Kernel of this file:
//   * peaks_scan_kernel<QB> -- index_scan_kernel's tile loop written out once more: 64 queries per pass in LDS, the exact-f32
//     MFMA v_mfma_f32_16x16x4_f32 with row = A operand and query = B operand, one accumulator per (query, row) over k ascending.  It shares
//     index_scan.h's constants and LDS layout (three score planes); the loop is this file's own (as an instantiation of one templated body
//     it measured 1 to 3 % slower at 32 and 128 queries: DESIGN.md).  What differs from index_scan_kernel lies between the MFMA and
//     the selection.  The scores of THREE consecutive tiles stay in LDS (a ring of [QP][S_LD] planes, tile t in plane t mod 3); a pair that
//     is not eligible (row invalid or past the end, id within the exclusion radius of the query's own) is stored as -inf, which can
//     neither be a peak nor come before a finite score, from a validity word and query ids fetched ahead of the tile's MFMAs.  Tile t - 1
//     is judged when tile t's scores land: lane = row, the lane's 2 * radius neighbours read from the ring (consecutive lanes read
//     consecutive words of one query's line, and the planes are a multiple of 64 words apart: no bank conflict), and only peaks enter the
//     threshold-and-pending path.  A workgroup owns a contiguous run of tiles and computes, for their scores alone, the tile before and
//     the tile after its run where they exist; those scores have the same bits in every workgroup, so no workgroup talks to another.  The
//     sorted candidates go to the index's own buffers; index_merge_kernel (run_scan_passes) finishes the query.  LDS: index_scan_kernel's
//     125 184 B + two more score planes = 158 464 B (opted in per device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "index_scan.h"
#include "topm_select.h"

namespace {

using bn::scan::KC;
using bn::scan::PLANE;
using bn::scan::QS_LD;
using bn::scan::S_LD;
using bn::scan::TILE;
constexpr int QP = bn::scan::LP;  // queries per scan pass
constexpr int RING = 3;           // tiles whose scores are kept: the judged one and its two neighbours
static_assert(BN_PEAK_RADIUS_MAX <= TILE, "a row's neighbours must lie in its own tile and the two adjacent ones");

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;  // the search's order: score descending, ties by id ascending

constexpr size_t PEAKS_LDS = bn::scan::Layout<RING>::BYTES;  // index_scan_kernel's + two more score planes

// Scan of one pass (nq <= QP queries, QB = ceil(nq / 16) query blocks), R = peak_radius in 1..TILE.  Workgroup g owns tiles
// [g * tiles_per_wg, ...) and computes one tile more on either side where the index has one.  Operands as in index_scan_kernel: lane l
// of wave w: A = row (tile row 16w + (l & 15)), k = 16s + 4(l >> 4) + c of each KC chunk; B = query 16qb + (l & 15) at the same k.
// D: query 16qb + (l & 15), row 16w + 4(l >> 4) + reg.  Out: cand[g][query][..] sorted, the first M kept; cand_len[g][query].
template <int QB>
__global__ __launch_bounds__(256) void peaks_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t n_rows,
                                                         uint32_t dpad, const float *__restrict__ q, const uint8_t *__restrict__ qvalid, int nq,
                                                         const uint32_t *__restrict__ qid, int64_t radius, int R, int M, uint32_t tiles_per_wg,
                                                         Cand *__restrict__ cand, int *__restrict__ cand_len) {
    extern __shared__ __align__(16) char pk_lds[];
    using L = bn::scan::Layout<RING>;                              // the shared layout with three score planes
    float *Qs = reinterpret_cast<float *>(pk_lds + L::B);         // [QP][QS_LD]: the queries' current k chunk
    float *S = reinterpret_cast<float *>(pk_lds + L::S);          // [RING][QP][S_LD]: scores of tile t in plane t mod 3, -inf where not eligible
    Cand *pend = reinterpret_cast<Cand *>(pk_lds + L::PENDING);   // [QP][PEND]
    Cand *scratch = reinterpret_cast<Cand *>(pk_lds + L::SCRATCH);  // [4][MMAX]
    Cand *thr = reinterpret_cast<Cand *>(pk_lds + L::THR);        // [QP]
    int *len = reinterpret_cast<int *>(pk_lds + L::LEN);          // [QP]
    int *pn = reinterpret_cast<int *>(pk_lds + L::PN);            // [QP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < QP; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    const uint32_t n_tiles = (n_rows + TILE - 1) / TILE;
    const uint32_t t0 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)blockIdx.x * tiles_per_wg);
    const uint32_t t1 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)t0 + tiles_per_wg);
    // the tiles computed: the run and its halo
    const uint32_t c0 = t0 > 0 && t0 < t1 ? t0 - 1 : t0;
    const uint32_t c1 = t0 < t1 && t1 < n_tiles ? t1 + 1 : t1;
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (c1 - c0) * nkc;
    Cand *my_cand = cand + (size_t)blockIdx.x * QP * MMAX;
    const float NEG_INF = -__builtin_inff();

    // the ids of this lane's queries (D mapping), for the exclusion test at the store
    int64_t my_qid[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) my_qid[b] = (radius >= 0 && b * 16 + r16 < nq) ? (int64_t)qid[b * 16 + r16] : 0;

    auto row_ptr = [&](uint32_t t, uint32_t c) {
        const size_t row = (size_t)t * TILE + w * 16 + r16;  // < the slab's rows (padded to TILE)
        return slab + row * dpad + c * KC + 4 * h;
    };
    constexpr int QV = QB * 16 * (KC / 4) / 256;  // float4 of the query chunk per thread
    auto load_q = [&](uint32_t c, float4 *qr) {
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            qr[j] = qq < nq ? *reinterpret_cast<const float4 *>(q + (size_t)qq * dpad + c * KC + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // the valid bytes of the four rows this lane stores (D mapping) of tile t: one aligned word
    auto valid_word = [&](uint32_t t) { return *reinterpret_cast<const uint32_t *>(valid + (size_t)t * TILE + w * 16 + h * 4); };

    // Judgment and selection of tile j, whose scores lie in plane pc, tile j - 1's in pp and tile j + 1's in px (each read only where the
    // index has such rows).  Wave w owns queries w, w + 4, ...; lane = row.
    auto judge = [&](uint32_t j, int pc, int pp, int px) {
        const uint32_t grow = j * TILE + lane;
        const float *Pc = S + pc * PLANE, *Pp = S + pp * PLANE, *Px = S + px * PLANE;
        for (int qq = w; qq < nq; qq += 4) {
            if (!qvalid[qq]) continue;
            const float s = Pc[qq * S_LD + lane];
            const Cand e{s, grow};
            int L = len[qq];
            // a row that would not enter the list needs no judgment
            bool alive = s > NEG_INF && (L < M || Ord::ahead(e, thr[qq]));
            if (!__ballot(alive)) continue;
            for (int d = 1; d <= R; d++) {
                if (grow >= (uint32_t)d) {  // row grow - d exists; with the lower id it wins a tie
                    const int o = lane - d;
                    const float v = (o >= 0 ? Pc : Pp)[qq * S_LD + (o & (TILE - 1))];
                    alive = alive && !(v >= s);
                }
                if ((uint64_t)grow + d < n_rows) {  // row grow + d exists
                    const int o = lane + d;
                    const float v = (o < TILE ? Pc : Px)[qq * S_LD + (o & (TILE - 1))];
                    alive = alive && !(v > s);
                }
                if (!__ballot(alive)) break;
            }
            const uint64_t m = __ballot(alive);
            if (!m) continue;
            int np = pn[qq];
            if (np + 64 > PEND) {
                L = merge_pending<Ord>(pend + qq * PEND, np, my_cand + qq * MMAX, L, M, scratch + w * MMAX, thr + qq);
                np = 0;
            }
            if (alive) pend[qq * PEND + np + lanes_below(m)] = e;
            wave_sync();
            if (lane == 0) {
                len[qq] = L;
                pn[qq] = np + __popcll(m);
            }
            wave_sync();
        }
    };

    float4 a[8], qr[QV];
    if (steps) {
        const float *rp = row_ptr(c0, 0);
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
        load_q(0, qr);
    }
    floatx4 acc[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};

    // step u = (tile t, chunk ck); the row chunk and the query chunk of step u + 1 are loaded during step u
    uint32_t t = c0, ck = 0, vw = 0;
    int plane = 0;  // of tile t: (t - c0) mod 3
    for (uint32_t u = 0; u < steps; u++) {
        __syncthreads();  // the previous chunk's Qs reads are done
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            *reinterpret_cast<float4 *>(Qs + qq * QS_LD + kk) = qr[j];
        }
        __syncthreads();
        if (ck == 0) vw = valid_word(t);  // ahead of the tile's MFMAs: nothing is loaded between the last of them and the store
        const uint32_t ck1 = ck + 1 == nkc ? 0 : ck + 1;
        float4 an[8];
        if (u + 1 < steps) {
            const float *rp = row_ptr(ck1 ? t : t + 1, ck1);
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

        // ---- end of tile t: its scores to the ring with eligibility written in, then the judgment of tile t - 1
        float *P = S + plane * PLANE;
        const uint32_t row0 = t * TILE + w * 16 + h * 4;
#pragma unroll
        for (int b = 0; b < QB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                bool ok = row0 + r < n_rows && ((vw >> (8 * r)) & 0xffu);
                if (radius >= 0) {
                    const int64_t d = (int64_t)(row0 + r) - my_qid[b];
                    ok = ok && (d > radius || d < -radius);
                }
                P[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = ok ? acc[b][r] : NEG_INF;
            }
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const int before = plane == 0 ? 2 : plane - 1, before2 = before == 0 ? 2 : before - 1;
        if (t > t0) judge(t - 1, before, before2, plane);
        if (t + 1 == c1 && t < t1) judge(t, plane, before, before2);  // the index's last tile: no tile follows, the third plane is not read
        plane = plane == 2 ? 0 : plane + 1;
        t++;
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

using bn::set_last_error;

// bn_index_search's refusals of its arguments, in its order, with the radius before the null arguments; none needs the index or a device
bn_status check_args(const void *queries, size_t n_queries, size_t peak_radius, size_t top_m, size_t m_stride, const uint64_t *id_out,
                     const float *score_out, const uint32_t *count_out) {
    if (bn_status st = bn::check_top_m(top_m, m_stride); st != BN_OK) return st;
    if (peak_radius > BN_PEAK_RADIUS_MAX)
        return set_last_error(BN_ERR_INVALID_ARG, "peak_radius must be in 0.." + std::to_string(BN_PEAK_RADIUS_MAX) + ", got " + std::to_string(peak_radius));
    return bn::check_search_buffers(queries, n_queries, id_out, score_out, count_out);
}

// Per round the scan + merge passes over the staged queries, results through the index's pinned mirrors.  The tiles are split among
// the workgroups as bn_index_search splits them: the result does not depend on the split, and the two halo tiles cost the least time
// where a workgroup's run is shortest
bn_status search(bn_index *ix, const bn::QuerySource &src, size_t n_queries, size_t peak_radius, size_t top_m, size_t m_stride, uint64_t *id_out,
                 float *score_out, uint32_t *count_out) {
    bn_status st = check_args(src.data(), n_queries, peak_radius, top_m, m_stride, id_out, score_out, count_out);
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!ix) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (peak_radius == 0)  // every eligible row is a peak: the exact search itself
        return src.ids ? bn_index_search_ids(ix, src.ids, n_queries, src.radius, top_m, m_stride, id_out, score_out, count_out)
                       : bn_index_search(ix, src.rows, n_queries, top_m, m_stride, id_out, score_out, count_out);
    if ((st = bn::check_query_ids(src, n_queries, bn_index_size(ix))) != BN_OK) return st;
    if (bn_index_size(ix) == 0) {  // no launch
        std::fill(count_out, count_out + n_queries, 0u);
        return BN_OK;
    }
    bn::IndexScan x;
    if ((st = bn::index_scan_state(ix, &x)) != BN_OK) return st;
    BN_HIP_TRY(g_scan_lds.prepare(x.device, {{(const void *)peaks_scan_kernel<1>, PEAKS_LDS}, {(const void *)peaks_scan_kernel<2>, PEAKS_LDS},
                                              {(const void *)peaks_scan_kernel<3>, PEAKS_LDS}, {(const void *)peaks_scan_kernel<4>, PEAKS_LDS}}));
    const int R = (int)peak_radius, M = (int)top_m;
    const bn::WgSplit sp = bn::split_tiles((uint32_t)((x.size + TILE - 1) / TILE), x.max_wg);
    return bn::for_each_round(ix, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) -> bn_status {
        bn_status rs = bn::run_scan_passes(x, nq, sp.n_wg, M, "peaks scan", [&](size_t p0, int np) {
            const bn::StagedQueries q = staged.at(p0);
            bn::by_blocks(np, [&](auto qb) {
                hipLaunchKernelGGL(peaks_scan_kernel<decltype(qb)::value>, dim3(sp.n_wg), dim3(256), PEAKS_LDS, x.stream, x.slab, x.valid, (uint32_t)x.size,
                                   (uint32_t)x.dpad, q.d_q, q.d_qvalid, np, q.d_qid, q.radius, R, M, sp.tiles_per_wg, x.d_cand, x.d_cand_len);
            });
        });
        if (rs == BN_OK) bn::scatter_results(x, q0, nq, top_m, m_stride, id_out, score_out, count_out);
        return rs;
    });
}

}  // namespace

extern "C" {

bn_status bn_index_search_peaks(bn_index *x, const float *queries, size_t n_queries, size_t peak_radius, size_t top_m, size_t m_stride,
                                uint64_t *id_out, float *score_out, uint32_t *count_out) {
    return search(x, bn::QuerySource::host(queries), n_queries, peak_radius, top_m, m_stride, id_out, score_out, count_out);
}

bn_status bn_index_search_peaks_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t peak_radius,
                                    size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out) {
    return search(x, bn::QuerySource::stored(query_ids, exclude_radius), n_queries, peak_radius, top_m, m_stride, id_out, score_out, count_out);
}

}  // extern "C"
