// bn_index_search_seq / bn_index_search_seq_ids behind the C ABI (include/birdnet_hip.h): a query is a RUN of seq_len consecutive
// windows, and start row i of the index scores the mean of the seq_len window scores along the diagonal, score(i) = mean_j
// dot(query_j, row[i + j]), summed in j order in f32 and multiplied once by fl32(1 / seq_len).  Window scores have bn_index_search's
// bits; the result is the first top_m eligible starts (or, with a peak radius, local peaks over start ids by bn_index_search_peaks'
// rule) in the search's order.
//
// Kernel of this file:
//   * seq_scan_kernel<QB> -- index_scan_kernel's tile loop written out once more, as peaks.hip writes it: 64 query rows per pass in
//     LDS, the exact-f32 MFMA v_mfma_f32_16x16x4_f32 with row = A operand and query = B operand, one accumulator per (query row, index
//     row) over k ascending, index_scan.h's constants and Layout<2>.  A pass holds P = min(64 / L, CAP) sequences; window j of
//     sequence p is query slot p * L + j.  The window scores of TWO consecutive tiles stay in LDS (tile t in plane t mod 2, an
//     invalid index row or one past the end as -inf).  When tile t + 1 lands, wave w takes sequences w, w + 4, ... and its lane =
//     start row of tile t: the L reads of the diagonal (for a fixed j consecutive lanes read consecutive words, the two planes a
//     multiple of 32 words apart: no bank conflict), L - 1 adds, one multiply; a start past size - L or inside the exclusion radius
//     becomes -inf, and a sum over an invalid row is -inf by itself.  The sequence scores go into a ring of three [P][64] planes
//     behind Layout<2>; tile t - 1 is judged from it by peaks.hip's rule when tile t's sequence scores exist (peak_radius 0: tile t at
//     once), and survivors enter topm_select.h's threshold-and-pending path, one candidate list per SEQUENCE.  A workgroup owns a
//     contiguous run of tiles and computes, for their scores alone, one tile before and up to two after its run (none before and one
//     after at peak_radius 0); those scores have the same bits in every workgroup, so no workgroup talks to another.
//     index_merge_kernel (run_scan_passes) finishes each sequence.  LDS: seq_plan.h, 163 552 B (opted in per device).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "index_scan.h"
#include "seq_plan.h"
#include "topm_select.h"

namespace {

using bn::scan::KC;
using bn::scan::PLANE;
using bn::scan::QS_LD;
using bn::scan::S_LD;
using bn::scan::TILE;
constexpr int QP = bn::scan::LP;  // query rows per scan pass, and the candidate lists a workgroup has room for
constexpr int RING = 2;           // tiles whose window scores are kept: a start's windows lie in its own tile and the next
constexpr int CAP = bn::seq::CAP;
constexpr int ZPLANE = CAP * TILE;  // words of one tile's sequence scores
static_assert(TILE == bn::seq::TILE && QP == bn::seq::SLOTS && bn::scan::Layout<RING>::BYTES == bn::seq::SCAN_LDS, "seq_plan.h restates index_scan.h");

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;
using Ord = bn::topm::ScoreDesc;  // the search's order: score descending, ties by id ascending

constexpr size_t SEQ_LDS = bn::seq::Lds::BYTES;

// Scan of one pass: ns <= CAP sequences of L windows in query slots [0, ns * L), QB = ceil(ns * L / 16) query blocks; inv = fl32(1 / L);
// R = peak_radius in 0..TILE.  Workgroup g owns tiles [g * tiles_per_wg, ...) and computes bn::seq::computed_tiles of them.  Operands as
// in index_scan_kernel: lane l of wave w: A = row (tile row 16w + (l & 15)), k = 16s + 4(l >> 4) + c of each KC chunk; B = query slot
// 16qb + (l & 15) at the same k.  D: slot 16qb + (l & 15), row 16w + 4(l >> 4) + reg.  qid: the ids of the query rows (_ids form, else
// NULL): sequence p starts at qid[p * L].  Out: cand[g][sequence][..] sorted, the first M kept; cand_len[g][sequence].
template <int QB>
__global__ __launch_bounds__(256) void seq_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t n_rows,
                                                       uint32_t dpad, const float *__restrict__ q, const uint8_t *__restrict__ qvalid, int ns, int L,
                                                       float inv, const uint32_t *__restrict__ qid, int64_t radius, int R, int M,
                                                       uint32_t tiles_per_wg, Cand *__restrict__ cand, int *__restrict__ cand_len) {
    extern __shared__ __align__(16) char sq_lds[];
    using Lay = bn::scan::Layout<RING>;
    float *Qs = reinterpret_cast<float *>(sq_lds + Lay::B);           // [QP][QS_LD]: the query rows' current k chunk
    float *S = reinterpret_cast<float *>(sq_lds + Lay::S);            // [RING][QP][S_LD]: window scores of tile t in plane t mod 2
    Cand *pend = reinterpret_cast<Cand *>(sq_lds + Lay::PENDING);     // [QP][PEND], one line per sequence
    Cand *scratch = reinterpret_cast<Cand *>(sq_lds + Lay::SCRATCH);  // [4][MMAX]
    Cand *thr = reinterpret_cast<Cand *>(sq_lds + Lay::THR);          // [QP]
    int *len = reinterpret_cast<int *>(sq_lds + Lay::LEN);            // [QP]
    int *pn = reinterpret_cast<int *>(sq_lds + Lay::PN);              // [QP]
    float *Z = reinterpret_cast<float *>(sq_lds + bn::seq::Lds::Z);   // [3][CAP][TILE]: sequence scores of tile t in plane t mod 3
    uint32_t *first = reinterpret_cast<uint32_t *>(sq_lds + bn::seq::Lds::FIRST);  // [CAP]
    int *sok = reinterpret_cast<int *>(sq_lds + bn::seq::Lds::OK);    // [CAP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const int nq = ns * L;  // query rows
    for (int i = tid; i < QP; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    if (tid < ns) {
        bool ok = true;
        for (int j = 0; j < L; j++) ok = ok && qvalid[tid * L + j];
        sok[tid] = ok;
        first[tid] = qid ? qid[tid * L] : 0u;
    }
    const uint32_t n_tiles = (n_rows + TILE - 1) / TILE;
    const uint32_t t0 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)blockIdx.x * tiles_per_wg);
    const uint32_t t1 = (uint32_t)min((uint64_t)n_tiles, (uint64_t)t0 + tiles_per_wg);
    // the tiles computed: the run and its halo
    const bn::seq::Computed ct = bn::seq::computed_tiles(t0, t1, n_tiles, (size_t)R);
    const uint32_t c0 = ct.c0, c1 = ct.c1;
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (c1 - c0) * nkc;
    Cand *my_cand = cand + (size_t)blockIdx.x * QP * MMAX;
    const float NEG_INF = -__builtin_inff();

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
    // planes of the two rings by tile; zplane also for the tile before c0, which is then never read
    auto splane = [&](uint32_t t) { return (int)((t - c0) & 1); };
    auto zplane = [&](uint32_t t) { return (int)((t + 3 - c0) % 3); };

    // Sequence scores of the starts of tile zt, whose window scores lie in S plane pc and tile zt + 1's in pn1.  Every lane with
    // lane + j >= 64 loads from pn1, also where the index has no tile zt + 1 and the plane is stale or was never written; such a start
    // does not fit (start + L > n_rows), so what it loaded is discarded for -inf.  Wave w owns sequences w, w + 4, ...; lane = start row.
    auto seq_scores = [&](uint32_t zt, int pc, int pn1) {
        const uint32_t start = zt * TILE + lane;
        const bool fits = (uint64_t)start + (uint32_t)L <= n_rows;
        float *Zt = Z + zplane(zt) * ZPLANE;
        for (int p = w; p < ns; p += 4) {
            if (!sok[p]) continue;
            const float *A = S + pc * PLANE + p * L * S_LD, *B = S + pn1 * PLANE + p * L * S_LD;
            float acc = A[lane];
            for (int j = 1; j < L; j++) {
                const int o = lane + j;
                acc = __fadd_rn(acc, (o < TILE ? A : B)[j * S_LD + (o & (TILE - 1))]);
            }
            bool ok = fits;
            if (radius >= 0) {
                const int64_t d = (int64_t)start - (int64_t)first[p];
                ok = ok && (d > radius || d < -radius);
            }
            Zt[p * TILE + lane] = ok ? __fmul_rn(acc, inv) : NEG_INF;
        }
    };

    // Judgment and selection of the starts of tile j, whose sequence scores lie in Z plane pc, tile j - 1's in pp and tile j + 1's in px
    // (each read only where the index has such rows): peaks.hip's judge over the sequence scores.  Wave w owns sequences w, w + 4, ...
    auto judge = [&](uint32_t j, int pc, int pp, int px) {
        const uint32_t grow = j * TILE + lane;
        const float *Pc = Z + pc * ZPLANE, *Pp = Z + pp * ZPLANE, *Px = Z + px * ZPLANE;
        for (int p = w; p < ns; p += 4) {
            if (!sok[p]) continue;
            const float s = Pc[p * TILE + lane];
            const Cand e{s, grow};
            int Ln = len[p];
            // a start that would not enter the list needs no judgment
            bool alive = s > NEG_INF && (Ln < M || Ord::ahead(e, thr[p]));
            if (!__ballot(alive)) continue;
            for (int d = 1; d <= R; d++) {
                if (grow >= (uint32_t)d) {  // start grow - d exists; with the lower id it wins a tie
                    const int o = lane - d;
                    const float v = (o >= 0 ? Pc : Pp)[p * TILE + (o & (TILE - 1))];
                    alive = alive && !(v >= s);
                }
                if ((uint64_t)grow + d < n_rows) {  // row grow + d exists
                    const int o = lane + d;
                    const float v = (o < TILE ? Pc : Px)[p * TILE + (o & (TILE - 1))];
                    alive = alive && !(v > s);
                }
                if (!__ballot(alive)) break;
            }
            const uint64_t m = __ballot(alive);
            if (!m) continue;
            int np = pn[p];
            if (np + 64 > PEND) {
                Ln = merge_pending<Ord>(pend + p * PEND, np, my_cand + p * MMAX, Ln, M, scratch + w * MMAX, thr + p);
                np = 0;
            }
            if (alive) pend[p * PEND + np + lanes_below(m)] = e;
            wave_sync();
            if (lane == 0) {
                len[p] = Ln;
                pn[p] = np + __popcll(m);
            }
            wave_sync();
        }
    };
    // what can be judged once the sequence scores of tile zt exist; only tiles of the workgroup's own run are judged
    auto judge_after = [&](uint32_t zt) {
        auto mine = [&](uint32_t t) { return t >= t0 && t < t1; };
        if (R == 0) {
            if (mine(zt)) judge(zt, zplane(zt), 0, 0);
            return;
        }
        if (zt >= 1 && mine(zt - 1)) judge(zt - 1, zplane(zt - 1), zplane(zt - 2), zplane(zt));
        if (zt + 1 == n_tiles && mine(zt)) judge(zt, zplane(zt), zplane(zt - 1), 0);  // the index's last tile: no tile follows
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

        // ---- end of tile t: its window scores to the ring, then the sequence scores of tile t - 1 and what they let be judged
        float *P = S + splane(t) * PLANE;
        const uint32_t row0 = t * TILE + w * 16 + h * 4;
#pragma unroll
        for (int b = 0; b < QB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const bool ok = row0 + r < n_rows && ((vw >> (8 * r)) & 0xffu);
                P[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = ok ? acc[b][r] : NEG_INF;
            }
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        if (t > c0) {
            seq_scores(t - 1, splane(t - 1), splane(t));
            __syncthreads();
            judge_after(t - 1);
        }
        if (t + 1 == n_tiles) {  // the index's last tile: no start of it reaches past it
            __syncthreads();     // the judgment above has read the Z plane written next
            seq_scores(t, splane(t), splane(t) ^ 1);
            __syncthreads();
            judge_after(t);
        }
        t++;
    }
    __syncthreads();
    for (int p = w; p < ns; p += 4) {
        int Ln = len[p];
        const int np = pn[p];
        if (np) Ln = merge_pending<Ord>(pend + p * PEND, np, my_cand + p * MMAX, Ln, M, scratch + w * MMAX, thr + p);
        if (lane == 0) cand_len[blockIdx.x * QP + p] = Ln;
    }
}

bn::LdsOptIn g_scan_lds;

using bn::set_last_error;

// The source's unit is a sequence: seq_len host rows, or the stored rows [first id, + seq_len).  Per round (as many sequences as the
// index's query buffers hold rows for) the scan + merge passes over the staged sequences, results through the index's pinned mirrors.
// The tiles are split among the workgroups as bn_index_search splits them: the result does not depend on the split
bn_status search(bn_index *ix, const bn::QuerySource &src, size_t n_seq, size_t seq_len, size_t peak_radius, size_t top_m, size_t m_stride,
                 uint64_t *id_out, float *score_out, uint32_t *count_out) {
    bn_status st = bn::seq::check_args(src.data(), n_seq, seq_len, peak_radius, top_m, m_stride, id_out, score_out, count_out);
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!ix) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    const size_t size = bn_index_size(ix);
    if (src.ids && (st = bn::seq::check_first_ids(src.ids, n_seq, seq_len, size)) != BN_OK) return st;
    if (size < seq_len) {  // no start is eligible: no launch
        std::fill(count_out, count_out + n_seq, 0u);
        return BN_OK;
    }
    bn::IndexScan x;
    if ((st = bn::index_scan_state(ix, &x)) != BN_OK) return st;
    BN_HIP_TRY(g_scan_lds.prepare(x.device, {{(const void *)seq_scan_kernel<1>, SEQ_LDS}, {(const void *)seq_scan_kernel<2>, SEQ_LDS},
                                              {(const void *)seq_scan_kernel<3>, SEQ_LDS}, {(const void *)seq_scan_kernel<4>, SEQ_LDS}}));
    const int L = (int)seq_len, R = (int)peak_radius, M = (int)top_m;
    const float inv = 1.0f / (float)L;
    const bn::WgSplit sp = bn::split_tiles((uint32_t)((x.size + TILE - 1) / TILE), x.max_wg);
    x.lists = (size_t)bn::seq::per_pass(seq_len);  // a pass of run_scan_passes is that many lists: one per sequence
    return bn::for_each_round(ix, src, n_seq, seq_len, [&](size_t s0, size_t ns, const bn::StagedQueries &staged) -> bn_status {
        bn_status rs = bn::run_scan_passes(x, ns, sp.n_wg, M, "sequence scan", [&](size_t p0, int np) {
            const bn::StagedQueries q = staged.at(p0 * L);
            bn::by_blocks(np * L, [&](auto qb) {
                hipLaunchKernelGGL(seq_scan_kernel<decltype(qb)::value>, dim3(sp.n_wg), dim3(256), SEQ_LDS, x.stream, x.slab, x.valid, (uint32_t)x.size,
                                   (uint32_t)x.dpad, q.d_q, q.d_qvalid, np, L, inv, q.d_qid, q.radius, R, M, sp.tiles_per_wg, x.d_cand, x.d_cand_len);
            });
        });
        if (rs == BN_OK) bn::scatter_results(x, s0, ns, top_m, m_stride, id_out, score_out, count_out);
        return rs;
    });
}

}  // namespace

extern "C" {

bn_status bn_index_search_seq(bn_index *x, const float *queries, size_t n_seq, size_t seq_len, size_t peak_radius, size_t top_m, size_t m_stride,
                              uint64_t *id_out, float *score_out, uint32_t *count_out) {
    return search(x, bn::QuerySource::host(queries), n_seq, seq_len, peak_radius, top_m, m_stride, id_out, score_out, count_out);
}

bn_status bn_index_search_seq_ids(bn_index *x, const uint64_t *first_ids, size_t n_seq, size_t seq_len, int64_t exclude_radius, size_t peak_radius,
                                  size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out) {
    return search(x, bn::QuerySource::stored(first_ids, exclude_radius), n_seq, seq_len, peak_radius, top_m, m_stride, id_out, score_out, count_out);
}

}  // extern "C"
