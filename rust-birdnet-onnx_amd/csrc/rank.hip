// bn_head_rank_index behind the C ABI (include/birdnet_hip.h): per class of a head, the top-M stored rows of an index by the
// head's own logit (TOP) or by nearness to the decision boundary (UNCERTAIN), without the slab leaving the device.
//
// Kernels:
//   * rank_exclude_kernel -- clears the listed ids in a per-call copy of the index's validity bytes (plain byte stores of the
//     same value; duplicates are harmless).
//   * rank_scan_kernel -- each workgroup streams its contiguous range of 64-row tiles ONCE for all classes of the pass (up to
//     64).  The products run on v_mfma_f32_16x16x4_f32 in head_apply_kernel's order (head.hip): row = A operand, class = B
//     operand, k = 16 s + 4 (lane >> 4) + t of each 128-wide chunk, s then t ascending, ONE accumulator per (class, row), then
//     the bias added -- so a logit's bits are bn_head_apply_host's on the stored row.  Each tile's [64 classes x 64 rows]
//     logits go to LDS; there a row is masked (outside the id range, invalid or excluded, past the end, NaN logit), and one
//     that beats the class's running M-th candidate joins a pending list; pending lists are merged by rank into the
//     workgroup's running top-M.  A candidate carries the logit itself; the order derives its key from it (topm_select.h:
//     ScoreDesc for TOP, AbsAsc for UNCERTAIN).  Out: [workgroups x classes x M] candidates; no [classes x rows] matrix exists.
//     LDS: index_scan_kernel's constants and layout (index_scan.h).
//   * rank_merge_kernel -- UNCERTAIN: one wave per class merges the workgroups' sorted lists into the final top-M.  TOP's order
//     is the search's, and index_merge_kernel merges it.
// The scan runs on the index's stream and borrows the search's candidate and result buffers (one thread at a time per index).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "index_scan.h"
#include "topm_select.h"

namespace {

using bn::scan::KC;
using bn::scan::S_LD;
using bn::scan::TILE;
constexpr int CP = bn::scan::LP;        // classes per scan pass
constexpr int WS_LD = bn::scan::QS_LD;  // words of a class's k chunk in LDS

using bn::floatx4;
using bn::topm::Cand;
using bn::topm::lanes_below;
using bn::topm::merge_pending;
using bn::topm::MMAX;
using bn::topm::PEND;
using bn::topm::wave_sync;

constexpr size_t SCAN_LDS = bn::scan::Layout<1>::BYTES;

template <uint32_t MODE>
struct OrderOf {
    using type = bn::topm::ScoreDesc;
};
template <>
struct OrderOf<BN_RANK_UNCERTAIN> {
    using type = bn::topm::AbsAsc;
};

__global__ __launch_bounds__(256) void rank_exclude_kernel(const uint32_t *__restrict__ ids, uint32_t n, uint8_t *__restrict__ mask) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) mask[ids[i]] = 0;  // ids[i] < the index's size: checked on the host
}

// Scan of one pass (nc <= CP classes, CB = ceil(nc / 16) class blocks) over the tiles [tile_lo, tile_hi).  Workgroup g owns tiles
// [tile_lo + g * tiles_per_wg, ...).  Lane l of wave w: A operand = row (tile row 16w + (l & 15)), k = 16s + 4(l >> 4) + t of each
// KC chunk (t = component of the float4); B operand = class 16cb + (l & 15) at the same k.  D: class 16cb + (l & 15), row
// 16w + 4(l >> 4) + reg.  W and bias point at the pass's first class; both are padded to 16 classes.
template <int CB, uint32_t MODE>
__global__ __launch_bounds__(256) void rank_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ mask, uint32_t id_lo, uint32_t id_hi,
                                                        uint32_t dpad, const float *__restrict__ W, const float *__restrict__ bias, int nc, int M,
                                                        uint32_t tile_lo, uint32_t tile_hi, uint32_t tiles_per_wg, Cand *__restrict__ cand,
                                                        int *__restrict__ cand_len) {
    using Ord = typename OrderOf<MODE>::type;
    extern __shared__ __align__(16) char rank_lds[];
    using L = bn::scan::Layout<1>;
    float *Ws = reinterpret_cast<float *>(rank_lds + L::B);             // [CP][WS_LD]: the classes' current k chunk
    float *S = reinterpret_cast<float *>(rank_lds + L::S);              // [CP][S_LD]: logits of the current tile
    Cand *pend = reinterpret_cast<Cand *>(rank_lds + L::PENDING);       // [CP][PEND]
    Cand *scratch = reinterpret_cast<Cand *>(rank_lds + L::SCRATCH);    // [4][MMAX]
    Cand *thr = reinterpret_cast<Cand *>(rank_lds + L::THR);            // [CP]
    int *len = reinterpret_cast<int *>(rank_lds + L::LEN);              // [CP]
    int *pn = reinterpret_cast<int *>(rank_lds + L::PN);                // [CP]

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < CP; i += 256) {
        len[i] = 0;
        pn[i] = 0;
    }
    const uint32_t t0 = min(tile_hi, tile_lo + blockIdx.x * tiles_per_wg);
    const uint32_t t1 = min(tile_hi, t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;
    Cand *my_cand = cand + (size_t)blockIdx.x * CP * MMAX;

    // step u = (tile t0 + u / nkc, chunk u % nkc); the row chunk and the class chunk of step u + 1 are loaded during step u
    auto row_ptr = [&](uint32_t u) {
        const size_t row = (size_t)(t0 + u / nkc) * TILE + w * 16 + r16;  // < the slab's rows (padded to TILE)
        return slab + row * dpad + (u % nkc) * KC + 4 * h;
    };
    constexpr int WV = CB * 16 * (KC / 4) / 256;  // float4 of the class chunk per thread
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
    float bv[CB];
#pragma unroll
    for (int b = 0; b < CB; b++) {
        acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        bv[b] = bias[b * 16 + r16];
    }

    for (uint32_t u = 0; u < steps; u++) {
        __syncthreads();  // the previous chunk's Ws reads are done
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

        // ---- end of a tile: logits to LDS, then selection (wave w owns classes w, w + 4, ...)
        const uint32_t t = t0 + u / nkc;
#pragma unroll
        for (int b = 0; b < CB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = acc[b][r] + bv[b];
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const uint32_t grow = t * TILE + lane;
        const bool row_ok = grow >= id_lo && grow < id_hi && mask[grow];
        for (int cc = w; cc < nc; cc += 4) {
            const Cand e{S[cc * S_LD + lane], grow};
            int L = len[cc];
            const bool pass = row_ok && e.s == e.s && (L < M || Ord::ahead(e, thr[cc]));
            const uint64_t m = __ballot(pass);
            if (!m) continue;
            int np = pn[cc];
            if (np + 64 > PEND) {
                L = merge_pending<Ord>(pend + cc * PEND, np, my_cand + cc * MMAX, L, M, scratch + w * MMAX, thr + cc);
                np = 0;
            }
            if (pass) pend[cc * PEND + np + lanes_below(m)] = e;
            wave_sync();
            if (lane == 0) {
                len[cc] = L;
                pn[cc] = np + __popcll(m);
            }
            wave_sync();
        }
    }
    __syncthreads();
    for (int cc = w; cc < nc; cc += 4) {
        int L = len[cc];
        const int np = pn[cc];
        if (np) L = merge_pending<Ord>(pend + cc * PEND, np, my_cand + cc * MMAX, L, M, scratch + w * MMAX, thr + cc);
        if (lane == 0) cand_len[blockIdx.x * CP + cc] = L;
    }
}

// one wave per class: the workgroups' sorted lists -> the final top-M (out [nc][M], count [nc]) in UNCERTAIN's order; TOP's is the
// search's own, and index_merge_kernel (index_enqueue_merge) merges it
__global__ __launch_bounds__(64) void rank_merge_kernel(const Cand *__restrict__ cand, const int *__restrict__ cand_len, int n_wg, int M,
                                                        Cand *__restrict__ out, uint32_t *__restrict__ count) {
    bn::topm::merge_lists<bn::topm::AbsAsc>(cand, cand_len, CP, n_wg, M, out, count);
}

template <uint32_t MODE>
const void *scan_of(int cb) {
    switch (cb) {
        case 1: return reinterpret_cast<const void *>(rank_scan_kernel<1, MODE>);
        case 2: return reinterpret_cast<const void *>(rank_scan_kernel<2, MODE>);
        case 3: return reinterpret_cast<const void *>(rank_scan_kernel<3, MODE>);
        default: return reinterpret_cast<const void *>(rank_scan_kernel<4, MODE>);
    }
}
const void *scan_of(uint32_t mode, int cb) { return mode == BN_RANK_UNCERTAIN ? scan_of<BN_RANK_UNCERTAIN>(cb) : scan_of<BN_RANK_TOP>(cb); }

bn::LdsOptIn g_scan_lds;
hipError_t opt_in_scan(int dev) {
    return g_scan_lds.prepare(dev, {{scan_of(BN_RANK_TOP, 1), SCAN_LDS}, {scan_of(BN_RANK_TOP, 2), SCAN_LDS}, {scan_of(BN_RANK_TOP, 3), SCAN_LDS},
                                    {scan_of(BN_RANK_TOP, 4), SCAN_LDS}, {scan_of(BN_RANK_UNCERTAIN, 1), SCAN_LDS}, {scan_of(BN_RANK_UNCERTAIN, 2), SCAN_LDS},
                                    {scan_of(BN_RANK_UNCERTAIN, 3), SCAN_LDS}, {scan_of(BN_RANK_UNCERTAIN, 4), SCAN_LDS}});
}

bn_status enqueue_abs_merge(hipStream_t stream, const Cand *cand, const int *cand_len, size_t n_classes, int n_wg, int M, Cand *out, uint32_t *count) {
    hipLaunchKernelGGL(rank_merge_kernel, dim3((unsigned)n_classes), dim3(64), 0, stream, cand, cand_len, n_wg, M, out, count);
    return bn::check_launch("rank merge");
}

using bn::check_launch;
using bn::set_last_error;

}  // namespace

extern "C" bn_status bn_head_rank_index(const bn_head *h, bn_index *x, uint32_t mode, uint64_t first_id, uint64_t n_ids, const uint64_t *exclude_ids,
                                        size_t n_exclude, size_t top_m, size_t m_stride, uint64_t *id_out, float *logit_out, uint32_t *count_out) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!h) return set_last_error(BN_ERR_INVALID_ARG, "null head");
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    if (!id_out || !logit_out || !count_out || (n_exclude && !exclude_ids)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (mode != BN_RANK_TOP && mode != BN_RANK_UNCERTAIN) return set_last_error(BN_ERR_INVALID_ARG, "unknown mode " + std::to_string(mode));
    if (bn_status ast = bn::check_top_m(top_m, m_stride); ast != BN_OK) return ast;
    const bn::HeadView hv = bn::head_view(h);
    const size_t size = bn_index_size(x), dim = bn_index_dim(x);
    if (!(hv.flags & BN_HEAD_L2NORM))
        return set_last_error(BN_ERR_INVALID_ARG, "the head lacks BN_HEAD_L2NORM: its weights expect raw embeddings, the index stores normalised rows");
    if (hv.dim != dim) return set_last_error(BN_ERR_INVALID_ARG, "the head's dim " + std::to_string(hv.dim) + " differs from the index's " + std::to_string(dim));
    if (first_id > size || n_ids > size - first_id)
        return set_last_error(BN_ERR_INVALID_ARG, "rows [" + std::to_string(first_id) + ", +" + std::to_string(n_ids) + ") run past the index's " + std::to_string(size) + " rows");
    for (size_t i = 0; i < n_exclude; i++)
        if (exclude_ids[i] >= size) return set_last_error(BN_ERR_INVALID_ARG, "excluded id " + std::to_string(exclude_ids[i]) + " is not in the index");
    bn::IndexScan s;
    bn_status st = bn::index_scan_state(x, &s);
    if (st != BN_OK) return st;
    if (hv.device != s.device) return set_last_error(BN_ERR_INVALID_ARG, "the head lives on device " + std::to_string(hv.device) + ", the index on " + std::to_string(s.device));

    const size_t C = hv.classes, M = top_m;
    const uint32_t id_lo = (uint32_t)first_id, id_hi = (uint32_t)(n_ids ? first_id + n_ids : size);
    if (id_lo == id_hi) {  // an empty index or an empty range
        std::fill(count_out, count_out + C, 0u);
        return BN_OK;
    }
    BN_HIP_TRY(opt_in_scan(s.device));
    bn::Scratch bufs;  // waits for the stream before it frees the mask
    bufs.stream = s.stream;
    const uint8_t *mask = s.valid;
    if (n_exclude) {
        std::vector<uint32_t> ids(exclude_ids, exclude_ids + n_exclude);
        uint8_t *d_mask = nullptr;
        uint32_t *d_ids = nullptr;
        BN_HIP_TRY(bufs.alloc(&d_mask, (s.size + TILE - 1) / TILE * TILE, false));  // whole tiles; the tail lies past id_hi
        BN_HIP_TRY(bufs.alloc(&d_ids, n_exclude * sizeof(uint32_t), false));
        BN_HIP_TRY(bn::gated::Memcpy(d_ids, ids.data(), n_exclude * sizeof(uint32_t), hipMemcpyHostToDevice));
        BN_HIP_TRY(hipMemcpyAsync(d_mask, s.valid, s.size, hipMemcpyDeviceToDevice, s.stream));
        hipLaunchKernelGGL(rank_exclude_kernel, dim3((unsigned)((n_exclude + 255) / 256)), dim3(256), 0, s.stream, d_ids, (uint32_t)n_exclude, d_mask);
        if ((st = check_launch("rank exclude")) != BN_OK) return st;
        mask = d_mask;
    }
    // the grid rule: the range's tiles in contiguous runs, at most one workgroup per compute unit
    uint32_t lo = id_lo, hi = id_hi, dpad = (uint32_t)s.dpad, tile_lo = id_lo / TILE, tile_hi = (id_hi + TILE - 1) / TILE;
    bn::WgSplit sp = bn::split_tiles(tile_hi - tile_lo, s.max_wg);
    int Mi = (int)M;
    for (size_t c0 = 0; c0 < C; c0 += s.out_lists) {
        const size_t nc = std::min(s.out_lists, C - c0);
        st = bn::run_scan_passes(
            s, nc, sp.n_wg, Mi, "rank scan",
            [&](size_t p0, int np) {
                const float *W = hv.d_W + (c0 + p0) * hv.dpad, *b = hv.d_b + c0 + p0;
                void *scan_args[] = {(void *)&s.slab, (void *)&mask, &lo, &hi, &dpad, (void *)&W, (void *)&b, &np, &Mi, &tile_lo, &tile_hi, &sp.tiles_per_wg,
                                     &s.d_cand, &s.d_cand_len};
                (void)hipLaunchKernel(scan_of(mode, (np + 15) / 16), dim3(sp.n_wg), dim3(256), scan_args, SCAN_LDS, s.stream);  // checked by the caller
            },
            mode == BN_RANK_UNCERTAIN ? enqueue_abs_merge : bn::index_enqueue_merge);
        if (st != BN_OK) return st;
        bn::scatter_results(s, c0, nc, M, m_stride, id_out, logit_out, count_out);
    }
    return BN_OK;
}
