// Classifier heads behind the C ABI (include/birdnet_hip.h, bn_head_*): an immutable linear head over a model's embedding,
// created from host weights or fitted on the device, applied to host rows or attached to a context's step.
//
// Layout: every row operand is [rows padded to 16 (64 in a fit)][dpad] with dpad = dim rounded up to KC and the padding zero;
// the head's weights are [cpad = classes rounded up to 16][dpad] + bias [cpad], padding zero.  No kernel has a k, row or class
// tail in its loads; only stores are guarded.
//
// Kernels:
//   * head_prep_kernel -- one wave per row: the raw row (stride dim) -> its padded operand row, normalised by the index's rule
//     (index.hip, index_normalise_kernel: the same chains, the same bits) under BN_HEAD_L2NORM, copied otherwise.  A row of up to
//     2048 elements is read once and held in registers between the sum of squares and the division.
//   * head_apply_kernel -- one wave per [16 rows x 16 classes] tile on the exact-f32 MFMA v_mfma_f32_16x16x4_f32, which is bit
//     for bit a k-ordered fmaf chain: ONE accumulator per output, its k order fixed by dpad alone, then the bias added.  The step,
//     bn_head_apply_host and the forward pass of a fit all run it.
//   * head_gather_kernel -- stored rows of an index -> the training slab (bn_head_fit_index).
//   * fit: head_trial_kernel (trial point = current point + a combination of the L-BFGS basis), head_apply_kernel (forward),
//     head_residual_kernel (residuals pw y (s - 1) + (1 - y) s, their per-block column sums for the bias gradient, loss partials),
//     head_grad_kernel (R^T X over fixed slices of n, one partial tile set per slice, exact-f32 MFMA), head_reduce_kernel (slices
//     summed in slice order + l2 * A, and the partial dot products L-BFGS and the stopping rule need), head_scalars_kernel (the
//     partials summed in block order), head_accept_kernel (the new (s, y) pair into its ring slot).  The host loop reads ONE block
//     of scalars per evaluation and runs the two-loop recursion on the basis' Gram matrix (vector-free L-BFGS), so no vector
//     ever crosses the bus.  Every reduction has a fixed order; there are no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "device_common.h"
#include "hip_gate.h"
#include "kernels.h"

namespace {

constexpr int KC = 128;            // k-step of the apply kernel; operand rows are padded to a multiple of it
constexpr size_t DIM_MAX = 8192, CLS_MAX = 4096;
constexpr size_t CHUNK = 1024;     // rows per round of bn_head_apply_host and of a fit's upload
constexpr int HM = 6;              // L-BFGS pairs kept
constexpr int NB = 2 * HM + 1;     // basis: s_0..s_5, y_0..y_5, g
constexpr int NCOL = 2 * HM + 3;   // dot-product columns: s_i, y_i, s_cand, y_cand, g_trial
constexpr int NQ = 3 * NCOL + 3;   // + |x_trial|^2, g_cur . s_cand, data loss
constexpr int RED_BLOCKS = 128;    // blocks of head_reduce_kernel (fixed: the order of its partial sums)
constexpr int PREP_REGS = 32;      // head_prep_kernel keeps a row of up to 64 * 32 = 2048 elements in registers
constexpr int RB = 64;             // rows per block of head_residual_kernel

using bn::floatx4;

// raw rows [n, dim] (stride src_stride) -> operand rows [npad, dpad]; rows >= n are zeros
__global__ __launch_bounds__(256) void head_prep_kernel(const float *__restrict__ src, size_t src_stride, uint32_t n, uint32_t npad, uint32_t dim,
                                                        int l2norm, float *__restrict__ dst, uint32_t dpad) {
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (r >= npad) return;
    float *y = dst + (size_t)r * dpad;
    if (r >= n) {
        for (uint32_t k = lane; k < dpad; k += 64) y[k] = 0.f;
        return;
    }
    const float *x = src + (size_t)r * src_stride;
    if (!l2norm) {
        for (uint32_t k = lane; k < dpad; k += 64) y[k] = k < dim ? x[k] : 0.f;
        return;
    }
    float ss = 0.f;
    bool fin = true;
    if (dim <= 64 * PREP_REGS) {
        // the row is read ONCE, every load in flight together, and kept in registers for the division; the chain below adds
        // the lane's elements in the same order as the loop of the long-row path (a missing element adds fmaf(0, 0, ss) = ss)
        float v[PREP_REGS];
#pragma unroll
        for (int j = 0; j < PREP_REGS; j++) {
            const uint32_t k = lane + 64 * j;
            v[j] = k < dim ? x[k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < PREP_REGS; j++) {
            fin = fin && isfinite(v[j]);
            ss = fmaf(v[j], v[j], ss);
        }
        for (int off = 32; off; off >>= 1) ss += __shfl_xor(ss, off);
        const bool ok = __ballot(!fin) == 0 && ss > 0.f && isfinite(ss);
        const float nrm = __fsqrt_rn(ss);
#pragma unroll
        for (int j = 0; j < PREP_REGS; j++) {
            const uint32_t k = lane + 64 * j;
            if (k < dpad) y[k] = (ok && k < dim) ? v[j] / nrm : 0.f;
        }
        return;
    }
    for (uint32_t k = lane; k < dim; k += 64) {
        const float v = x[k];
        fin = fin && isfinite(v);
        ss = fmaf(v, v, ss);
    }
    for (int off = 32; off; off >>= 1) ss += __shfl_xor(ss, off);
    const bool ok = __ballot(!fin) == 0 && ss > 0.f && isfinite(ss);
    const float nrm = __fsqrt_rn(ss);
    for (uint32_t k = lane; k < dpad; k += 64) y[k] = (ok && k < dim) ? x[k] / nrm : 0.f;
}

// stored rows ids[i] of an index slab (row stride dpad) -> slab rows [npad, dpad]; rows >= n are zeros
__global__ __launch_bounds__(256) void head_gather_kernel(const float *__restrict__ slab, const uint32_t *__restrict__ ids, uint32_t n, uint32_t dpad,
                                                          float *__restrict__ dst) {
    const uint32_t r = blockIdx.x;
    float *y = dst + (size_t)r * dpad;
    if (r >= n) {
        for (uint32_t k = threadIdx.x; k < dpad; k += 256) y[k] = 0.f;
        return;
    }
    const float *x = slab + (size_t)ids[r] * dpad;
    for (uint32_t k = threadIdx.x; k < dpad; k += 256) y[k] = x[k];
}

// Z[r][c] = chain_k(X[r][k] * W[c][k]) + b[c].  Wave w of block (bx, by) owns row tile bx and class tile 4 * by + w.
// Lane l: A operand = row 16 bx + (l & 15), B operand = class 16 ct + (l & 15), both at k = 16 s + 4 (l >> 4) + t of each KC chunk
// (t = component of the float4).  D: row 16 bx + 4 (l >> 4) + reg, class 16 ct + (l & 15).
__global__ __launch_bounds__(256) void head_apply_kernel(const float *__restrict__ X, const float *__restrict__ W, const float *__restrict__ bias,
                                                         uint32_t n, uint32_t C, uint32_t dpad, float *__restrict__ Z) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const uint32_t ct = blockIdx.y * 4 + w;
    if (ct * 16 >= C) return;  // wave-uniform; the weights hold ceil(C / 16) class tiles
    const float *xp = X + (size_t)(blockIdx.x * 16 + r16) * dpad + 4 * h;
    const float *wp = W + (size_t)(ct * 16 + r16) * dpad + 4 * h;
    float4 a[8], b[8];
#pragma unroll
    for (int s = 0; s < 8; s++) {
        a[s] = *reinterpret_cast<const float4 *>(xp + 16 * s);
        b[s] = *reinterpret_cast<const float4 *>(wp + 16 * s);
    }
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    const uint32_t nkc = dpad / KC;
    for (uint32_t u = 0; u < nkc; u++) {
        float4 an[8], bn_[8];
        if (u + 1 < nkc) {
#pragma unroll
            for (int s = 0; s < 8; s++) {
                an[s] = *reinterpret_cast<const float4 *>(xp + (size_t)(u + 1) * KC + 16 * s);
                bn_[s] = *reinterpret_cast<const float4 *>(wp + (size_t)(u + 1) * KC + 16 * s);
            }
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, b[s].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, b[s].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, b[s].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, b[s].w, acc, 0, 0, 0);
        }
        if (u + 1 < nkc) {
#pragma unroll
            for (int s = 0; s < 8; s++) {
                a[s] = an[s];
                b[s] = bn_[s];
            }
        }
    }
    const uint32_t cls = ct * 16 + r16;
    const float bv = bias[cls];  // cls < cpad
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t row = blockIdx.x * 16 + 4 * h + r;
        if (row < n && cls < C) Z[(size_t)row * C + cls] = acc[r] + bv;
    }
}

__device__ inline double softplus(double u) { return fmax(u, 0.0) + log1p(exp(-fabs(u))); }

// Block b: rows [RB b, RB b + RB).  R[row][c] = (pw_c y (s - 1) + (1 - y) s) / n (0 past n or C), Rb[b][c] = their sum over the
// block's rows in row order, lossp[b] = the block's share of the data loss (threads summed by a fixed tree).
__global__ __launch_bounds__(256) void head_residual_kernel(const float *__restrict__ Z, const uint8_t *__restrict__ Y, const float *__restrict__ pw,
                                                            uint32_t n, uint32_t C, uint32_t cpad, double inv_n, float *__restrict__ R,
                                                            float *__restrict__ Rb, double *__restrict__ lossp) {
    __shared__ double sh[256];
    const uint32_t r0 = blockIdx.x * RB;
    double loss = 0.0;
    for (uint32_t c = threadIdx.x; c < cpad; c += 256) {
        const double p = c < C ? (double)pw[c] : 0.0;
        float rb = 0.f;
        for (uint32_t i = 0; i < RB; i++) {
            const uint32_t row = r0 + i;
            float r = 0.f;
            if (row < n && c < C) {
                const double z = (double)Z[(size_t)row * C + c];
                const double s = 1.0 / (1.0 + exp(-z));
                if (Y[(size_t)row * C + c]) {
                    loss += p * softplus(-z);
                    r = (float)(p * (s - 1.0) * inv_n);
                } else {
                    loss += softplus(z);
                    r = (float)(s * inv_n);
                }
            }
            R[(size_t)row * cpad + c] = r;  // R has RB * gridDim.x rows
            rb += r;
        }
        Rb[(size_t)blockIdx.x * cpad + c] = rb;
    }
    sh[threadIdx.x] = loss;
    __syncthreads();
    for (int off = 128; off; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) lossp[blockIdx.x] = sh[0] * inv_n;
}

// Gp[slice][c][k] = sum over the slice's rows i, in row order, of R[i][c] * X[i][k].  Wave w of block (bx, by, bz): class tile
// by, columns [64 (4 bx + w), + 64) as four 16-column tiles, slice bz = rows [bz * slice_rows, min(+ slice_rows, npad)).
// Lane l: A = R[i0 + (l >> 4)][16 by + (l & 15)], B = X[i0 + (l >> 4)][col + (l & 15)]; D: class 16 by + 4 (l >> 4) + reg, col (l & 15).
__global__ __launch_bounds__(256) void head_grad_kernel(const float *__restrict__ R, const float *__restrict__ X, uint32_t npad, uint32_t cpad,
                                                        uint32_t dpad, uint32_t slice_rows, float *__restrict__ Gp) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    const uint32_t col0 = (blockIdx.x * 4 + w) * 64;
    if (col0 >= dpad) return;  // wave-uniform; dpad % 64 == 0
    const uint32_t i0 = blockIdx.z * slice_rows, i1 = min(npad, i0 + slice_rows);  // both multiples of 4
    floatx4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = floatx4{0.f, 0.f, 0.f, 0.f};
    const float *rp = R + (size_t)h * cpad + blockIdx.y * 16 + r16;
    const float *xp = X + (size_t)h * dpad + col0 + r16;
    for (uint32_t i = i0; i < i1; i += 4) {
        const float a = rp[(size_t)i * cpad];
        const float *xr = xp + (size_t)i * dpad;
#pragma unroll
        for (int j = 0; j < 4; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, xr[16 * j], acc[j], 0, 0, 0);
    }
    float *gp = Gp + ((size_t)blockIdx.z * cpad + blockIdx.y * 16 + 4 * h) * dpad + col0 + r16;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) gp[(size_t)r * dpad + 16 * j] = acc[j][r];
}

struct TrialCoef {
    float c[NB];
};

// x_trial = x_cur + sum_j coef_j * basis_j (basis: the s ring, the y ring, g_cur), one fmaf chain in basis order
__global__ __launch_bounds__(256) void head_trial_kernel(const float *__restrict__ xc, const float *__restrict__ hist, const float *__restrict__ gc,
                                                         TrialCoef coef, size_t pv, float *__restrict__ xt) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pv) return;
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 2 * HM; j++) v = fmaf(coef.c[j], hist[(size_t)j * pv + e], v);
    v = fmaf(coef.c[2 * HM], gc[e], v);
    xt[e] = xc[e] + v;
}

// g_trial = slices summed in slice order (weights) or residual blocks summed in block order (biases) + l2 * x_trial, and this
// block's partial sums of the NQ - 1 dot products (thread sums in element order, lanes by a fixed butterfly, waves in order)
__global__ __launch_bounds__(256) void head_reduce_kernel(const float *__restrict__ Gp, uint32_t n_slices, const float *__restrict__ Rb,
                                                          uint32_t n_rblocks, uint32_t cpad, size_t wv, size_t pv, float l2,
                                                          const float *__restrict__ xt, const float *__restrict__ xc, const float *__restrict__ gc,
                                                          const float *__restrict__ hist, float *__restrict__ gt, double *__restrict__ part) {
    __shared__ double sh[4][NQ];
    double q[NQ - 1];
#pragma unroll
    for (int j = 0; j < NQ - 1; j++) q[j] = 0.0;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < pv; e += (size_t)RED_BLOCKS * 256) {
        float g = 0.f;
        if (e < wv) {
            for (uint32_t s = 0; s < n_slices; s++) g += Gp[(size_t)s * wv + e];
        } else {
            for (uint32_t b = 0; b < n_rblocks; b++) g += Rb[(size_t)b * cpad + (e - wv)];
        }
        const float x = xt[e];
        g = fmaf(l2, x, g);
        gt[e] = g;
        const float gcur = gc[e];
        double col[NCOL];
#pragma unroll
        for (int j = 0; j < 2 * HM; j++) col[j] = (double)hist[(size_t)j * pv + e];
        col[2 * HM] = (double)(x - xc[e]);
        col[2 * HM + 1] = (double)(g - gcur);
        col[2 * HM + 2] = (double)g;
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int j = 0; j < NCOL; j++) q[a * NCOL + j] += col[2 * HM + a] * col[j];
        q[3 * NCOL] += (double)x * (double)x;
        q[3 * NCOL + 1] += (double)gcur * col[2 * HM];
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < NQ - 1; j++) {
        double v = q[j];
        for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) sh[w][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < NQ - 1) part[(size_t)blockIdx.x * NQ + threadIdx.x] = ((sh[0][threadIdx.x] + sh[1][threadIdx.x]) + sh[2][threadIdx.x]) + sh[3][threadIdx.x];
}

// out[j] = the blocks' partials in block order; out[NQ - 1] = the residual blocks' loss shares in block order
__global__ __launch_bounds__(64) void head_scalars_kernel(const double *__restrict__ part, const double *__restrict__ lossp, uint32_t n_rblocks,
                                                          double *__restrict__ out) {
    const int j = threadIdx.x;
    if (j < NQ - 1) {
        double v = 0.0;
        for (int b = 0; b < RED_BLOCKS; b++) v += part[(size_t)b * NQ + j];
        out[j] = v;
    } else if (j == NQ - 1) {
        double v = 0.0;
        for (uint32_t b = 0; b < n_rblocks; b++) v += lossp[b];
        out[j] = v;
    }
}

// the accepted step's pair into ring slot `slot`: s = x_trial - x_cur, y = g_trial - g_cur (the values head_reduce_kernel used)
__global__ __launch_bounds__(256) void head_accept_kernel(const float *__restrict__ xt, const float *__restrict__ xc, const float *__restrict__ gt,
                                                          const float *__restrict__ gc, size_t pv, int slot, float *__restrict__ hist) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pv) return;
    hist[(size_t)slot * pv + e] = xt[e] - xc[e];
    hist[(size_t)(HM + slot) * pv + e] = gt[e] - gc[e];
}

}  // namespace

struct bn_head {
    std::atomic<int> refs{1};  // the caller's handle + one per context that attached it
    int device = 0;
    size_t dim = 0, dpad = 0, classes = 0, cpad = 0;
    uint32_t flags = 0;
    // bn_head_apply_host's own stream and staging, allocated on first use
    bn::Stream stream;  // before the buffers: it goes last (device_mem.h)
    bn::DeviceBuf<float> d_raw, d_x, d_z;  // [CHUNK, dim], [CHUNK, dpad], [CHUNK, classes]
    bn::DeviceBuf<float> d_W;  // [cpad, dpad]
    bn::DeviceBuf<float> d_b;  // [cpad]
    ~bn_head() {
        (void)bn::use_device(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

struct bn::HeadAttach {
    bn_head *head = nullptr;
    size_t max_batch = 0, k = 0;
    int32_t has_min = 0;
    float min_conf = 0.f;
    bn::DeviceBuf<float> d_x;   // [max_batch padded to 16, dpad]
    bn::DeviceBuf<float> d_z;   // [max_batch, classes]
    bn::TopkRows rows;          // the last step's top-K rows: device block and pinned mirror
    bn::DeviceBuf<uint32_t> d_flags;
    bn::PinnedBuf<float> h_z;  // pinned mirror of d_z
    ~HeadAttach();             // drops the reference
};

namespace {

using bn::set_last_error;

using bn::check_launch;

size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

void head_unref(bn_head *h) {
    if (h && h->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete h;
}

bn_status check_shape(size_t dim, size_t n_classes) {
    if (dim < 1 || dim > DIM_MAX) return set_last_error(BN_ERR_INVALID_ARG, "dim must be in 1..8192, got " + std::to_string(dim));
    if (n_classes < 1 || n_classes > CLS_MAX) return set_last_error(BN_ERR_INVALID_ARG, "n_classes must be in 1..4096, got " + std::to_string(n_classes));
    return BN_OK;
}

// a head on `device` whose weights and bias the caller fills WHOLE, padding included (bn_head_create from the host, a fit from
// its solution)
bn_status new_head(int32_t device, size_t dim, size_t n_classes, uint32_t flags, std::unique_ptr<bn_head> &h) {
    BN_HIP_TRY(bn::use_device(device));
    if (!bn::prepare_device(device)) return set_last_error(BN_ERR_BACKEND, "device refused the kernels' dynamic-LDS opt-in");
    h.reset(new bn_head);
    h->device = device;
    h->dim = dim;
    h->dpad = round_up(dim, KC);
    h->classes = n_classes;
    h->cpad = round_up(n_classes, 16);
    h->flags = flags;
    BN_HIP_TRY(h->d_W.alloc(h->cpad * h->dpad * sizeof(float)));
    BN_HIP_TRY(h->d_b.alloc(h->cpad * sizeof(float)));
    return BN_OK;
}

// raw rows at d_src (stride dim) -> operand rows at d_x -> logits at d_z, on `stream`
bn_status enqueue_apply(const bn_head *h, hipStream_t stream, const float *d_src, size_t n, float *d_x, float *d_z) {
    const uint32_t npad = (uint32_t)round_up(n, 16);
    hipLaunchKernelGGL(head_prep_kernel, dim3((npad + 3) / 4), dim3(256), 0, stream, d_src, h->dim, (uint32_t)n, npad, (uint32_t)h->dim,
                       (h->flags & BN_HEAD_L2NORM) ? 1 : 0, d_x, (uint32_t)h->dpad);
    bn_status st = check_launch("head prep");
    if (st != BN_OK) return st;
    hipLaunchKernelGGL(head_apply_kernel, dim3(npad / 16, (unsigned)((h->cpad / 16 + 3) / 4)), dim3(256), 0, stream, d_x, h->d_W, h->d_b, (uint32_t)n,
                       (uint32_t)h->classes, (uint32_t)h->dpad, d_z);
    return check_launch("head apply");
}

struct FitOpts {
    float l2 = 1e-3f, tol = 1e-6f;
    uint32_t max_iters = 2000, flags = 0;
    const float *pos_weight = nullptr;
};

bn_status read_opts(const bn_head_fit_opts *opts, size_t opts_size, size_t n_classes, FitOpts *o, std::vector<float> *pw) {
    bn_head_fit_opts in{};
    if (opts) memcpy(&in, opts, std::min(opts_size, sizeof(in)));  // a shorter (older) struct leaves the rest at its defaults
    auto pos = [](float v) { return std::isfinite(v) && v > 0.f; };
    if (in.l2 != 0.f) {
        if (!pos(in.l2)) return set_last_error(BN_ERR_INVALID_ARG, "l2 must be positive and finite");
        o->l2 = in.l2;
    }
    if (in.tol != 0.f) {
        if (!pos(in.tol)) return set_last_error(BN_ERR_INVALID_ARG, "tol must be positive and finite");
        o->tol = in.tol;
    }
    if (in.max_iters) o->max_iters = in.max_iters;
    if (in.flags & ~BN_HEAD_L2NORM) return set_last_error(BN_ERR_INVALID_ARG, "unknown flag");
    o->flags = in.flags;
    pw->assign(n_classes, 1.f);
    if (in.pos_weight) {
        for (size_t c = 0; c < n_classes; c++) {
            if (!pos(in.pos_weight[c])) return set_last_error(BN_ERR_INVALID_ARG, "pos_weight[" + std::to_string(c) + "] must be positive and finite");
            (*pw)[c] = in.pos_weight[c];
        }
    }
    return BN_OK;
}

bn_status check_labels(const uint8_t *labels, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (labels[i] > 1) return set_last_error(BN_ERR_INVALID_ARG, "labels must be 0 or 1 (element " + std::to_string(i) + " is " + std::to_string(labels[i]) + ")");
    return BN_OK;
}

// The solver.  d_X: the training slab [npad (multiple of RB), dpad], padding zero.  L-BFGS over all classes at once with Armijo
// backtracking (the objective is strongly convex: every accepted pair has s.y > 0, no curvature condition is needed).  One
// "iteration" is one evaluation of (L, grad L) at a trial point; the scalars of an evaluation cross the bus once.
bn_status solve(bn::Scratch &bufs, bn_head *h, const float *d_X, size_t n, size_t npad, const uint8_t *labels, const std::vector<float> &pw, const FitOpts &o,
                bn_head_fit_report *rep) {
    const size_t C = h->classes, cpad = h->cpad, dpad = h->dpad;
    const size_t wv = cpad * dpad, pv = wv + cpad;
    hipStream_t s = bufs.stream;
    // slices of the gradient's reduction over n: as many as the partial buffer affords (at most 64), each a multiple of 16 rows
    const size_t max_slices = std::max<size_t>(1, std::min<size_t>(64, ((size_t)1 << 26) / wv));
    const size_t slice_rows = round_up((npad + max_slices - 1) / max_slices, 16);
    const uint32_t n_slices = (uint32_t)((npad + slice_rows - 1) / slice_rows);
    const uint32_t n_rblocks = (uint32_t)(npad / RB);

    uint8_t *d_Y = nullptr;
    float *d_pw = nullptr, *d_Z = nullptr, *d_R = nullptr, *d_Rb = nullptr, *d_Gp = nullptr, *d_hist = nullptr, *d_x[2] = {nullptr, nullptr},
          *d_g[2] = {nullptr, nullptr};
    double *d_lossp = nullptr, *d_part = nullptr, *d_out = nullptr;
    BN_HIP_TRY(bufs.alloc(&d_Y, n * C, false));
    BN_HIP_TRY(bn::gated::Memcpy(d_Y, labels, n * C, hipMemcpyHostToDevice));
    BN_HIP_TRY(bufs.alloc(&d_pw, C * sizeof(float), false));
    BN_HIP_TRY(bn::gated::Memcpy(d_pw, pw.data(), C * sizeof(float), hipMemcpyHostToDevice));
    BN_HIP_TRY(bufs.alloc(&d_Z, n * C * sizeof(float), false));
    BN_HIP_TRY(bufs.alloc(&d_R, npad * cpad * sizeof(float), false));
    BN_HIP_TRY(bufs.alloc(&d_Rb, (size_t)n_rblocks * cpad * sizeof(float), false));
    BN_HIP_TRY(bufs.alloc(&d_Gp, (size_t)n_slices * wv * sizeof(float), false));
    BN_HIP_TRY(bufs.alloc(&d_hist, (size_t)2 * HM * pv * sizeof(float), true));
    for (int i = 0; i < 2; i++) {
        BN_HIP_TRY(bufs.alloc(&d_x[i], pv * sizeof(float), true));
        BN_HIP_TRY(bufs.alloc(&d_g[i], pv * sizeof(float), true));
    }
    BN_HIP_TRY(bufs.alloc(&d_lossp, n_rblocks * sizeof(double), false));
    BN_HIP_TRY(bufs.alloc(&d_part, (size_t)RED_BLOCKS * NQ * sizeof(double), true));
    BN_HIP_TRY(bufs.alloc(&d_out, NQ * sizeof(double), false));
    BN_HIP_TRY(bufs.pinned.alloc(NQ * sizeof(double)));
    double *h_out = static_cast<double *>(bufs.pinned.get());

    int cur = 0;  // d_x[cur], d_g[cur]: the current point and its gradient; [1 - cur]: the trial
    // (L, grad L) at d_x[1 - cur] and every dot product of the candidate pair; results in h_out
    auto evaluate = [&]() -> bn_status {
        float *xt = d_x[1 - cur], *gt = d_g[1 - cur];
        hipLaunchKernelGGL(head_apply_kernel, dim3((unsigned)(npad / 16), (unsigned)((cpad / 16 + 3) / 4)), dim3(256), 0, s, d_X, xt, xt + wv, (uint32_t)n,
                           (uint32_t)C, (uint32_t)dpad, d_Z);
        hipLaunchKernelGGL(head_residual_kernel, dim3(n_rblocks), dim3(256), 0, s, d_Z, d_Y, d_pw, (uint32_t)n, (uint32_t)C, (uint32_t)cpad, 1.0 / (double)n,
                           d_R, d_Rb, d_lossp);
        hipLaunchKernelGGL(head_grad_kernel, dim3((unsigned)((dpad / 64 + 3) / 4), (unsigned)(cpad / 16), n_slices), dim3(256), 0, s, d_R, d_X, (uint32_t)npad,
                           (uint32_t)cpad, (uint32_t)dpad, (uint32_t)slice_rows, d_Gp);
        hipLaunchKernelGGL(head_reduce_kernel, dim3(RED_BLOCKS), dim3(256), 0, s, d_Gp, n_slices, d_Rb, n_rblocks, (uint32_t)cpad, wv, pv, o.l2, xt, d_x[cur],
                           d_g[cur], d_hist, gt, d_part);
        hipLaunchKernelGGL(head_scalars_kernel, dim3(1), dim3(64), 0, s, d_part, d_lossp, n_rblocks, d_out);
        bn_status st = check_launch("head fit");
        if (st != BN_OK) return st;
        BN_HIP_TRY(hipMemcpyAsync(h_out, d_out, NQ * sizeof(double), hipMemcpyDeviceToHost, s));
        BN_HIP_TRY(hipStreamSynchronize(s));
        return BN_OK;
    };
    auto dot = [&](int a, int col) { return h_out[a * NCOL + col]; };  // a: 0 s_cand, 1 y_cand, 2 g_trial
    constexpr int CS = 2 * HM, CY = 2 * HM + 1, CG = 2 * HM + 2;
    auto loss_of = [&]() { return h_out[NQ - 1] + 0.5 * (double)o.l2 * h_out[3 * NCOL]; };

    double M[NB][NB] = {};  // Gram matrix of the basis (s ring, y ring, g_cur)
    int count = 0, next = 0;  // pairs held; the slot the next pair goes to
    // the trial becomes the current point; with_pair: its (s, y) joins the history
    auto accept = [&](bool with_pair) -> bn_status {
        const int G = 2 * HM;
        if (with_pair) {
            const int p = next;
            hipLaunchKernelGGL(head_accept_kernel, dim3((unsigned)((pv + 255) / 256)), dim3(256), 0, s, d_x[1 - cur], d_x[cur], d_g[1 - cur], d_g[cur], pv, p,
                               d_hist);
            bn_status st = check_launch("head accept");
            if (st != BN_OK) return st;
            for (int i = 0; i < HM; i++) {
                M[p][i] = M[i][p] = dot(0, i);
                M[p][HM + i] = M[HM + i][p] = dot(0, HM + i);
                M[HM + p][i] = M[i][HM + p] = dot(1, i);
                M[HM + p][HM + i] = M[HM + i][HM + p] = dot(1, HM + i);
            }
            M[p][p] = dot(0, CS);
            M[p][HM + p] = M[HM + p][p] = dot(0, CY);
            M[HM + p][HM + p] = dot(1, CY);
            next = (next + 1) % HM;
            count = std::min(count + 1, HM);
            for (int j = 0; j < 2 * HM; j++) M[G][j] = M[j][G] = dot(2, j);
            M[G][p] = M[p][G] = dot(2, CS);
            M[G][HM + p] = M[HM + p][G] = dot(2, CY);
        } else {
            for (int j = 0; j < 2 * HM; j++) M[G][j] = M[j][G] = dot(2, j);
        }
        M[G][G] = dot(2, CG);
        cur = 1 - cur;
        return BN_OK;
    };
    // -H g as coefficients over the basis (two-loop recursion on the Gram matrix); returns g . d
    auto direction = [&](double *delta) {
        const int G = 2 * HM;
        for (int j = 0; j < NB; j++) delta[j] = 0.0;
        delta[G] = 1.0;
        if (count == 0) {
            delta[G] = -1.0;
            return -M[G][G];
        }
        double alpha[HM];
        auto col_dot = [&](int col) {
            double v = 0.0;
            for (int j = 0; j < NB; j++) v += delta[j] * M[j][col];
            return v;
        };
        for (int t = 0; t < count; t++) {  // newest first
            const int i = ((next - 1 - t) % HM + HM) % HM;
            alpha[i] = col_dot(i) / M[i][HM + i];
            delta[HM + i] -= alpha[i];
        }
        const int newest = ((next - 1) % HM + HM) % HM;
        const double gamma = M[newest][HM + newest] / M[HM + newest][HM + newest];
        for (int j = 0; j < NB; j++) delta[j] *= gamma;
        for (int t = count - 1; t >= 0; t--) {  // oldest first
            const int i = ((next - 1 - t) % HM + HM) % HM;
            const double beta = col_dot(HM + i) / M[i][HM + i];
            delta[i] += alpha[i] - beta;
        }
        double gd = 0.0;
        for (int j = 0; j < NB; j++) {
            delta[j] = -delta[j];
            gd += delta[j] * M[j][G];
        }
        return gd;
    };

    // the starting point: A = 0
    bn_status st = evaluate();
    if (st != BN_OK) return st;
    uint32_t iters = 1;
    double f = loss_of(), gg = dot(2, CG);
    if ((st = accept(false)) != BN_OK) return st;
    double cert = gg / (2.0 * (double)o.l2);
    bool converged = cert <= (double)o.tol;
    double delta[NB];
    while (!converged && iters < o.max_iters) {
        double gd = direction(delta);
        if (!(gd < 0.0)) {  // rounding spoiled the history: steepest descent
            count = 0;
            gd = direction(delta);
        }
        double t = count ? 1.0 : std::min(1.0, 1.0 / std::sqrt(gg));
        int tries = 0;
        bool moved = false;
        while (iters < o.max_iters) {
            TrialCoef coef;
            for (int j = 0; j < NB; j++) coef.c[j] = (float)(t * delta[j]);
            hipLaunchKernelGGL(head_trial_kernel, dim3((unsigned)((pv + 255) / 256)), dim3(256), 0, s, d_x[cur], d_hist, d_g[cur], coef, pv, d_x[1 - cur]);
            if ((st = evaluate()) != BN_OK) return st;
            iters++;
            const double ft = loss_of(), ggt = dot(2, CG), gs = h_out[3 * NCOL + 1];  // gs = g_cur . s_cand = t * (g . d) as stepped
            const bool armijo = ft <= f + 1e-4 * gs;
            const bool flat = std::fabs(ft - f) <= 1e-9 * std::fabs(f) && ggt < gg;  // below the loss' own resolution: the gradient decides
            if (std::isfinite(ft) && (armijo || flat)) {
                const double sy = dot(0, CY);
                if ((st = accept(sy > 1e-30 && sy > 1e-12 * dot(1, CY))) != BN_OK) return st;
                f = ft;
                gg = ggt;
                moved = true;
                break;
            }
            if (++tries >= 30) break;
            t *= 0.5;
        }
        cert = gg / (2.0 * (double)o.l2);
        converged = cert <= (double)o.tol;
        if (!moved) {
            if (count == 0) break;  // no descent along the gradient itself: the f32 floor is reached
            count = 0;
        }
    }
    // the current point becomes the head (the same padded layout)
    BN_HIP_TRY(hipMemcpyAsync(h->d_W, d_x[cur], wv * sizeof(float), hipMemcpyDeviceToDevice, s));
    BN_HIP_TRY(hipMemcpyAsync(h->d_b, d_x[cur] + wv, cpad * sizeof(float), hipMemcpyDeviceToDevice, s));
    BN_HIP_TRY(hipStreamSynchronize(s));
    rep->iters = iters;
    rep->converged = converged ? 1 : 0;
    rep->loss = f;
    rep->certificate = cert;
    return BN_OK;
}

void write_report(const bn_head_fit_report &rep, bn_head_fit_report *out, size_t size) {
    if (out) memcpy(out, &rep, std::min(size, sizeof(rep)));
}

}  // namespace

bn::HeadView bn::head_view(const bn_head *h) { return {h->device, h->dim, h->dpad, h->classes, h->cpad, h->flags, h->d_W, h->d_b}; }

bn_status bn::head_attach(bn_head *h, int device, bool has_embedding, size_t embedding_dim, size_t max_batch, size_t top_k, int32_t has_min, float min_conf,
                          HeadAttach **out) {
    if (!h || !out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (!has_embedding) return set_last_error(BN_ERR_INVALID_ARG, "the context's model has no embedding output");
    if (embedding_dim != h->dim)
        return set_last_error(BN_ERR_INVALID_ARG, "the head's dim " + std::to_string(h->dim) + " differs from the model's embedding_dim " + std::to_string(embedding_dim));
    if (device != h->device) return set_last_error(BN_ERR_INVALID_ARG, "the context lives on device " + std::to_string(device) + ", the head on " + std::to_string(h->device));
    size_t k = 0;
    bn_status st = bn::check_top_k(h->classes, top_k, &k);
    if (st != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(device));
    auto a = std::make_unique<HeadAttach>();
    a->max_batch = max_batch;
    a->k = k;
    a->has_min = has_min;
    a->min_conf = min_conf;
    BN_HIP_TRY(a->d_x.alloc(round_up(max_batch, 16) * h->dpad * sizeof(float)));
    BN_HIP_TRY(a->d_z.alloc(max_batch * h->classes * sizeof(float)));
    if ((st = a->rows.reserve(max_batch, k, nullptr, true, true)) != BN_OK) return st;
    BN_HIP_TRY(a->d_flags.alloc(max_batch * sizeof(uint32_t)));
    BN_HIP_TRY(a->h_z.alloc(max_batch * h->classes * sizeof(float)));
    h->refs.fetch_add(1, std::memory_order_relaxed);
    a->head = h;
    *out = a.release();
    return BN_OK;
}

bn::HeadAttach::~HeadAttach() { head_unref(head); }
void bn::head_detach(HeadAttach *a) { delete a; }

bn_status bn::head_step(HeadAttach *a, hipStream_t stream, const float *d_emb, size_t batch) {
    const bn_head *h = a->head;
    if (batch > a->max_batch) return set_last_error(BN_ERR_INVALID_ARG, "batch exceeds the context's max_batch");
    bn_status st = enqueue_apply(h, stream, d_emb, batch, a->d_x, a->d_z);
    if (st != BN_OK) return st;
    const size_t k = a->k, C = h->classes;
    st = bn::enqueue_topk_rows(stream, a->d_z, batch, C, k, a->has_min, a->min_conf, bn::TopkRows::view(a->rows.d, batch, k), a->d_flags);
    if (st != BN_OK) return st;
    const bn::OutRegion regs[2] = {{a->h_z, a->d_z, batch * C * sizeof(float)}, {a->rows.h, a->rows.d, bn::TopkRows::bytes(batch, k)}};
    if ((st = bn::results_to_host(stream, regs, 2)) != BN_OK) return st;
    a->rows.mark(batch, k);
    return BN_OK;
}

bn_status bn::head_step_results(const HeadAttach *a, const float **logits, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride,
                                size_t *n_classes) {
    static const char *none = "no step has run on this context since a head was attached";
    if (!a) return set_last_error(BN_ERR_INVALID_ARG, none);
    bn_status st = a->rows.results(none, idx, conf, count, k_stride);
    if (st != BN_OK) return st;
    if (logits) *logits = a->h_z;
    if (n_classes) *n_classes = a->head->classes;
    return BN_OK;
}

extern "C" {

bn_status bn_head_create(int32_t device, size_t dim, size_t n_classes, const float *W, const float *bias, uint32_t flags, bn_head **out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    bn_status st = check_shape(dim, n_classes);
    if (st != BN_OK) return st;
    if (!W) return set_last_error(BN_ERR_INVALID_ARG, "null weights");
    if (flags & ~BN_HEAD_L2NORM) return set_last_error(BN_ERR_INVALID_ARG, "unknown flag");
    if ((st = bn::require_device(device)) != BN_OK) return st;
    std::unique_ptr<bn_head> h;
    if ((st = new_head(device, dim, n_classes, flags, h)) != BN_OK) return st;
    std::vector<float> pad(h->cpad * h->dpad, 0.f);
    for (size_t c = 0; c < n_classes; c++) memcpy(pad.data() + c * h->dpad, W + c * dim, dim * sizeof(float));
    BN_HIP_TRY(bn::gated::Memcpy(h->d_W, pad.data(), pad.size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float> bpad(h->cpad, 0.f);
    if (bias) memcpy(bpad.data(), bias, n_classes * sizeof(float));
    BN_HIP_TRY(bn::gated::Memcpy(h->d_b, bpad.data(), bpad.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = h.release();
    return BN_OK;
}

void bn_head_free(bn_head *h) { head_unref(h); }

size_t bn_head_dim(const bn_head *h) { return h ? h->dim : 0; }
size_t bn_head_classes(const bn_head *h) { return h ? h->classes : 0; }
uint32_t bn_head_flags(const bn_head *h) { return h ? h->flags : 0; }

bn_status bn_head_read(const bn_head *h, float *W_out, float *bias_out) {
    if (!h) return set_last_error(BN_ERR_INVALID_ARG, "null head");
    BN_HIP_TRY(bn::use_device(h->device));
    if (W_out) {
        std::vector<float> pad(h->cpad * h->dpad);
        BN_HIP_TRY(bn::gated::Memcpy(pad.data(), h->d_W, pad.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < h->classes; c++) memcpy(W_out + c * h->dim, pad.data() + c * h->dpad, h->dim * sizeof(float));
    }
    if (bias_out) BN_HIP_TRY(bn::gated::Memcpy(bias_out, h->d_b, h->classes * sizeof(float), hipMemcpyDeviceToHost));
    return BN_OK;
}

bn_status bn_head_apply_host(const bn_head *hc, const float *rows, size_t n, float *logits_out) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!hc) return set_last_error(BN_ERR_INVALID_ARG, "null head");
    if (n && (!rows || !logits_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    bn_head *h = const_cast<bn_head *>(hc);  // the staging buffers are not part of the head's value
    BN_HIP_TRY(bn::use_device(h->device));
    // each piece on its own: a call that failed half way leaves the rest to the next one
    if (!h->stream) BN_HIP_TRY(h->stream.create(hipStreamNonBlocking));
    if (!h->d_raw) BN_HIP_TRY(h->d_raw.alloc(CHUNK * h->dim * sizeof(float)));
    if (!h->d_x) BN_HIP_TRY(h->d_x.alloc(CHUNK * h->dpad * sizeof(float)));
    if (!h->d_z) BN_HIP_TRY(h->d_z.alloc(CHUNK * h->classes * sizeof(float)));
    for (size_t r0 = 0; r0 < n; r0 += CHUNK) {
        const size_t k = std::min(CHUNK, n - r0);
        BN_HIP_TRY(bn::gated::Memcpy(h->d_raw, rows + r0 * h->dim, k * h->dim * sizeof(float), hipMemcpyHostToDevice));
        bn_status st = enqueue_apply(h, h->stream, h->d_raw, k, h->d_x, h->d_z);
        if (st != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(h->stream));
        BN_HIP_TRY(bn::gated::Memcpy(logits_out + r0 * h->classes, h->d_z, k * h->classes * sizeof(float), hipMemcpyDeviceToHost));
    }
    return BN_OK;
}

bn_status bn_head_fit(int32_t device, size_t dim, size_t n_classes, const float *rows, const uint8_t *labels, size_t n, const bn_head_fit_opts *opts,
                      size_t opts_size, bn_head **out, bn_head_fit_report *report, size_t report_size) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    bn_status st = check_shape(dim, n_classes);
    if (st != BN_OK) return st;
    if (n == 0) return set_last_error(BN_ERR_INVALID_ARG, "a fit needs at least one row");
    if (n > 0x7fffffffull / std::max(n_classes, (size_t)16)) return set_last_error(BN_ERR_INVALID_ARG, "n * n_classes must stay below 2^31");
    if (!rows || !labels) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    FitOpts o;
    std::vector<float> pw;
    if ((st = read_opts(opts, opts_size, n_classes, &o, &pw)) != BN_OK) return st;
    if ((st = check_labels(labels, n * n_classes)) != BN_OK) return st;
    if ((st = bn::require_device(device)) != BN_OK) return st;
    std::unique_ptr<bn_head> h;
    if ((st = new_head(device, dim, n_classes, o.flags, h)) != BN_OK) return st;
    bn::Scratch bufs;
    BN_HIP_TRY(bufs.create_stream(hipStreamNonBlocking));
    const size_t npad = round_up(n, RB);
    float *d_X = nullptr, *d_raw = nullptr;
    BN_HIP_TRY(bufs.alloc(&d_X, npad * h->dpad * sizeof(float), false));
    BN_HIP_TRY(bufs.alloc(&d_raw, CHUNK * dim * sizeof(float), false));
    for (size_t r0 = 0; r0 < npad; r0 += CHUNK) {  // the last round also zeroes the slab's padding rows
        const size_t rows_here = std::min(CHUNK, npad - r0), real = r0 < n ? std::min(CHUNK, n - r0) : 0;
        if (real) BN_HIP_TRY(bn::gated::Memcpy(d_raw, rows + r0 * dim, real * dim * sizeof(float), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(head_prep_kernel, dim3((unsigned)((rows_here + 3) / 4)), dim3(256), 0, bufs.stream, d_raw, dim, (uint32_t)real, (uint32_t)rows_here,
                           (uint32_t)dim, (o.flags & BN_HEAD_L2NORM) ? 1 : 0, d_X + r0 * h->dpad, (uint32_t)h->dpad);
        if ((st = check_launch("head prep")) != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(bufs.stream));
    }
    bn_head_fit_report rep{};
    if ((st = solve(bufs, h.get(), d_X, n, npad, labels, pw, o, &rep)) != BN_OK) return st;
    write_report(rep, report, report_size);
    *out = h.release();
    return BN_OK;
}

bn_status bn_head_fit_index(bn_index *x, const uint64_t *ids, const uint8_t *labels, size_t n, size_t n_classes, const bn_head_fit_opts *opts,
                            size_t opts_size, bn_head **out, bn_head_fit_report *report, size_t report_size) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!x) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    bn::IndexRows ir;
    bn_status st = bn::index_rows(x, &ir);
    if (st != BN_OK) return st;
    if ((st = check_shape(ir.dim, n_classes)) != BN_OK) return st;
    if (n == 0) return set_last_error(BN_ERR_INVALID_ARG, "a fit needs at least one row");
    if (n > 0x7fffffffull / std::max(n_classes, (size_t)16)) return set_last_error(BN_ERR_INVALID_ARG, "n * n_classes must stay below 2^31");
    if (!ids || !labels) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    FitOpts o;
    std::vector<float> pw;
    if ((st = read_opts(opts, opts_size, n_classes, &o, &pw)) != BN_OK) return st;
    o.flags = BN_HEAD_L2NORM;
    if ((st = check_labels(labels, n * n_classes)) != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(ir.device));
    std::vector<uint8_t> valid(ir.size);
    if (ir.size) BN_HIP_TRY(bn::gated::Memcpy(valid.data(), ir.valid, ir.size, hipMemcpyDeviceToHost));
    std::vector<uint32_t> id32(n);
    for (size_t i = 0; i < n; i++) {
        if (ids[i] >= ir.size) return set_last_error(BN_ERR_INVALID_ARG, "id " + std::to_string(ids[i]) + " is not in the index");
        if (!valid[ids[i]]) return set_last_error(BN_ERR_INVALID_ARG, "row " + std::to_string(ids[i]) + " of the index is stored as zeros (it had no direction)");
        id32[i] = (uint32_t)ids[i];
    }
    std::unique_ptr<bn_head> h;
    if ((st = new_head(ir.device, ir.dim, n_classes, o.flags, h)) != BN_OK) return st;
    bn::Scratch bufs;
    BN_HIP_TRY(bufs.create_stream(hipStreamNonBlocking));
    const size_t npad = round_up(n, RB);
    float *d_X = nullptr;
    uint32_t *d_ids = nullptr;
    BN_HIP_TRY(bufs.alloc(&d_X, npad * h->dpad * sizeof(float), false));
    BN_HIP_TRY(bufs.alloc(&d_ids, n * sizeof(uint32_t), false));
    BN_HIP_TRY(bn::gated::Memcpy(d_ids, id32.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(head_gather_kernel, dim3((unsigned)npad), dim3(256), 0, bufs.stream, ir.slab, d_ids, (uint32_t)n, (uint32_t)h->dpad, d_X);
    if ((st = check_launch("head gather")) != BN_OK) return st;
    bn_head_fit_report rep{};
    if ((st = solve(bufs, h.get(), d_X, n, npad, labels, pw, o, &rep)) != BN_OK) return st;
    write_report(rep, report, report_size);
    *out = h.release();
    return BN_OK;
}

}  // extern "C"
