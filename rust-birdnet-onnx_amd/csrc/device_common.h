// Device helpers shared by the kernel translation units (kernels.hip, stft.hip): the logistic / exp / log / pow
// forms of the network path and the one-dispatch-per-stage unary / binary stage functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace bn {
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// operands of __builtin_amdgcn_global_load_lds: the global source and the LDS destination in their address spaces
#define BN_GLB_PTR(p) ((const __attribute__((address_space(1))) void *)(p))
#define BN_LDS_PTR(p) ((__attribute__((address_space(3))) void *)(p))

// Logistic function inside the network (SE gates, SiLU): hardware exp2 and reciprocal
// (v_exp_f32 / v_rcp_f32, ~1 ulp each; the argument scaling adds |x| * 2^-24 relative), 6
// instructions instead of ~30 for the IEEE expf + division.  Saturates correctly: x -> -inf gives
// rcp(inf) = 0, x -> +inf gives rcp(1) = 1.  The CONFIDENCE sigmoid of the post-processing
// (topk.hip) does not use this: it is bit-exact against the reference's f32 sigmoid.
__device__ __forceinline__ float net_sigmoid(float x) {
    return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896340736f));
}
// exp / log / pow of the front end's dynamic-range compression (power spectrum -> x^p, log-mel):
// hardware exp2 / log2 (v_exp_f32 / v_log_f32, ~1 ulp each).  pow(x, p) = exp2(p * log2 x) for
// x > 0 has a relative error of about |p * log2 x| * 2^-23 (<= 1e-5 over the 1e-30..1e30 range a
// spectrogram can span), against ~150 instructions for the correctly rounded powf -- the two Pow
// chains of the v2.4 front end were VALU-bound on it.  Non-positive bases keep the libm path
// (signs, zeros, NaN rules).
__device__ __forceinline__ float net_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }
__device__ __forceinline__ float net_log(float x) { return __builtin_amdgcn_logf(x) * 0.693147180559945309417f; }
__device__ __forceinline__ float net_pow(float x, float p) {
    return x > 0.0f ? __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(x)) : powf(x, p);
}

template <int N, class F>
__device__ __forceinline__ void map_array(float (&v)[N], F f) {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = f(v[i]);
}

// x^p without libm: exp2(p log2 |x|) (hardware exp2 / log2, ~1e-6 relative), the sign and the special cases by hand
__device__ __forceinline__ float pow_compact(float x, float p) {
    const float ax = fabsf(x);
    float r = __builtin_amdgcn_exp2f(p * __builtin_amdgcn_logf(ax));
    if (x < 0.0f) {
        const float fl = floorf(p);
        if (fl != p) r = __builtin_nanf("");                 // negative base, non-integer exponent
        else if (fl * 0.5f != floorf(fl * 0.5f)) r = -r;     // odd integer exponent keeps the sign
    }
    if (p == 0.0f) r = 1.0f;
    return r;
}

// THE definition of every unary stage code (Act, kernels.h): X(code, its value at x with the parameters p0, p1).  POW has two forms:
// the compact family (COMPACT: no libm anywhere in its code) computes it with pow_compact, every other one with net_pow.
#define BN_ACT_TABLE(X)                                                               \
    X(ACT_RELU, fmaxf(x, 0.0f))                                                       \
    X(ACT_CLIP, fminf(fmaxf(x, p0), p1))                                              \
    X(ACT_SIGMOID, net_sigmoid(x))                                                    \
    X(ACT_SILU, x * net_sigmoid(x))                                                   \
    X(ACT_HSIGMOID, fminf(fmaxf(p0 * x + p1, 0.0f), 1.0f))                            \
    X(ACT_HSWISH, x * fminf(fmaxf(x * (1.0f / 6.0f) + 0.5f, 0.0f), 1.0f))             \
    X(ACT_LEAKY, x >= 0.0f ? x : p0 * x)                                              \
    X(ACT_TANH, tanhf(x))                                                             \
    X(ACT_EXP, net_exp(x))                                                            \
    X(ACT_LOG, net_log(x))                                                            \
    X(ACT_SQRT, sqrtf(x))                                                             \
    X(ACT_ABS, fabsf(x))                                                              \
    X(ACT_NEG, -x)                                                                    \
    X(ACT_RECIP, 1.0f / x)                                                            \
    X(ACT_POW, COMPACT ? pow_compact(x, p0) : net_pow(x, p0))                         \
    X(ACT_AFFINE, p0 * x + p1)                                                        \
    X(ACT_MAXC, fmaxf(x, p0))                                                         \
    X(ACT_MINC, fminf(x, p0))                                                         \
    X(ACT_RSUB, p0 - x)                                                               \
    X(ACT_RDIV, p0 / x)                                                               \
    X(ACT_SQUARE, x * x)                                                              \
    X(ACT_FLOOR, floorf(x))                                                           \
    X(ACT_CEIL, ceilf(x))                                                             \
    X(ACT_ERF, erff(x))                                                               \
    X(ACT_SOFTPLUS, log1pf(expf(x)))                                                  \
    X(ACT_GTC, x > p0 ? 1.0f : 0.0f)                                                  \
    X(ACT_LTC, x < p0 ? 1.0f : 0.0f)                                                  \
    X(ACT_GEC, x >= p0 ? 1.0f : 0.0f)                                                 \
    X(ACT_LEC, x <= p0 ? 1.0f : 0.0f)                                                 \
    X(ACT_EQC, x == p0 ? 1.0f : 0.0f)                                                 \
    X(ACT_NEZ, x != 0.0f ? 1.0f : 0.0f)                                               \
    X(ACT_TRUNC, truncf(x))                                                           \
    X(ACT_ROUND, rintf(x))

// one code's formula, the code known at compile time
template <int ACT, bool COMPACT = false>
__device__ __forceinline__ float act_fn(float x, float p0, float p1) {
#define BN_ACT_FN(code, value) if constexpr (ACT == code) return value; else
    BN_ACT_TABLE(BN_ACT_FN) return x;
#undef BN_ACT_FN
}

// THE dispatcher: ONE branch on the (launch-uniform) code, then `apply` receives the selected formula as a float -> float function
// and runs it over whatever the caller holds (a register array, an accumulator tile, one value) -- a dispatch per element
// would cost a branch tree per element per stage.  SET (an ACT_SET_* of kernels.h) is the family's set: a code outside it
// generates no code here and is the identity, which the planner's predicates on the same constant keep from being asked for.
template <uint64_t SET, bool COMPACT = false, class Apply>
__device__ __forceinline__ void act_dispatch(int act, float p0, float p1, Apply apply) {
    switch (act) {
#define BN_ACT_CASE(code, value)                                                                             \
    case code:                                                                                               \
        if constexpr (act_in(SET, code)) apply([=](float x) { return act_fn<code, COMPACT>(x, p0, p1); });   \
        return;
        BN_ACT_TABLE(BN_ACT_CASE)
#undef BN_ACT_CASE
        default: return;
    }
}
template <uint64_t SET, bool COMPACT = false, int N>
__device__ __forceinline__ void act_array(int act, float p0, float p1, float (&v)[N]) {
    act_dispatch<SET, COMPACT>(act, p0, p1, [&](auto f) { map_array<N>(v, f); });
}
template <uint64_t SET, int NT>
__device__ __forceinline__ void act_tile(int act, float p0, float p1, floatx16 (&acc)[NT]) {
    act_dispatch<SET>(act, p0, p1, [&](auto f) {
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[t][r] = f(acc[t][r]);
    });
}
// one value of a kernel that applies its activation per element (every code)
__device__ __forceinline__ float act_apply(int act, float x, float p0, float p1) {
    act_dispatch<ACT_SET_ALL>(act, p0, p1, [&](auto f) { x = f(x); });
    return x;
}

template <int N, class F>
__device__ __forceinline__ void zip_array(float (&v)[N], const float (&w)[N], F f) {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = f(v[i], w[i]);
}
template <int N>
__device__ __forceinline__ void bin_array(int bin, int bsq, float (&v)[N], float (&w)[N]) {
    if (bsq) map_array<N>(w, [](float x) { return x * x; });
    switch (bin) {
        case BIN_ADD: zip_array<N>(v, w, [](float a, float b) { return a + b; }); return;
        case BIN_SUB: zip_array<N>(v, w, [](float a, float b) { return a - b; }); return;
        case BIN_MUL: zip_array<N>(v, w, [](float a, float b) { return a * b; }); return;
        case BIN_DIV: zip_array<N>(v, w, [](float a, float b) { return a / b; }); return;
        case BIN_POW: zip_array<N>(v, w, [](float a, float b) { return net_pow(a, b); }); return;
        case BIN_MAX: zip_array<N>(v, w, [](float a, float b) { return fmaxf(a, b); }); return;
        case BIN_MIN: zip_array<N>(v, w, [](float a, float b) { return fminf(a, b); }); return;
        case BIN_GT: zip_array<N>(v, w, [](float a, float b) { return a > b ? 1.0f : 0.0f; }); return;
        case BIN_LT: zip_array<N>(v, w, [](float a, float b) { return a < b ? 1.0f : 0.0f; }); return;
        case BIN_GE: zip_array<N>(v, w, [](float a, float b) { return a >= b ? 1.0f : 0.0f; }); return;
        case BIN_LE: zip_array<N>(v, w, [](float a, float b) { return a <= b ? 1.0f : 0.0f; }); return;
        case BIN_EQ: zip_array<N>(v, w, [](float a, float b) { return a == b ? 1.0f : 0.0f; }); return;
        case BIN_NE: zip_array<N>(v, w, [](float a, float b) { return a != b ? 1.0f : 0.0f; }); return;
        case BIN_SELA: zip_array<N>(v, w, [](float a, float b) { return b != 0.0f ? a : 0.0f; }); return;
        case BIN_SELB: zip_array<N>(v, w, [](float a, float b) { return b != 0.0f ? 0.0f : a; }); return;
        default: return;
    }
}

}  // namespace
// Stage functions of the absorbed chains, COMPACT on purpose: the full set and bin_array inline
// libm (tanhf, erff, powf, ...) for every instantiation -- with nine stage slots that made this kernel 676 KB of code,
// and walking through it ran at instruction-fetch speed (a 4-stage chain over 16 floats per thread cost 19 us per
// tile).  Only codes with a few-instruction body are accepted here (kernels.h, ACT_SET_COMPACT: the planner
// absorbs nothing else).
template <int N>
__device__ __forceinline__ void act_small(int act, float p0, float p1, float (&v)[N]) {
    act_array<ACT_SET_COMPACT, true>(act, p0, p1, v);
}

// binary stage against ONE scalar for the whole array (the absorbed per-sample chains: stft.hip, the framing GEMMs of kernels.hip)
template <int N>
__device__ __forceinline__ void bin_small(int bin, float b, float (&v)[N]) {
    if (bin == BIN_ADD) map_array<N>(v, [=](float a) { return a + b; });
    else if (bin == BIN_SUB) map_array<N>(v, [=](float a) { return a - b; });
    else if (bin == BIN_MUL) map_array<N>(v, [=](float a) { return a * b; });
    else if (bin == BIN_DIV) {
        // one divisor for the whole array: 1 / b once, then q = a r corrected by one residual step, which is what the
        // hardware's division sequence computes minus its scaling for denormal / overflowing quotients (3 instructions per
        // element instead of ~10; the absorbed chain divides the whole segment by max - min)
        const float r = 1.0f / b;
        map_array<N>(v, [=](float a) {
            const float q = a * r;
            return fmaf(fmaf(-q, b, a), r, q);
        });
    }
    else if (bin == BIN_MAX) map_array<N>(v, [=](float a) { return fmaxf(a, b); });
    else if (bin == BIN_MIN) map_array<N>(v, [=](float a) { return fminf(a, b); });
}

// The absorbed per-sample chain: up to four stages  v = act(bin(v, scalar)).  All indices are literals so that the
// fields stay in registers.
struct PreChain {
    int n, bin[4], act[4];
    float sc[4], p0[4], p1[4];
};
template <int S, int N>
__device__ __forceinline__ void pre_stage(const PreChain &c, float (&v)[N]) {
    if (S < c.n) {
        bin_small<N>(c.bin[S], c.sc[S], v);
        act_small<N>(c.act[S], c.p0[S], c.p1[S], v);
    }
}
template <int N>
__device__ __forceinline__ void pre_chain(const PreChain &c, float (&v)[N]) {
    pre_stage<0, N>(c, v);
    pre_stage<1, N>(c, v);
    pre_stage<2, N>(c, v);
    pre_stage<3, N>(c, v);
}

}  // namespace bn
