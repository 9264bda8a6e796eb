// The reference's confidence arithmetic on the device, shared by the kernels that rank confidences (topk.hip, prior.hip):
// f32::total_cmp as an integer key, and sigmoid(x) = 1 / (1 + exp(-x)) with glibc's expf restated operation for operation
// (see topk.hip's header comment), so confidences are bit-identical to the reference on an FMA-capable host.
// Device code only; every translation unit that includes it must be compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bn {
namespace {

__device__ __forceinline__ uint32_t total_key(uint32_t b) {
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the float bits a key came from
__device__ __forceinline__ uint32_t total_key_bits(uint32_t k) {
    return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
}

__constant__ uint64_t kExp2fTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

// glibc 2.35 expf, FMA build.  Compiled with -ffp-contract=off so only the
// explicit fma() calls fuse.
__device__ float expf_glibc(float x) {
    const uint32_t ix = __float_as_uint(x);
    const uint32_t abstop = (ix >> 20) & 0x7ffu;
    if (abstop >= 0x42bu) {  // |x| >= 88 or NaN
        if (ix == 0xff800000u) return 0.0f;
        if (abstop >= 0x7f8u) return x + x;
        if (x > 0x1.62e42ep6f) return __uint_as_float(0x7f800000u);  // overflow
        if (x < -0x1.9fe368p6f) return 0.0f;                         // underflow
    }
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0;
    const double Shift = 0x1.8p52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0;
    const double C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0;
    const double C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    const double xd = (double)x;
    double kd = fma(InvLn2N, xd, Shift);
    const uint64_t ki = (uint64_t)__double_as_longlong(kd);
    kd = kd - Shift;
    const double r = fma(InvLn2N, xd, -kd);
    const uint64_t t = kExp2fTab[ki & 31u] + (ki << 47);
    const double s = __longlong_as_double((long long)t);
    const double z = fma(C0, r, C1);
    const double r2 = r * r;
    double y = fma(r, C2, 1.0);
    y = fma(z, r2, y);
    y = y * s;
    return (float)y;
}

__device__ __forceinline__ float sigmoid_ref(float x) { return 1.0f / (1.0f + expf_glibc(-x)); }

}  // namespace
}  // namespace bn
