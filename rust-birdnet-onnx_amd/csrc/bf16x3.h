// f32 as three exact bf16 terms, device side (gemm_dma3.hip, gemm_b3.hip): x = hi + mid + lo with hi = x's top 8 significand bits (the f32
// with its low 16 bits cleared), mid the same of the remainder x - hi (exact), lo = x - hi - mid (at most 8 significant bits are left: a
// bf16 number).  The six partial products kept by the kernels (everything but mid lo, lo mid, lo lo) are each exact in f32; the dropped
// ones sum to less than 2^-21 |x w| in the worst case, 2^-24 |x w| in the root mean square (|mid| < 2^-7 |x|, |lo| < 2^-15 |x|).  Host side and the weight packers: plan_rules.h (split_bf16x3, pack_w3, pack_w3f).
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.h"

namespace bn {
namespace {

// the exact top bf16 of an f32 (as an f32), and two such tops side by side in one word (v_perm_b32): `lo16` in the low half
__device__ __forceinline__ float bf16_top(float v) { return __uint_as_float(__float_as_uint(v) & 0xffff0000u); }
__device__ __forceinline__ uint32_t bf16_pack(float hi16, float lo16) { return __builtin_amdgcn_perm(__float_as_uint(hi16), __float_as_uint(lo16), 0x07060302u); }
// two f32 values -> one word of two bf16 per plane, x0 in bits [0, 15]
__device__ __forceinline__ void split3_pair(float x0, float x1, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
    const float r10 = x0 - bf16_top(x0), r11 = x1 - bf16_top(x1);      // exact: the low 16 significand bits
    const float r20 = r10 - bf16_top(r10), r21 = r11 - bf16_top(r11);  // exact: at most 8 significant bits are left
    hi = bf16_pack(x1, x0);
    mid = bf16_pack(r11, r10);
    lo = bf16_pack(r21, r20);
}
// eight f32 values (a = elements 0..3, b = 4..7) -> three vectors of eight bf16, element e in bits [16 e, 16 e + 15]
__device__ __forceinline__ void split3(const floatx4 &a, const floatx4 &b, u32x4 &hi, u32x4 &mid, u32x4 &lo) {
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int p = 0; p < 4; p++) {
        uint32_t h, m, l;
        split3_pair(x[2 * p], x[2 * p + 1], h, m, l);
        hi[p] = h; mid[p] = m; lo[p] = l;
    }
}

__device__ __forceinline__ floatx4 mm_bf16(const u32x4 &w, const u32x4 &x, const floatx4 &acc) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, x), acc, 0, 0, 0);
}
__device__ __forceinline__ floatx16 mm32_bf16(const u32x4 &a, const u32x4 &b, const floatx16 &acc) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
// the six partial products of one 16 x 16 tile and 32-deep k, smallest terms first (fixed order: part of every output's arithmetic)
__device__ __forceinline__ floatx4 mm6(const u32x4 &wh, const u32x4 &wm, const u32x4 &wl, const u32x4 &xh, const u32x4 &xm,
                                    const u32x4 &xl, floatx4 a) {
    a = mm_bf16(wl, xh, a);
    a = mm_bf16(wh, xl, a);
    a = mm_bf16(wm, xm, a);
    a = mm_bf16(wm, xh, a);
    a = mm_bf16(wh, xm, a);
    a = mm_bf16(wh, xh, a);
    return a;
}

}  // namespace
}  // namespace bn
