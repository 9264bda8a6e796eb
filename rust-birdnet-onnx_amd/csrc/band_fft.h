// One frame in one wave: the transform band_levels.hip and spectral_profile.hip share (the layout and the arithmetic are described in
// band_levels.hip's header; the error bound BN_BAND_EPS_ULPS of include/birdnet_hip.h is this code's).  BandFft<N> holds what a lane
// needs for every frame of a workgroup -- its window values, twiddles and bin indices, loaded once from the host's tables
// (band_plan.h, fill_tables) -- and frame() turns N samples of a window into the one-sided power of the lane's bins:
//   e[r]   P_k of bin k = L RR + rev(r), r < RR = N / 128 (RR consecutive bins per lane, L the 6-bit reversal of the lane)
//   e_top  P_{N/2} in lane 0, 0.0f in every other lane
// Every lane of the wave must call frame() together (cross-lane moves).  Plain f32, no fused multiply-add, no LDS.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bn {
namespace band {

constexpr uint32_t ilog2(uint32_t v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
constexpr uint32_t bitrev(uint32_t v, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}

template <uint32_t N>
struct BandFft {
    static constexpr uint32_t M = N / 2, RR = M / 64, LR = ilog2(RR);
    static_assert(RR >= 2 && RR <= 16 && (1u << LR) == RR, "frames of 256 .. 2048 samples");

    float2 hw[RR];      // the window at its two samples of register r
    float2 tw_reg[RR];  // stage s < LR, register r0 < RR >> (s + 1): at RR - (RR >> s) + r0 (RR - 1 in all)
    float2 tw_lane[5];  // the stages h = 32 .. 2 (h = 1 multiplies by 1)
    float2 tw_bin[RR];  // W_N^k of its bins
    uint32_t L;         // the 6-bit reversal of the lane
    uint32_t zero_from; // the lane that holds Z[M - L RR]

    // bin of register r of this lane
    __device__ __forceinline__ uint32_t bin(uint32_t r) const { return L * RR + bitrev(r, LR); }

    __device__ __forceinline__ void load_tables(const float *__restrict__ tab, uint32_t lane) {
        const float2 *__restrict__ tw = reinterpret_cast<const float2 *>(tab + N);  // W_N^k, k < N/2
        L = __brev(lane) >> 26;
        zero_from = __brev((64u - L) & 63u) >> 26;
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            hw[r] = *reinterpret_cast<const float2 *>(tab + 2u * (r * 64u + lane));
            tw_bin[r] = tw[L * RR + bitrev(r, LR)];
        }
#pragma unroll
        for (uint32_t s = 0; s < LR; s++) {
#pragma unroll
            for (uint32_t r0 = 0; r0 < (RR >> (s + 1)); r0++) tw_reg[RR - (RR >> s) + r0] = tw[(r0 * 64u + lane) << (s + 1)];
        }
#pragma unroll
        for (uint32_t s = 0; s < 5; s++) tw_lane[s] = tw[(lane & ((32u >> s) - 1u)) * ((N / 64u) << s)];
    }

    // The frame at window positions [base, base + N) of the window that starts at sample `start` and holds `valid` samples of the
    // recording (zeros behind them).  s_in / s_edge: scale * c_k / 4 for the inner bins and for bins 0 and N/2 (the unpack leaves
    // 2 X_k).  `bad` collects NaN or +-Inf among the samples this lane read
    template <class R>
    __device__ __forceinline__ void frame(const R &src, uint64_t start, uint32_t base, uint64_t valid, uint32_t lane, float s_in, float s_edge, uint32_t &bad,
                                          float (&e)[RR], float &e_top) const {
        float zr[RR], zi[RR];
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            const uint32_t p = base + 2u * (r * 64u + lane);
            float x0 = 0.0f, x1 = 0.0f;
            if (p < valid) x0 = src(start + p);
            if ((uint64_t)p + 1u < valid) x1 = src(start + p + 1u);
            bad |= !(fabsf(x0) < __builtin_inff());  // NaN or +-Inf
            bad |= !(fabsf(x1) < __builtin_inff());
            zr[r] = x0 * hw[r].x;
            zi[r] = x1 * hw[r].y;
        }
        // ---- stages inside a lane: points 64 h apart, h = RR/2 .. 1
#pragma unroll
        for (uint32_t s = 0; s < LR; s++) {
            const uint32_t h = RR >> (s + 1);
#pragma unroll
            for (uint32_t blk = 0; blk < RR; blk += 2 * h) {
#pragma unroll
                for (uint32_t r0 = 0; r0 < h; r0++) {
                    const uint32_t i = blk + r0;
                    const float2 w = tw_reg[RR - (RR >> s) + r0];
                    const float ar = zr[i], ai = zi[i], br = zr[i + h], bi = zi[i + h];
                    zr[i] = ar + br;
                    zi[i] = ai + bi;
                    const float dr = ar - br, di = ai - bi;
                    zr[i + h] = dr * w.x - di * w.y;
                    zi[i + h] = dr * w.y + di * w.x;
                }
            }
        }
        // ---- stages across lanes: points h = 32 .. 1 apart
#pragma unroll
        for (uint32_t s = 0; s < 6; s++) {
            const uint32_t h = 32u >> s;
            const bool upper = (lane & h) != 0;
#pragma unroll
            for (uint32_t r = 0; r < RR; r++) {
                const float pr = __shfl_xor(zr[r], (int)h), pi = __shfl_xor(zi[r], (int)h);
                const float ar = upper ? pr : zr[r], ai = upper ? pi : zi[r];
                const float br = upper ? zr[r] : pr, bi = upper ? zi[r] : pi;
                const float sr = ar + br, si = ai + bi, dr = ar - br, di = ai - bi;
                if (s < 5) {
                    const float2 w = tw_lane[s < 5 ? s : 0];
                    const float mr = dr * w.x - di * w.y, mi = dr * w.y + di * w.x;
                    zr[r] = upper ? mr : sr;
                    zi[r] = upper ? mi : si;
                } else {
                    zr[r] = upper ? dr : sr;
                    zi[r] = upper ? di : si;
                }
            }
        }
        // ---- the real-input unpack and the power of this lane's bins k = L RR + rev(r)
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            const uint32_t q = bitrev(r, LR);
            float pr, pi;
            if (q == 0) {
                pr = __shfl(zr[0], (int)zero_from);
                pi = __shfl(zi[0], (int)zero_from);
            } else {
                pr = __shfl_xor(zr[bitrev(RR - q, LR)], 63);
                pi = __shfl_xor(zi[bitrev(RR - q, LR)], 63);
            }
            const float ar = zr[r] + pr, ai = zi[r] - pi, br = zr[r] - pr, bi = zi[r] + pi;
            const float2 w = tw_bin[r];
            const float cr = w.x * br - w.y * bi, ci = w.x * bi + w.y * br;
            const float xr = ar + ci, xi = ai - cr;
            e[r] = (xr * xr + xi * xi) * ((q == 0 && L == 0) ? s_edge : s_in);
        }
        // bin N/2, from Z[0]: lane 0, register 0
        e_top = 0.0f;
        {
            const float d = zr[0] - zi[0], d2 = d + d;
            if (lane == 0) e_top = (d2 * d2 + 0.0f) * s_edge;
        }
    }
};

}  // namespace band
}  // namespace bn
