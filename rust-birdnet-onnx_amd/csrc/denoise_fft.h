// One frame in one wave, there and back: the transform of denoise.hip.  The layout is band_fft.h's -- N windowed real samples packed
// as M = N/2 complex points, lane l holds point m = 64 r + l (frame positions 2 m and 2 m + 1) in register r < RR = N / 128 -- and so
// are the twiddle tables, which this struct takes from a band::BandFft<N> (its Hann values are never read, so they cost no register).
// Unlike band_fft.h, which keeps only the power of a bin, gate() keeps the complex spectrum:
//   1. the forward stages, band_fft.h's: in-lane h = RR/2 .. 1, then cross-lane h = 32 .. 1 (decimation in frequency; bit-reversed out:
//      lane l, register r holds Z[k], k = L RR + rev(r), L the 6-bit reversal of l).
//   2. the real-input unpack.  With Z' = Z[M - k] fetched from the partner lane as band_fft.h fetches it, A = Z + conj Z',
//      C = W_N^k (Z - conj Z'):        2 X_k = A - i C,        conj(2 X_{M-k}) = A + i C.
//      So BOTH spectra of the pair (k, M - k) are in this lane, and the partner lane, which holds bin M - k, forms the same two.  For
//      k = 0 (lane 0, register 0) the partner is the lane itself and the pair is (0, N/2): bin N/2 needs no code of its own.
//   3. the gain of each of the two, from its own power and threshold: g = 1 where a == 0, else max(floor_gain, 1 - a / P); P == 0
//      gives 1 - Inf = -Inf and so floor_gain.  The one division of the kernel.  No further exchange: the lane knows a_k and a_{M-k}.
//   4. the repack.  With U = g_k (A - i C), V = g_{M-k} (A + i C):     4 Z~_k = (U + V) + i conj(W_N^k) (U - V).
//   5. the inverse stages, the mirror image of 1 with conjugated twiddles: cross-lane h = 1 .. 32, then in-lane h = 1 .. RR/2; each
//      undoes (a + b, (a - b) w) as s + d conj(w), s - d conj(w), without the halving, which leaves a factor M.
// The factors 4 and M are taken out with the gains (s_out = 1 / (2 N), a power of two), so gate() returns, in the register and lane
// each windowed sample came from, (1/N) sum_k g_k X_k exp(+2 pi i jk / N): the frame before its synthesis window.
// Every lane of the wave must call gate() together (cross-lane moves).  Plain f32, no fused multiply-add, no LDS, no math library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "band_fft.h"

namespace bn {
namespace denoise {

template <uint32_t N>
struct DenoiseFft {
    using F = band::BandFft<N>;
    static constexpr uint32_t M = F::M, RR = F::RR, LR = F::LR;
    static constexpr float S_OUT = 1.0f / (2.0f * (float)N);  // 4 from the unpack and repack, M from the inverse stages

    F fft;                    // twiddles, L, zero_from
    float a_own[RR], a_par[RR];  // a_k of its bins k = L RR + rev(r), and of their partners M - k
    float floor_gain, s_in, s_edge;  // scale * c_k / 4 for the inner bins and for bins 0 and N/2 (the unpack leaves 2 X_k)

    // band_tab: band::fill_tables' (the twiddles behind its window); a: the N/2 + 1 thresholds; scale = 1 / (N sum w^2)
    __device__ __forceinline__ void load(const float *__restrict__ band_tab, const float *__restrict__ a, uint32_t lane, float floor, float scale) {
        fft.load_tables(band_tab, lane);
        floor_gain = floor, s_in = scale * 0.5f, s_edge = scale * 0.25f;
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            const uint32_t k = fft.bin(r);  // < M
            a_own[r] = a[k];
            a_par[r] = a[M - k];
        }
    }

    __device__ __forceinline__ float gain(float a, float p) const { return a == 0.0f ? 1.0f : fmaxf(floor_gain, 1.0f - a / p); }

    __device__ __forceinline__ void gate(float (&zr)[RR], float (&zi)[RR], uint32_t lane) const {
        // ---- 1. forward, inside a lane: points 64 h apart, h = RR/2 .. 1
#pragma unroll
        for (uint32_t s = 0; s < LR; s++) {
            const uint32_t h = RR >> (s + 1);
#pragma unroll
            for (uint32_t blk = 0; blk < RR; blk += 2 * h) {
#pragma unroll
                for (uint32_t r0 = 0; r0 < h; r0++) {
                    const uint32_t i = blk + r0;
                    const float2 w = fft.tw_reg[RR - (RR >> s) + r0];
                    const float ar = zr[i], ai = zi[i], br = zr[i + h], bi = zi[i + h];
                    zr[i] = ar + br;
                    zi[i] = ai + bi;
                    const float dr = ar - br, di = ai - bi;
                    zr[i + h] = dr * w.x - di * w.y;
                    zi[i + h] = dr * w.y + di * w.x;
                }
            }
        }
        // ---- forward, across lanes: points h = 32 .. 1 apart
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
                    const float2 w = fft.tw_lane[s < 5 ? s : 0];
                    const float mr = dr * w.x - di * w.y, mi = dr * w.y + di * w.x;
                    zr[r] = upper ? mr : sr;
                    zi[r] = upper ? mi : si;
                } else {
                    zr[r] = upper ? dr : sr;
                    zi[r] = upper ? di : si;
                }
            }
        }
        // ---- 2 .. 4. unpack, gain, repack of the pair (k, M - k), k = L RR + rev(r).  Into a second array: the partner lanes read
        // zr / zi until the last fetch
        float nr[RR], ni[RR];
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            const uint32_t q = band::bitrev(r, LR);
            float pr, pi;
            if (q == 0) {
                pr = __shfl(zr[0], (int)fft.zero_from);
                pi = __shfl(zi[0], (int)fft.zero_from);
            } else {
                pr = __shfl_xor(zr[band::bitrev(RR - q, LR)], 63);
                pi = __shfl_xor(zi[band::bitrev(RR - q, LR)], 63);
            }
            const float ar = zr[r] + pr, ai = zi[r] - pi, br = zr[r] - pr, bi = zi[r] + pi;
            const float2 w = fft.tw_bin[r];
            const float cr = w.x * br - w.y * bi, ci = w.x * bi + w.y * br;
            const float xr = ar + ci, xi = ai - cr;  // 2 X_k
            const float yr = ar - ci, yi = ai + cr;  // conj(2 X_{M-k})
            const float sc = (q == 0 && fft.L == 0) ? s_edge : s_in;
            const float g = gain(a_own[r], (xr * xr + xi * xi) * sc) * S_OUT, gp = gain(a_par[r], (yr * yr + yi * yi) * sc) * S_OUT;
            const float ur = g * xr, ui = g * xi, vr = gp * yr, vi = gp * yi;
            const float dr = ur - vr, di = ui - vi;
            const float er = w.x * dr + w.y * di, ei = w.x * di - w.y * dr;  // conj(W) (U - V)
            nr[r] = (ur + vr) - ei;
            ni[r] = (ui + vi) + er;
        }
        // ---- 5. inverse, across lanes: h = 1 .. 32.  The upper lane holds d: it sends d conj(w) and takes s
#pragma unroll
        for (uint32_t s = 6; s-- > 0;) {
            const uint32_t h = 32u >> s;
            const bool upper = (lane & h) != 0;
#pragma unroll
            for (uint32_t r = 0; r < RR; r++) {
                float vr = nr[r], vi = ni[r];
                if (s < 5) {
                    const float2 w = fft.tw_lane[s < 5 ? s : 0];
                    const float mr = vr * w.x + vi * w.y, mi = vi * w.x - vr * w.y;
                    vr = upper ? mr : vr;
                    vi = upper ? mi : vi;
                }
                const float pr = __shfl_xor(vr, (int)h), pi = __shfl_xor(vi, (int)h);
                nr[r] = upper ? pr - vr : vr + pr;
                ni[r] = upper ? pi - vi : vi + pi;
            }
        }
        // ---- inverse, inside a lane: h = 1 .. RR/2
#pragma unroll
        for (uint32_t s = LR; s-- > 0;) {
            const uint32_t h = RR >> (s + 1);
#pragma unroll
            for (uint32_t blk = 0; blk < RR; blk += 2 * h) {
#pragma unroll
                for (uint32_t r0 = 0; r0 < h; r0++) {
                    const uint32_t i = blk + r0;
                    const float2 w = fft.tw_reg[RR - (RR >> s) + r0];
                    const float dr = nr[i + h], di = ni[i + h];
                    const float tr = dr * w.x + di * w.y, ti = di * w.x - dr * w.y;
                    const float sr = nr[i], si = ni[i];
                    nr[i] = sr + tr;
                    ni[i] = si + ti;
                    nr[i + h] = sr - tr;
                    ni[i + h] = si - ti;
                }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) zr[r] = nr[r], zi[r] = ni[r];
    }
};

}  // namespace denoise
}  // namespace bn
