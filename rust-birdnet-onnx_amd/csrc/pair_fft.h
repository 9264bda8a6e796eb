// The transform of denoise_fft.h cut into the four pieces DenoiseFft::gate() runs in a row, for delay.hip, which puts its own
// arithmetic between them (two spectra, their cross-spectrum, one inverse per window).  Layout, twiddles and arithmetic are
// denoise_fft.h's, piece for piece -- see its header for the derivation.  gate() itself is NOT built from these: routing it through
// them changed the instruction order of every denoise_kernel instantiation, and the bits of a denoised recording are a contract, so
// denoise_fft.h stays as it is and only delay.hip includes this file.
//   forward       the radix-2 stages, in-lane h = RR/2 .. 1, then cross-lane h = 32 .. 1: lane l, register r then holds Z[k],
//                 k = L RR + rev(r), L the 6-bit reversal of l
//   unpack_pair   from Z and the partner lane's Z[M - k]: x = 2 X_k and y = conj(2 X_{M-k}); for k = 0 the pair is (0, N/2)
//   repack_pair   from U at bin k and V = conj of what stands at bin M - k: 4 Z~_k = (U + V) + i conj(W_N^k) (U - V)
//   inverse       the mirror image of forward with conjugated twiddles, without the halving: with the repack it returns
//                 sum_{k < N} U_k exp(+2 pi i jk / N) of the Hermitian extension of U, position j = 2 m in nr and 2 m + 1 in ni of
//                 lane and register m = 64 r + lane
// Every lane of the wave must call each piece together (cross-lane moves).  Plain f32, no fused multiply-add, no LDS, no math library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "band_fft.h"

namespace bn {
namespace delay {

template <uint32_t N>
struct PairFft {
    using F = band::BandFft<N>;
    static constexpr uint32_t M = F::M, RR = F::RR, LR = F::LR;

    static __device__ __forceinline__ void forward(const F &fft, float (&zr)[RR], float (&zi)[RR], uint32_t lane) {
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
    }

    // the partner lanes read zr / zi until the last pair is fetched: nothing may be written back into them before
    static __device__ __forceinline__ void unpack_pair(const F &fft, const float (&zr)[RR], const float (&zi)[RR], uint32_t r, float &xr, float &xi, float &yr,
                                                       float &yi) {
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
        xr = ar + ci, xi = ai - cr;  // 2 X_k
        yr = ar - ci, yi = ai + cr;  // conj(2 X_{M-k})
    }

    static __device__ __forceinline__ void repack_pair(const F &fft, uint32_t r, float ur, float ui, float vr, float vi, float &nr, float &ni) {
        const float2 w = fft.tw_bin[r];
        const float dr = ur - vr, di = ui - vi;
        const float er = w.x * dr + w.y * di, ei = w.x * di - w.y * dr;  // conj(W) (U - V)
        nr = (ur + vr) - ei;
        ni = (ui + vi) + er;
    }

    // across lanes the upper lane holds d: it sends d conj(w) and takes s
    static __device__ __forceinline__ void inverse(const F &fft, float (&nr)[RR], float (&ni)[RR], uint32_t lane) {
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
    }
};

}  // namespace delay
}  // namespace bn
