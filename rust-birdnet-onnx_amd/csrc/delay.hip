// delay_kernel -- the generalised cross-correlation of bn_recording_delay (launched by recording.cpp; declarations in delay.h, the rule
// in include/birdnet_hip.h, "bn_recording_delay", the host's arithmetic in delay_plan.h).  One workgroup of 256 lanes per window,
// templated on the frame length N and on ONE reader (pcm_read.h) that serves both recordings, with spectral_profile.hip's data flow:
// time runs inside a wave, bins leave once per window through swizzled LDS rows.  New here is what happens in between.
//
// TWO FRAMES, ONE SET OF TABLES.  A wave windows frame t of a and frame t of b with the same band::BandFft<N> tables and runs both
// through the forward stages (pair_fft.h).  The real-input unpack of bin k needs the partner lane's Z[M - k] of the SAME frame, so
// both packed spectra stay in registers (4 RR floats) while the lane walks its RR bins: unpack a, unpack b, and
// A conj(B) = (ar br + ai bi) + i (ai br - ar bi), four multiplies and two adds, each sum added to its own accumulator.  No fused
// multiply-add.  The unpack leaves 2 X, so the sums are 4 G; the 4 leaves with PLAIN's normalisation (plan.out_scale = 1 / (4 Z))
// and in PHAT's division by the magnitude (out_scale = 1 / Z).
//
// TIME INSIDE A WAVE.  Wave w owns frames [w q, min((w + 1) q, F)), q = ceil(F / 4) (profile::wave_frames) and keeps its partial G in
// registers, added in ascending frame order from 0.0f.  The unpack offers both spectra of a pair (k, M - k) in one lane, which
// would be 4 RR accumulators; this kernel keeps the lane's OWN bins only, 2 RR + 2: every bin below N/2 is some lane's own bin, the partner lane
// would accumulate the same bin a second time from differently rounded values, and the one wave that runs the inverse has to fetch
// its partner bins from LDS in any case, because the four waves' partials meet there.  Bin N/2 is nobody's own bin: it is the partner
// of bin 0, and lane 0 keeps it in the two extra accumulators.  Half the multiplies, 32 fewer registers at N = 2048.
//
// ONE PASS THROUGH LDS PER WINDOW.  Each wave writes its partial into a row of N/2 + 1 values per component at profile::lds_index's
// swizzle (conflict free from the bit-reversed lane order).  After one barrier wave 0 reads, in the transform's own lane and register
// order, its own bin k and the partner bin M - k, each as (w0 + w1) + (w2 + w3) per component; zeroes what lies outside
// [bin_lo, bin_hi); for PHAT divides by the magnitude (one correctly rounded root, one division per bin, 0 where the magnitude is 0);
// drops the imaginary part of bins 0 and N/2 (the rule takes Re, and the repack would fold it into the other bins); and runs the
// repack and the inverse stages once.  r lands at positions 2 m and 2 m + 1 of lane and register m and goes to one LDS row of N
// floats as 8-byte stores contiguous over the lanes.  After a second barrier all 256 lanes scale and store the 2 max_lag + 1 lags
// contiguously (if a curve is wanted) and reduce delay::peak_key, which encodes the tie rule, by the xor butterfly; after a third,
// lanes 0 .. 5 pick the best of the four waves' keys and store the record's dwords.  No atomics, no scratch.
//
// REGISTERS (gfx950, the N = 2048 instantiations, from the cross-compile's kernel metadata).  The live set in the time loop is the
// tables (about 106 floats), both packed spectra (64) and the accumulators (34); the compiler keeps all of it in the unified file:
//   PcmMono<int16_t>, PcmMono<float>   342 VGPRs (256 + 86 accumulation registers used as spill space), scratch 0, LDS 41 040 bytes
//   PcmFrames<I16 | F32 | I32 | U8>    478 VGPRs (256 + 222), scratch 0
//   PcmFrames<I24>                     480 VGPRs (256 + 224), scratch 0
// Above 256 a workgroup's four waves have a SIMD each to themselves, which a workgroup of 256 lanes has in any case.  The interleaved
// readers hoist their address arithmetic for both recordings ahead of the transforms; nobody has measured what that costs.
// pair_fft.h, not a split of DenoiseFft::gate(): see that header.
#include "delay.h"

#include <type_traits>

#include "band_fft.h"
#include "kernels.h"
#include "pair_fft.h"
#include "pcm_read.h"

namespace bn {
namespace {

constexpr uint32_t DELAY_WAVES = delay::WAVES;

// delta_k's fixed depth, as a complex magnitude (3/2 >= sqrt 2 times a component's): the products and their sum count as 2, the four
// waves as 2; 2 spare.  The chain over a wave's frames is the 2 q the header adds (>= sqrt 2 * q)
static_assert((3 * (2 + band::ilog2(DELAY_WAVES)) + 1) / 2 + 2 == BN_DELAY_ACC_DEPTH, "BN_DELAY_ACC_DEPTH is the cross-spectrum's fixed depth");
// the unit phasor: the squares and their sum are 2 u of the squared magnitude, 1 u under the root; the root; the reciprocal; the
// product; 2 spare
static_assert(1 + 1 + 1 + 1 + 2 == BN_DELAY_PHAT_ULPS, "BN_DELAY_PHAT_ULPS is the weighting's share");
// behind the inverse: 1 / (4 Z) or 1 / Z rounded to f32 once, the product with it; 2 spare
static_assert(1 + 1 + 2 == BN_DELAY_OUT_ULPS, "BN_DELAY_OUT_ULPS is the normalisation's share");
// the inverse is the forward's mirror image (denoise.hip states the same): one eps per direction
static_assert(7 * band::ilog2(band::FRAME_MAX / 2) + 2 + 7 + 1 == BN_BAND_EPS_ULPS, "one eps per transform direction");

// what the kernel needs of a plan, as kernel arguments (scalar registers)
struct DelayArgs {
    uint32_t lo, hi, hop, n_frames, run, max_lag, weighting;
    float scale;
};

// the window's frame at positions [base, base + N), windowed, as band::BandFft<N>::frame reads it: M complex points, zeros behind
// the `valid` samples the recording holds; `bad` collects NaN or +-Inf among the samples this lane read
template <uint32_t N, class R>
__device__ __forceinline__ void load_frame(const band::BandFft<N> &fft, const R &src, uint64_t start, uint32_t base, uint64_t valid, uint32_t lane, uint32_t &bad,
                                           float (&zr)[N / 128], float (&zi)[N / 128]) {
#pragma unroll
    for (uint32_t r = 0; r < N / 128; r++) {
        const uint32_t p = base + 2u * (r * 64u + lane);
        float x0 = 0.0f, x1 = 0.0f;
        if (p < valid) x0 = src(start + p);
        if ((uint64_t)p + 1u < valid) x1 = src(start + p + 1u);
        bad |= !(fabsf(x0) < __builtin_inff());  // NaN or +-Inf
        bad |= !(fabsf(x1) < __builtin_inff());
        zr[r] = x0 * fft.hw[r].x;
        zi[r] = x1 * fft.hw[r].y;
    }
}

// Psi of bin k from the combined 4 G
__device__ __forceinline__ void weigh(float &re, float &im, uint32_t k, const DelayArgs &a) {
    const bool in_band = k >= a.lo && k < a.hi;
    if (a.weighting == BN_DELAY_PHAT) {
        const float mag = sqrtf(re * re + im * im);
        const float inv = 1.0f / mag;
        const bool keep = in_band && mag != 0.0f;
        re = keep ? re * inv : 0.0f;
        im = keep ? im * inv : 0.0f;
    } else {
        re = in_band ? re : 0.0f;
        im = in_band ? im : 0.0f;
    }
}

template <uint32_t N, class R>
__global__ __launch_bounds__(256) void delay_kernel(WindowDelay *__restrict__ out, float *__restrict__ curve, const R src_a, const R src_b, uint64_t n_a,
                                                   uint64_t n_b, uint64_t first_start, uint64_t step, uint32_t S, const float *__restrict__ tab,
                                                   const DelayArgs a) {
    using P = delay::PairFft<N>;
    constexpr uint32_t M = N / 2, RR = M / 64, ROW = M + 1;
    __shared__ uint64_t w_key[DELAY_WAVES];
    __shared__ float part[DELAY_WAVES][2][ROW];
    __shared__ float corr[N];
    __shared__ uint32_t w_bad[DELAY_WAVES];
    static_assert(sizeof(part) + sizeof(corr) + sizeof(w_bad) + sizeof(w_key) == delay::lds_bytes(N), "the LDS delay_plan.h states");
    static_assert(delay::lds_index(N, M) == M && delay::lds_index(N, M - 1) < M, "the swizzle stays inside a row");
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t start = first_start + (uint64_t)blockIdx.x * step;
    // samples of the window that each recording holds
    const uint64_t valid_a = start < n_a ? (n_a - start < S ? n_a - start : (uint64_t)S) : 0;
    const uint64_t valid_b = start < n_b ? (n_b - start < S ? n_b - start : (uint64_t)S) : 0;
    band::BandFft<N> fft;
    fft.load_tables(tab, lane);

    // 4 G of this lane's bins, and of bin N/2 (lane 0 alone holds it: the partner of its bin 0)
    float g_re[RR], g_im[RR], top_re = 0.0f, top_im = 0.0f;
#pragma unroll
    for (uint32_t r = 0; r < RR; r++) g_re[r] = 0.0f, g_im[r] = 0.0f;
    uint32_t bad = 0;

    uint32_t f0, f1;
    bool extra;
    delay::wave_frames(a.n_frames, a.run, wave, &f0, &f1, &extra);
    for (uint32_t j = f0; j < f1; j++) {
        const uint32_t base = j * a.hop;  // base + N <= S
        float ar[RR], ai[RR], br[RR], bi[RR];
        load_frame<N>(fft, src_a, start, base, valid_a, lane, bad, ar, ai);
        P::forward(fft, ar, ai, lane);
        load_frame<N>(fft, src_b, start, base, valid_b, lane, bad, br, bi);
        P::forward(fft, br, bi, lane);
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            float xar, xai, yar, yai, xbr, xbi, ybr, ybi;
            P::unpack_pair(fft, ar, ai, r, xar, xai, yar, yai);
            P::unpack_pair(fft, br, bi, r, xbr, xbi, ybr, ybi);
            g_re[r] = g_re[r] + (xar * xbr + xai * xbi);
            g_im[r] = g_im[r] + (xai * xbr - xar * xbi);
            if (r == 0) {
                // y = conj(2 X_{M-k}): conj(ya) yb is the cross-spectrum of the partner bin, N/2 in lane 0
                top_re = top_re + (yar * ybr + yai * ybi);
                top_im = top_im + (yar * ybi - yai * ybr);
            }
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) bad |= __shfl_xor(bad, m);

    // ---- the wave's partial sums, bin by bin (a wave without frames writes its zeros)
#pragma unroll
    for (uint32_t r = 0; r < RR; r++) {
        const uint32_t at = delay::lds_index(N, fft.bin(r));
        part[wave][0][at] = g_re[r];
        part[wave][1][at] = g_im[r];
    }
    if (lane == 0) {
        part[wave][0][M] = top_re;
        part[wave][1][M] = top_im;
        w_bad[wave] = bad;
    }
    __syncthreads();

    // ---- one wave: the combined bins back in the transform's order, the weighting, the repack and the inverse
    if (wave == 0) {
        float nr[RR], ni[RR];
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) {
            const uint32_t k = fft.bin(r), kp = M - k;  // k == 0: the pair (0, N/2), M stays where it is under the swizzle
            const uint32_t at = delay::lds_index(N, k), atp = delay::lds_index(N, kp);
            float ur = (part[0][0][at] + part[1][0][at]) + (part[2][0][at] + part[3][0][at]);
            float ui = (part[0][1][at] + part[1][1][at]) + (part[2][1][at] + part[3][1][at]);
            float pr = (part[0][0][atp] + part[1][0][atp]) + (part[2][0][atp] + part[3][0][atp]);
            float pi = (part[0][1][atp] + part[1][1][atp]) + (part[2][1][atp] + part[3][1][atp]);
            weigh(ur, ui, k, a);
            weigh(pr, pi, kp, a);
            if (k == 0) ui = 0.0f, pi = 0.0f;  // bins 0 and N/2 enter with their real parts
            P::repack_pair(fft, r, ur, ui, pr, -pi, nr[r], ni[r]);
        }
        P::inverse(fft, nr, ni, lane);
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) *reinterpret_cast<float2 *>(&corr[2u * (r * 64u + lane)]) = make_float2(nr[r], ni[r]);
    }
    __syncthreads();
    bad = w_bad[0] | w_bad[1] | w_bad[2] | w_bad[3];

    // ---- the lags: r[tau] = corr[tau mod N] * out_scale, -0.0f stored as +0.0f so that equal values have equal bits
    const auto lag_value = [&](int32_t tau) {
        const float v = corr[delay::lag_index(N, tau)] * a.scale;
        return v == 0.0f ? 0.0f : v;
    };
    const uint32_t n_lags = 2u * a.max_lag + 1u;
    float *__restrict__ mine = curve ? curve + (size_t)blockIdx.x * n_lags : nullptr;
    uint64_t best = 0;  // below every key
    for (uint32_t i = t; i < n_lags; i += delay::LANES) {
        const int32_t tau = (int32_t)i - (int32_t)a.max_lag;
        const float v = lag_value(tau);
        if (mine) mine[i] = bad ? __builtin_nanf("") : v;
        const uint64_t key = delay::peak_key(__float_as_uint(v), tau);
        best = key > best ? key : best;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), m), lo = __shfl_xor((uint32_t)best, m);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        best = other > best ? other : best;
    }
    if (lane == 0) w_key[wave] = best;
    __syncthreads();
    if (t >= sizeof(WindowDelay) / 4) return;
    // lane t stores dword t of the record: peak_lag, peak, before, after, flags, n_frames
    const uint64_t k01 = w_key[0] > w_key[1] ? w_key[0] : w_key[1], k23 = w_key[2] > w_key[3] ? w_key[2] : w_key[3];
    const int32_t lag = bad ? 0 : delay::key_lag(k01 > k23 ? k01 : k23);  // |lag| <= max_lag <= N/2 - 1: both neighbours exist
    uint32_t bits;
    if (t == 0) {
        bits = (uint32_t)lag;
    } else if (t < 4) {
        const float v = lag_value(lag + (t == 2 ? -1 : t == 3 ? 1 : 0));
        bits = __float_as_uint(bad ? __builtin_nanf("") : v);
    } else if (t == 4) {
        bits = ((valid_a < S || valid_b < S) ? BN_LEVEL_PADDED : 0u) | (bad ? BN_LEVEL_NONFINITE : 0u);
    } else {
        bits = a.n_frames;
    }
    reinterpret_cast<uint32_t *>(out + blockIdx.x)[t] = bits;
}

template <uint32_t N, class R>
void launch_one(hipStream_t s, WindowDelay *out, float *curve, const R &ra, const R &rb, uint64_t n_a, uint64_t n_b, uint64_t first_start, uint64_t step,
                uint32_t S, uint32_t count, const float *tab, const DelayArgs &args) {
    hipLaunchKernelGGL((delay_kernel<N, R>), dim3(count), dim3(delay::LANES), 0, s, out, curve, ra, rb, n_a, n_b, first_start, step, S, tab, args);
}

}  // namespace

void launch_delay(hipStream_t s, WindowDelay *out, float *curve, const PcmSrc &a, uint64_t n_a, const PcmSrc &b, uint64_t n_b, uint64_t first_start,
                  uint64_t step, uint32_t S, uint32_t count, const delay::Plan &plan, const float *tab) {
    if (count == 0) return;
    if (!band::frame_ok(plan.N) || S < plan.N || plan.n_frames == 0 || plan.span > S || plan.hop == 0 || plan.lo >= plan.hi || plan.hi > plan.N / 2 + 1 ||
        plan.max_lag > plan.N / 2 - 1 || plan.n_lags != 2 * plan.max_lag + 1 || (plan.weighting != BN_DELAY_PLAIN && plan.weighting != BN_DELAY_PHAT) ||
        plan.run != plan.n_frames / DELAY_WAVES + (plan.n_frames % DELAY_WAVES != 0) || !tab || !out) {
        launch_error("delay: a plan the kernel cannot take");
        return;
    }
    const DelayArgs args{plan.lo, plan.hi, plan.hop, plan.n_frames, plan.run, plan.max_lag, plan.weighting, plan.out_scale};
    bool same = false;
    const bool known = pcm_visit(a, [&](auto ra) {
        using R = decltype(ra);
        pcm_visit(b, [&](auto rb) {
            if constexpr (std::is_same_v<R, decltype(rb)>) {
                same = true;
                switch (plan.N) {
                    case 256: launch_one<256, R>(s, out, curve, ra, rb, n_a, n_b, first_start, step, S, count, tab, args); break;
                    case 512: launch_one<512, R>(s, out, curve, ra, rb, n_a, n_b, first_start, step, S, count, tab, args); break;
                    case 1024: launch_one<1024, R>(s, out, curve, ra, rb, n_a, n_b, first_start, step, S, count, tab, args); break;
                    default: launch_one<2048, R>(s, out, curve, ra, rb, n_a, n_b, first_start, step, S, count, tab, args); break;
                }
            }
        });
    });
    if (!known) launch_error("delay: a layout no reader knows");
    else if (!same) launch_error("delay: the two recordings take different readers");
}

}  // namespace bn
