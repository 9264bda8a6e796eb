// band_levels_kernel -- the band meter of bn_recording_band_levels (launched by recording.cpp; declarations in band_levels.h, the rule in
// include/birdnet_hip.h, "bn_recording_band_levels").  One workgroup of 256 lanes per window, templated on the frame length N and on
// the reader (pcm_read.h) like levels_kernel, so a sample is exactly the f32 value bn_recording_windows returns, 0 past the end.
// Wave w takes frames w, w + 4, ... of the window; nothing is shared between windows, so a window's bits cannot depend on the step.
//
// ONE FRAME IN ONE WAVE, in registers and cross-lane moves (no LDS traffic, so no bank conflict to avoid).  The N real samples are
// windowed on load and packed as M = N/2 complex points z[m] = (w x)[2m] + i (w x)[2m+1]; lane l holds points m = 64 r + l in
// registers r = 0 .. R-1, R = M/64 = 2, 4, 8 or 16 (its two samples are neighbours, a wave's loads one contiguous span).
//   * log2 R radix-2 decimation-in-frequency stages pair points 64 h apart: both sit in one lane (registers r and r + h).
//   * 6 more stages pair points h = 32 .. 1 apart inside each block of 64: lanes l and l ^ h exchange with __shfl_xor, the lane with
//     bit h clear keeps a + b, the other (a - b) * W.  The twiddle of a lane at such a stage is the same for every register.
//   * The spectrum is then in bit-reversed order: lane l, register r holds Z[k], k = L R + rev(r), L = the 6-bit reversal of l --
//     R CONSECUTIVE bins per lane.  The real-input unpack of bin k needs Z[M - k]: for rev(r) = q >= 1 that is register
//     rev(R - q) of lane l ^ 63, for q = 0 register 0 of the lane whose reversal is (64 - L) % 64.
//         2 X_k = (Z_k + conj Z_{M-k}) - i W_N^k (Z_k - conj Z_{M-k}),  k < M;    2 X_M = 2 (Re Z_0 - Im Z_0)  (lane 0)
//     and bin k's power is |2 X_k|^2 * (c_k / 4) * scale, scale = 1 / (N sum w^2) from the host.
// Every twiddle, window value and index a lane needs is loop-invariant: loaded from the tables once per workgroup, kept in
// registers over its frames.  The tables are computed in double on the host and rounded once (band_plan.h); there is no sincosf here.
//
// THE TREE (BN_BAND_SUM_DEPTH; every addition a plain f32 addition, the library is built with -ffp-contract=off).  Per frame and
// band: a lane adds its R bins in register order r = 0 .. R-1 from 0.0f, bins outside the band as 0.0f, lane 0 then bin N/2
// (R + 1 <= 17 additions); the wave adds v = v + v(lane ^ m), m = 32 .. 1 (6; every lane ends with the same bits).  Per wave the
// frames are added in ascending order from 0.0f (ceil(n_frames / 4)), the four waves as (w0 + w1) + (w2 + w3) through LDS (2), and
// the sum is divided by (float)n_frames once.  The maximum runs over the same values.  The order is a function of (S, spec) alone.
// No atomics, no scratch; lanes 0 .. 19 store the window's 20 dwords.
#include "band_levels.h"

#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "device_mem.h"
#include "kernels.h"
#include "pcm_read.h"

namespace bn {
namespace {

constexpr uint32_t BAND_WAVES = band::WAVES, BAND_SLOTS = BN_BAND_MAX + 1;  // the bands, then the total
constexpr uint32_t BAND_DWORDS = sizeof(WindowBands) / 4;

constexpr uint32_t ilog2(uint32_t v) { return v <= 1 ? 0 : 1 + ilog2(v >> 1); }
constexpr uint32_t bitrev(uint32_t v, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; i++) r |= ((v >> i) & 1u) << (bits - 1 - i);
    return r;
}
// eps: 7 u per radix-2 stage (twiddle rounding, the complex product, the additions) over the log2(N/2) stages of the
// longest frame, 2 u for the rounded window and its product, 7 u for the unpack, 1 u for what is of second order
static_assert(7 * ilog2(band::FRAME_MAX / 2) + 2 + 7 + 1 == BN_BAND_EPS_ULPS, "BN_BAND_EPS_ULPS is this transform's bound");
// delta's fixed part: a lane's bins at the longest frame and bin N/2, a wave, four waves; x*x, y*y and their sum count as 2, the
// scale, the division and the f32 scale constant as 3, 2 spare
static_assert((band::FRAME_MAX / 128 + 1) + 6 + 2 + 7 == BN_BAND_SUM_DEPTH, "BN_BAND_SUM_DEPTH is this tree's fixed depth");
static_assert(BAND_DWORDS == 2 * BN_BAND_MAX + 4, "mean[], max[], two totals, flags, n_frames");

// what the kernel needs of a plan, as kernel arguments (scalar registers)
struct BandArgs {
    uint32_t lo[BN_BAND_MAX], hi[BN_BAND_MAX];
    uint32_t n_bands, hop, n_frames;
    float scale;
};

__device__ __forceinline__ float band_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

template <uint32_t N, class R>
__global__ __launch_bounds__(256) void band_levels_kernel(WindowBands *__restrict__ out, const R src, uint64_t n_samples, uint64_t first_start, uint64_t step,
                                                         uint32_t S, const float *__restrict__ tab, const BandArgs a) {
    constexpr uint32_t M = N / 2, RR = M / 64, LR = ilog2(RR);
    static_assert(RR >= 2 && RR <= 16 && (1u << LR) == RR, "frames of 256 .. 2048 samples");
    __shared__ float w_sum[BAND_WAVES][BAND_SLOTS], w_max[BAND_WAVES][BAND_SLOTS];
    __shared__ uint32_t w_bad[BAND_WAVES];
    static_assert(sizeof(w_sum) + sizeof(w_max) + sizeof(w_bad) == band::lds_bytes(N), "the LDS band_plan.h states");
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t start = first_start + (uint64_t)blockIdx.x * step;
    // frames of the window that the recording holds
    const uint64_t valid = start < n_samples ? (n_samples - start < S ? n_samples - start : (uint64_t)S) : 0;
    const float2 *__restrict__ tw = reinterpret_cast<const float2 *>(tab + N);  // W_N^k, k < N/2
    const uint32_t L = __brev(lane) >> 26;                                       // the 6-bit reversal of the lane
    const uint32_t zero_from = __brev((64u - L) & 63u) >> 26;                    // the lane that holds Z[M - L R]

    // ---- what a lane needs for every frame
    float2 hw[RR];       // the window at its two samples of register r
    float2 tw_reg[RR];   // stage s < LR, register r0 < RR >> (s + 1): at RR - (RR >> s) + r0 (RR - 1 in all)
    float2 tw_lane[5];   // the stages h = 32 .. 2 (h = 1 multiplies by 1)
    float2 tw_bin[RR];   // W_N^k of its bins
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

    float acc_sum[BAND_SLOTS], acc_max[BAND_SLOTS];
#pragma unroll
    for (uint32_t b = 0; b < BAND_SLOTS; b++) acc_sum[b] = 0.0f, acc_max[b] = 0.0f;
    uint32_t bad = 0;
    const float s_in = a.scale * 0.5f, s_edge = a.scale * 0.25f;  // c_k / 4: the unpack below leaves 2 X_k

    for (uint32_t j = wave; j < a.n_frames; j += BAND_WAVES) {
        const uint32_t base = j * a.hop;  // base + N <= S
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
        float e[RR];
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
        float e_top = 0.0f;
        {
            const float d = zr[0] - zi[0], d2 = d + d;
            if (lane == 0) e_top = (d2 * d2 + 0.0f) * s_edge;
        }
        // ---- the bands and the total of this frame
#pragma unroll
        for (uint32_t b = 0; b < BAND_SLOTS; b++) {
            if (b < BN_BAND_MAX && b >= a.n_bands) continue;  // uniform
            const uint32_t lo = b < BN_BAND_MAX ? a.lo[b < BN_BAND_MAX ? b : 0] : 0u, hi = b < BN_BAND_MAX ? a.hi[b < BN_BAND_MAX ? b : 0] : M + 1u;
            float v = 0.0f;
#pragma unroll
            for (uint32_t r = 0; r < RR; r++) {
                const uint32_t k = L * RR + bitrev(r, LR);
                v = v + ((k >= lo && k < hi) ? e[r] : 0.0f);
            }
            v = v + ((M >= lo && M < hi) ? e_top : 0.0f);
            v = band_wave_sum(v);
            acc_sum[b] = acc_sum[b] + v;
            acc_max[b] = fmaxf(acc_max[b], v);
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) bad |= __shfl_xor(bad, m);
    if (lane == 0) {
#pragma unroll
        for (uint32_t b = 0; b < BAND_SLOTS; b++) w_sum[wave][b] = acc_sum[b], w_max[wave][b] = acc_max[b];
        w_bad[wave] = bad;
    }
    __syncthreads();
    if (t >= BAND_DWORDS) return;
    // lane t stores dword t of the record: mean[0..8), max[0..8), total_mean, total_max, flags, n_frames
    bad = w_bad[0] | w_bad[1] | w_bad[2] | w_bad[3];
    uint32_t bits;
    if (t < 2 * BN_BAND_MAX + 2) {
        const bool is_max = (t >= BN_BAND_MAX && t < 2 * BN_BAND_MAX) || t == 2 * BN_BAND_MAX + 1;
        const uint32_t slot = t < BN_BAND_MAX ? t : t < 2 * BN_BAND_MAX ? t - BN_BAND_MAX : BN_BAND_MAX;
        float v;
        if (is_max) v = fmaxf(fmaxf(w_max[0][slot], w_max[1][slot]), fmaxf(w_max[2][slot], w_max[3][slot]));
        else v = ((w_sum[0][slot] + w_sum[1][slot]) + (w_sum[2][slot] + w_sum[3][slot])) / (float)a.n_frames;
        // never "quiet": the sums of such a window mean nothing.  Bands the spec does not have stay 0
        if (bad && (slot == BN_BAND_MAX || slot < a.n_bands)) v = __builtin_inff();
        bits = __float_as_uint(v);
    } else if (t == 2 * BN_BAND_MAX + 2) {
        bits = (valid < S ? BN_LEVEL_PADDED : 0u) | (bad ? BN_LEVEL_NONFINITE : 0u);
    } else {
        bits = a.n_frames;
    }
    reinterpret_cast<uint32_t *>(out + blockIdx.x)[t] = bits;
}

template <uint32_t N, class R>
void launch_one(hipStream_t s, WindowBands *out, const R &rd, uint64_t n_samples, uint64_t first_start, uint64_t step, uint32_t S, uint32_t count,
                const float *tab, const BandArgs &args) {
    hipLaunchKernelGGL((band_levels_kernel<N, R>), dim3(count), dim3(band::LANES), 0, s, out, rd, n_samples, first_start, step, S, tab, args);
}

struct Tables {
    DeviceBuf<float> d;
    float scale = 0.0f;
};

}  // namespace

hipError_t band_tables(int device, uint32_t N, const float **tab, float *scale) {
    // never destroyed: the tables live as long as the process, and at exit the runtime may be gone before static destructors run
    static std::mutex mu;
    static auto *cache = new std::map<std::pair<int, uint32_t>, Tables>();
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache->find({device, N});
    if (it == cache->end()) {
        std::vector<float> host(band::table_floats(N));
        Tables tb;
        tb.scale = band::fill_tables(N, host.data());
        hipError_t e = tb.d.alloc(host.size() * sizeof(float));
        if (e == hipSuccess) e = gated::Memcpy(tb.d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        it = cache->emplace(std::make_pair(device, N), std::move(tb)).first;
    }
    *tab = it->second.d.get();
    *scale = it->second.scale;
    return hipSuccess;
}

void launch_band_levels(hipStream_t s, WindowBands *out, const PcmSrc &src, uint64_t n_samples, uint64_t first_start, uint64_t step, uint32_t S, uint32_t count,
                        const band::Plan &plan, const float *tab, float scale) {
    if (count == 0) return;
    if (!band::frame_ok(plan.N) || S < plan.N || plan.n_frames == 0 || plan.span > S || !tab) {
        launch_error("band levels: a plan the kernel cannot take");
        return;
    }
    BandArgs args;
    for (uint32_t b = 0; b < BN_BAND_MAX; b++) args.lo[b] = plan.lo[b], args.hi[b] = plan.hi[b];
    args.n_bands = plan.n_bands, args.hop = plan.hop, args.n_frames = plan.n_frames, args.scale = scale;
    const bool known = pcm_visit(src, [&](auto rd) {
        using R = decltype(rd);
        switch (plan.N) {
            case 256: launch_one<256, R>(s, out, rd, n_samples, first_start, step, S, count, tab, args); break;
            case 512: launch_one<512, R>(s, out, rd, n_samples, first_start, step, S, count, tab, args); break;
            case 1024: launch_one<1024, R>(s, out, rd, n_samples, first_start, step, S, count, tab, args); break;
            default: launch_one<2048, R>(s, out, rd, n_samples, first_start, step, S, count, tab, args); break;
        }
    });
    if (!known) launch_error("band levels: a layout no reader knows");
}

}  // namespace bn
