// spectral_profile_kernel -- the per-bin meter of bn_recording_spectral_profile (launched by recording.cpp; declarations in
// spectral_profile.h, the rule in include/birdnet_hip.h, "bn_recording_spectral_profile").  One workgroup of 256 lanes per window,
// templated on the frame length N and on the reader (pcm_read.h) like band_levels_kernel, and around the same transform (band_fft.h:
// one frame in one wave's registers), but with the other data flow: band levels reduces over the bins of a frame and hands frames to
// waves round-robin; this kernel keeps the bins and reduces over TIME, so time has to run inside a wave.
//
// TIME INSIDE A WAVE.  With q = ceil(F / 4), wave w owns the consecutive frames [w q, min((w + 1) q, F)) (profile::wave_frames).  The
// transform leaves bin k = rev6(lane) RR + rev(r) in the same lane and register for every frame, so a lane keeps, per bin it holds
// (RR = N / 128 of them, lane 0 also bin N/2), the previous frame's amplitude and three accumulators: sum P, sum A, sum |A - A_prev|,
// A = sqrtf(P) (correctly rounded).  All in registers: 4 (RR + 1) floats, 68 at N = 2048.  A wave whose run ends before F also
// transforms the first frame of the next run; that frame adds |A - A_prev| to plane 2 and nothing else.  So no amplitude travels
// between waves and the time loop touches no LDS.  Every accumulator adds its frames in ascending order from 0.0f; a frame that does
// not count for an accumulator adds 0.0f, which changes no bit of a non-negative sum.
//
// THE TOTAL is band levels' tree: a lane adds its RR bins in register order from 0.0f, lane 0 then bin N/2, the wave adds by the xor
// butterfly, the wave's owned frames in ascending order, the four waves as (w0 + w1) + (w2 + w3), one division by (float)F.
//
// BINS LEAVE THROUGH LDS ONCE PER WINDOW.  Each wave writes its three partial sums per bin into rows of N/2 + 1 floats (4 waves x 3
// planes; with the waves' totals, ACI shares and flags 49 248 bytes at N = 2048, profile::lds_bytes).  After one barrier lane t takes
// bins bin_lo + t, + 256, ...: (w0 + w1) + (w2 + w3) per plane, plane 0 divided by (float)F, three stores that are contiguous over
// the lanes -- the pass through LDS is what turns the bit-reversed lane order into that.  The same lane forms D_k / S_k (0 where
// S_k == 0) and adds its bins in ascending order; the wave adds by the xor butterfly, the waves as (w0 + w1) + (w2 + w3) after a
// second barrier.  Lanes 0 .. 3 store the record's four dwords.  No atomics, no scratch.
//
// BANK CONFLICTS.  The write of one register puts the 64 lanes RR floats apart (up to a 32-way conflict at N = 2048 if stored
// as is).  Rows are not padded; the index is swizzled instead, k ^ ((k >> 5) & (2 RR - 1)) (profile::lds_index): within a half wave
// (lanes 32 h .. 32 h + 31, rev6(lane) = 2 L' + h) the address is 2 RR L' + (h RR + q), and xor-ing the field below 2 RR with
// floor(L' / (16 / RR)) gives 32 different banks, so every ds_write of the 3 RR per lane is conflict free.  The reads of 32
// consecutive bins stay inside one or two aligned blocks of 32, each a permutation of its block: at most 2-way, once per window.
#include "spectral_profile.h"

#include "band_fft.h"
#include "kernels.h"
#include "pcm_read.h"

namespace bn {
namespace {

constexpr uint32_t PROFILE_WAVES = profile::WAVES, PLANES = BN_PROFILE_PLANES;

// delta's fixed part (plane 0): x*x, y*y and their sum count as 2; the scale, its f32 constant and the division as 3; the four waves;
// 2 spare.  The chain over a wave's frames is the ceil(F / 4) the header adds
static_assert(2 + 3 + band::ilog2(PROFILE_WAVES) + 2 == BN_PROFILE_POW_DEPTH, "BN_PROFILE_POW_DEPTH is plane 0's fixed depth");
// delta_a's fixed part (planes 1 and 2): the 4 u of the power are 2 u under the root; the root; the four waves; 2 spare (plane 2's
// subtraction takes the place of the root: 1 u relative to the difference)
static_assert(2 + 1 + band::ilog2(PROFILE_WAVES) + 2 == BN_PROFILE_AMP_DEPTH, "BN_PROFILE_AMP_DEPTH is the amplitude planes' fixed depth");
// aci: the quotient, a lane's bins at the longest frame, a wave, four waves, 2 spare
static_assert(1 + (band::FRAME_MAX / 2 + 1 + profile::LANES - 1) / profile::LANES + 6 + band::ilog2(PROFILE_WAVES) + 2 == BN_PROFILE_ACI_DEPTH,
              "BN_PROFILE_ACI_DEPTH is the ACI tree's depth");

// what the kernel needs of a plan, as kernel arguments (scalar registers)
struct ProfileArgs {
    uint32_t lo, hi, hop, n_frames, run;
    float scale;
};

__device__ __forceinline__ float profile_wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

template <uint32_t N, class R>
__global__ __launch_bounds__(256) void spectral_profile_kernel(WindowProfile *__restrict__ out, float *__restrict__ planes, const R src, uint64_t n_samples,
                                                              uint64_t first_start, uint64_t step, uint32_t S, const float *__restrict__ tab,
                                                              const ProfileArgs a) {
    constexpr uint32_t M = N / 2, RR = M / 64, ROW = M + 1;
    __shared__ float part[PROFILE_WAVES][PLANES][ROW];
    __shared__ float w_tot[PROFILE_WAVES], w_aci[PROFILE_WAVES];
    __shared__ uint32_t w_bad[PROFILE_WAVES];
    static_assert(sizeof(part) + sizeof(w_tot) + sizeof(w_aci) + sizeof(w_bad) == profile::lds_bytes(N), "the LDS profile_plan.h states");
    static_assert(profile::lds_index(N, M) == M && profile::lds_index(N, M - 1) < M, "the swizzle stays inside a row");
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t start = first_start + (uint64_t)blockIdx.x * step;
    // frames of the window that the recording holds
    const uint64_t valid = start < n_samples ? (n_samples - start < S ? n_samples - start : (uint64_t)S) : 0;
    band::BandFft<N> fft;
    fft.load_tables(tab, lane);

    // per bin of this lane (slot RR: bin N/2, which lane 0 alone holds): the last amplitude, sum P, sum A, sum |dA|
    float prev[RR + 1], sum_p[RR + 1], sum_a[RR + 1], sum_d[RR + 1];
#pragma unroll
    for (uint32_t r = 0; r <= RR; r++) prev[r] = 0.0f, sum_p[r] = 0.0f, sum_a[r] = 0.0f, sum_d[r] = 0.0f;
    float tot = 0.0f;
    uint32_t bad = 0;
    const float s_in = a.scale * 0.5f, s_edge = a.scale * 0.25f;  // c_k / 4: the unpack leaves 2 X_k

    uint32_t f0, f1;
    bool extra;
    profile::wave_frames(a.n_frames, a.run, wave, &f0, &f1, &extra);
    const uint32_t f_end = f1 + (extra ? 1u : 0u);  // <= n_frames
    for (uint32_t j = f0; j < f_end; j++) {
        const uint32_t base = j * a.hop;  // base + N <= S
        float e[RR], e_top;
        fft.frame(src, start, base, valid, lane, s_in, s_edge, bad, e, e_top);
        const bool own = j < f1, diff = j > f0;  // wave-uniform
        if (own) {
            float v = 0.0f;
#pragma unroll
            for (uint32_t r = 0; r < RR; r++) v = v + e[r];
            v = v + e_top;
            tot = tot + profile_wave_sum(v);
        }
#pragma unroll
        for (uint32_t r = 0; r <= RR; r++) {
            const float p = r < RR ? e[r < RR ? r : 0] : e_top;
            const float amp = sqrtf(p);
            const float d = fabsf(amp - prev[r]);
            sum_d[r] = sum_d[r] + (diff ? d : 0.0f);
            sum_p[r] = sum_p[r] + (own ? p : 0.0f);
            sum_a[r] = sum_a[r] + (own ? amp : 0.0f);
            prev[r] = amp;
        }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) bad |= __shfl_xor(bad, m);

    // ---- the wave's partial sums, bin by bin (a wave without frames writes its zeros)
#pragma unroll
    for (uint32_t r = 0; r < RR; r++) {
        const uint32_t at = profile::lds_index(N, fft.bin(r));
        part[wave][0][at] = sum_p[r];
        part[wave][1][at] = sum_a[r];
        part[wave][2][at] = sum_d[r];
    }
    if (lane == 0) {
        part[wave][0][M] = sum_p[RR];
        part[wave][1][M] = sum_a[RR];
        part[wave][2][M] = sum_d[RR];
        w_tot[wave] = tot;
        w_bad[wave] = bad;
    }
    __syncthreads();
    bad = w_bad[0] | w_bad[1] | w_bad[2] | w_bad[3];
    const float frames = (float)a.n_frames;
    const uint32_t n_bins = a.hi - a.lo;
    float *__restrict__ mine = planes ? planes + (size_t)blockIdx.x * PLANES * n_bins : nullptr;
    float aci = 0.0f;
    for (uint32_t k = a.lo + t; k < a.hi; k += profile::LANES) {
        const uint32_t at = profile::lds_index(N, k);
        float v[PLANES];
#pragma unroll
        for (uint32_t p = 0; p < PLANES; p++) v[p] = (part[0][p][at] + part[1][p][at]) + (part[2][p][at] + part[3][p][at]);
        v[0] = v[0] / frames;
        aci = aci + (v[1] > 0.0f ? v[2] / v[1] : 0.0f);
        if (mine) {
#pragma unroll
            for (uint32_t p = 0; p < PLANES; p++) mine[(size_t)p * n_bins + (k - a.lo)] = bad ? __builtin_inff() : v[p];
        }
    }
    aci = profile_wave_sum(aci);
    if (lane == 0) w_aci[wave] = aci;
    __syncthreads();
    if (t >= sizeof(WindowProfile) / 4) return;
    // lane t stores dword t of the record: aci, total_mean, flags, n_frames
    uint32_t bits;
    if (t < 2) {
        float v = t == 0 ? (w_aci[0] + w_aci[1]) + (w_aci[2] + w_aci[3]) : ((w_tot[0] + w_tot[1]) + (w_tot[2] + w_tot[3])) / frames;
        if (bad) v = __builtin_inff();  // never "quiet", never "simple": the sums of such a window mean nothing
        bits = __float_as_uint(v);
    } else if (t == 2) {
        bits = (valid < S ? BN_LEVEL_PADDED : 0u) | (bad ? BN_LEVEL_NONFINITE : 0u);
    } else {
        bits = a.n_frames;
    }
    reinterpret_cast<uint32_t *>(out + blockIdx.x)[t] = bits;
}

template <uint32_t N, class R>
void launch_one(hipStream_t s, WindowProfile *out, float *planes, const R &rd, uint64_t n_samples, uint64_t first_start, uint64_t step, uint32_t S,
                uint32_t count, const float *tab, const ProfileArgs &args) {
    hipLaunchKernelGGL((spectral_profile_kernel<N, R>), dim3(count), dim3(profile::LANES), 0, s, out, planes, rd, n_samples, first_start, step, S, tab, args);
}

}  // namespace

void launch_spectral_profile(hipStream_t s, WindowProfile *out, float *planes, const PcmSrc &src, uint64_t n_samples, uint64_t first_start, uint64_t step,
                             uint32_t S, uint32_t count, const profile::Plan &plan, const float *tab, float scale) {
    if (count == 0) return;
    if (!band::frame_ok(plan.N) || S < plan.N || plan.n_frames == 0 || plan.span > S || plan.lo >= plan.hi || plan.hi > plan.N / 2 + 1 ||
        plan.n_bins != plan.hi - plan.lo || plan.run != plan.n_frames / PROFILE_WAVES + (plan.n_frames % PROFILE_WAVES != 0) || !tab || !out) {
        launch_error("spectral profile: a plan the kernel cannot take");
        return;
    }
    const ProfileArgs args{plan.lo, plan.hi, plan.hop, plan.n_frames, plan.run, scale};
    const bool known = pcm_visit(src, [&](auto rd) {
        using R = decltype(rd);
        switch (plan.N) {
            case 256: launch_one<256, R>(s, out, planes, rd, n_samples, first_start, step, S, count, tab, args); break;
            case 512: launch_one<512, R>(s, out, planes, rd, n_samples, first_start, step, S, count, tab, args); break;
            case 1024: launch_one<1024, R>(s, out, planes, rd, n_samples, first_start, step, S, count, tab, args); break;
            default: launch_one<2048, R>(s, out, planes, rd, n_samples, first_start, step, S, count, tab, args); break;
        }
    });
    if (!known) launch_error("spectral profile: a layout no reader knows");
}

}  // namespace bn
