// The host-side arithmetic of spectral-gating noise reduction (recording.cpp: bn_recording_create_denoised, bn_noise_floor; kernel in
// denoise.hip) that needs neither a device nor the runtime: the spec and the noise estimate checked and turned into the thresholds
// a_k, the frames, blocks and runs of a recording of any length n without a product that can wrap, where every (frame, register, lane)
// position of the kernel lies, the grid, the window table, and bn_noise_floor's selection.  Host code only, so that a stand-alone
// program can run it under a sanitizer (tools/asan_denoise_plan.cpp).
//
// GEOMETRY.  H = N / 2.  Frame t, t = 0 .. B, B = ceil(n / H), covers source positions [(t - 1) H, (t + 1) H); output block b < B,
// samples [b H, (b + 1) H) cut to n, is the second half of frame b plus the first half of frame b + 1.  A wave owns RUN consecutive
// blocks [b0, b1) and transforms frames b0 .. b1; a workgroup is WAVES waves.
//
// RUN = 16.  A wave transforms RUN + 1 frames for RUN blocks, so 1 / RUN of the transforms are redundant: 6.25 % at 16, 3.1 % at 32.
// Against that stands the number of workgroups a short recording gives: one minute at 48 kHz and N = 512 is 11 250 blocks, 176
// workgroups at RUN = 16 and 88 at RUN = 32, on a part with 256 compute units that each hold one such workgroup at the longest frame
// (a wave per SIMD).  Half the machine idle costs more than 3 % of the transforms, and a 3 s window (563 blocks) is 9 workgroups
// against 5; so 16.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "band_plan.h"

namespace bn {
namespace denoise {

constexpr uint32_t LANES = band::LANES, WAVES = band::WAVES;
constexpr uint32_t RUN = 16;  // output blocks per wave (see above)
static_assert(RUN == 16 || RUN == 32, "the redundancy 1 / RUN against the workgroups of a short recording");

// a checked spec
struct Plan {
    uint32_t N = 0, H = 0;
    float floor_gain = 0.0f;
    double alpha = 0.0;
};

// Refuses a NULL spec or noise, a spec_size below the struct's, a frame not in the list, alpha negative or non-finite, floor_gain
// outside [0, 1] or NaN, a noise entry that is negative or non-finite.  a_k = alpha * noise[k] is formed in double and rounded to
// f32 once (an overflow to +Inf gates the bin to floor_gain, as the rule's 1 - a / P does); `a` takes N/2 + 1 floats.  Spec and
// noise are read through memcpy: any alignment
inline bn_status check_spec(const bn_denoise_spec *spec, size_t spec_size, const float *noise, Plan *out, std::vector<float> *a) {
    if (!spec) return set_last_error(BN_ERR_INVALID_ARG, "null denoise spec");
    if (spec_size < sizeof(bn_denoise_spec)) return set_last_error(BN_ERR_INVALID_ARG, "spec_size is below sizeof(bn_denoise_spec)");
    bn_denoise_spec s;
    memcpy(&s, spec, sizeof(s));
    if (!band::frame_ok(s.frame)) return set_last_error(BN_ERR_INVALID_ARG, "frame " + std::to_string(s.frame) + " is not 256, 512, 1024 or 2048");
    if (!(s.alpha >= 0.0f) || !std::isfinite(s.alpha)) return set_last_error(BN_ERR_INVALID_ARG, "alpha must be finite and not negative");
    if (!(s.floor_gain >= 0.0f && s.floor_gain <= 1.0f)) return set_last_error(BN_ERR_INVALID_ARG, "floor_gain must lie in [0, 1]");
    if (!noise) return set_last_error(BN_ERR_INVALID_ARG, "null noise estimate");
    const uint32_t bins = s.frame / 2 + 1;
    a->assign(bins, 0.0f);
    for (uint32_t k = 0; k < bins; k++) {
        float v;
        memcpy(&v, reinterpret_cast<const char *>(noise) + (size_t)k * sizeof(float), sizeof(v));
        if (!(v >= 0.0f) || !std::isfinite(v)) return set_last_error(BN_ERR_INVALID_ARG, "noise[" + std::to_string(k) + "] is negative or not finite");
        const double p = (double)s.alpha * (double)v;
        (*a)[k] = p > (double)FLT_MAX ? INFINITY : (float)p;
    }
    *out = Plan{};
    out->N = s.frame, out->H = s.frame / 2, out->floor_gain = s.floor_gain, out->alpha = s.alpha;
    return BN_OK;
}

// ---- frames, blocks, runs.  Nothing below forms n + something or b * H for a b that is not a block of the recording
constexpr uint64_t n_blocks(uint64_t n, uint32_t N) { return n / (N / 2) + (n % (N / 2) != 0); }  // B; frames are 0 .. B
constexpr uint64_t n_waves(uint64_t n, uint32_t N) { return n_blocks(n, N) / RUN + (n_blocks(n, N) % RUN != 0); }
constexpr uint64_t n_groups(uint64_t n, uint32_t N) { return n_waves(n, N) / WAVES + (n_waves(n, N) % WAVES != 0); }
constexpr uint64_t GRID_MAX = 0x7fffffffull;
// the longest recording a call takes: its f32 store must have a size, and (B + 1) * H must not wrap
constexpr uint64_t N_MAX = (uint64_t)1 << 60;

// the blocks [*b0, *b1) of wave `wave` of workgroup `group` (empty past the end); it transforms frames *b0 .. *b1 if not empty
constexpr void wave_blocks(uint64_t B, uint64_t group, uint32_t wave, uint64_t *b0, uint64_t *b1) {
    const uint64_t w = group * WAVES + wave;  // < n_waves + WAVES <= 2^60 / 128 / 16 + 8
    const uint64_t first = w * RUN;           // <= B + WAVES * RUN
    *b0 = first < B ? first : B;
    *b1 = B - *b0 < RUN ? B : *b0 + RUN;
}

// ---- where the kernel's positions lie.  Register r < RR = N / 128 of lane l holds frame positions p and p + 1, p = 2 (64 r + l)
constexpr uint32_t frame_pos(uint32_t r, uint32_t lane) { return 2u * (64u * r + lane); }
// frame t's position p is source sample (t - 1) H + p: false where that is negative (a zero by the rule), else *at
constexpr bool source_of(uint64_t t, uint32_t H, uint32_t p, uint64_t *at) {
    if (t == 0 && p < H) return false;
    *at = t == 0 ? (uint64_t)(p - H) : (t - 1) * H + p;
    return true;
}
// THE REGISTER SHIFT.  H = 64 * (RR / 2) * 2, so position p >= H of frame t, which is position p - H of frame t + 1, sits in the same
// lane RR / 2 registers lower: frame_pos(r, l) - H == frame_pos(r - RR / 2, l)
constexpr bool shift_holds(uint32_t N, uint32_t r, uint32_t lane) {
    const uint32_t RR = N / 128, H = N / 2;
    return r >= RR / 2 && r < RR && frame_pos(r, lane) - H == frame_pos(r - RR / 2, lane);
}
// register r' < RR / 2 of lane l stores output samples block * H + frame_pos(r', l) and the one after it; how many of the two lie
// below n (0, 1 or 2)
constexpr uint32_t store_count(uint64_t n, uint64_t block, uint32_t H, uint32_t r, uint32_t lane, uint64_t *at) {
    *at = block * H + frame_pos(r, lane);  // block < B: block * H <= n - 1
    return *at >= n ? 0u : (n - *at >= 2 ? 2u : 1u);
}

// ---- the tables: N floats w_j = sin(pi j / N), the square root of the periodic Hann window, computed in double and rounded to f32
// once, exact at j = 0 (0) and j = N/2 (1).  (The twiddles are band levels': band::fill_tables.)  Returns 1 / (N sum w^2) of the
// DOUBLE window rounded to f32, the scale of the one-sided power: sum w^2 = N / 2, so it is the power of two 2 / N^2
constexpr size_t table_floats(uint32_t N) { return N; }
inline float fill_tables(uint32_t N, float *tab) {
    const double pi = 3.14159265358979323846264338327950288;
    double sum2 = 0.0;
    for (uint32_t j = 0; j < N; j++) {
        double w = std::sin(pi * (double)j / (double)N);
        if (j == 0) w = 0.0;
        if (2 * j == N) w = 1.0;
        tab[j] = (float)w;
        sum2 += w * w;
    }
    return (float)(1.0 / ((double)N * sum2));
}

// ---- bn_noise_floor: per bin the plane-0 value of rank floor(quantile * (count - 1)) among the windows; profile_bins is
// [count][BN_PROFILE_PLANES][n_bins].  +Inf sorts last (it is the largest float); a NaN, which the profile never writes, is refused
inline bn_status noise_floor(const float *profile_bins, size_t count, size_t n_bins, double quantile, float *noise_out) {
    if (!profile_bins || !noise_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (count == 0) return set_last_error(BN_ERR_INVALID_ARG, "count must be positive");
    if (n_bins == 0) return set_last_error(BN_ERR_INVALID_ARG, "n_bins must be positive");
    if (!(quantile >= 0.0 && quantile <= 1.0)) return set_last_error(BN_ERR_INVALID_ARG, "quantile must lie in [0, 1]");
    if (n_bins > SIZE_MAX / sizeof(float) / BN_PROFILE_PLANES || count > SIZE_MAX / sizeof(float) / BN_PROFILE_PLANES / n_bins)
        return set_last_error(BN_ERR_INVALID_ARG, "count * 3 * n_bins floats do not fit a size_t");
    size_t rank = (size_t)std::floor(quantile * (double)(count - 1));
    if (rank > count - 1) rank = count - 1;
    std::vector<float> col(count);
    std::vector<float> result(n_bins);
    for (size_t k = 0; k < n_bins; k++) {
        for (size_t i = 0; i < count; i++) {
            memcpy(&col[i], reinterpret_cast<const char *>(profile_bins) + (i * BN_PROFILE_PLANES * n_bins + k) * sizeof(float), sizeof(float));
            if (col[i] != col[i]) return set_last_error(BN_ERR_INVALID_ARG, "profile_bins holds a NaN");
        }
        std::nth_element(col.begin(), col.begin() + (ptrdiff_t)rank, col.end());
        result[k] = col[rank];
    }
    memcpy(noise_out, result.data(), n_bins * sizeof(float));  // a refusal writes nothing
    return BN_OK;
}

}  // namespace denoise
}  // namespace bn
