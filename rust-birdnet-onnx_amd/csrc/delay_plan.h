// The host-side arithmetic of cross-channel delay estimation (recording.cpp: bn_recording_delay, bn_delay_refine; kernel in delay.hip)
// that needs neither a device nor the runtime: a spec checked and copied, the frames of a window and each wave's run of them
// (band_plan.h's and profile_plan.h's, which this header includes), the normalisation Z of each weighting as the one f32 factor the
// kernel multiplies with, the LDS a workgroup takes, the floats of `out_curve` without a product that can wrap, the windows of one
// launch, where a lag lies in the row of correlations, the key that orders the lags of a window, and the parabola through a peak.
// Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_delay_plan.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "profile_plan.h"

namespace bn {
namespace delay {

constexpr uint32_t LANES = profile::LANES, WAVES = profile::WAVES;  // one workgroup per window, wave w owns frames [w q, (w + 1) q)
using band::last_sample_read;
using profile::lds_index;
using profile::wave_frames;

// a checked spec with what follows from it and S
struct Plan {
    uint32_t N = 0, hop = 0, lo = 0, hi = 0;
    uint32_t max_lag = 0, n_lags = 0;  // 2 max_lag + 1 <= N - 1
    uint32_t weighting = 0;
    uint32_t n_frames = 0;  // (S - N) / hop + 1
    uint32_t span = 0;      // window positions [0, span) are read
    uint32_t run = 0;       // q = ceil(n_frames / WAVES): the frames a wave owns
    float out_scale = 0.0f;  // PLAIN 1 / (4 Z): the kernel's spectra are 2 X, so its cross-spectrum is 4 G; PHAT 1 / Z: a unit phasor has no 4
};

// sum_n w_n^2 of the periodic Hann window of N samples, in double, as band::fill_tables adds it
inline double window_energy(uint32_t N) {
    const double two_pi = 6.283185307179586476925286766559;
    double sum2 = 0.0;
    for (uint32_t n = 0; n < N; n++) {
        double w = 0.5 - 0.5 * std::cos(two_pi * (double)n / (double)N);
        if (n == 0) w = 0.0;
        if (2 * n == N) w = 1.0;
        sum2 += w * w;
    }
    return sum2;
}

// sum of c_k over the bins [lo, hi), hi <= N/2 + 1: c_k = 1 for k = 0 and k = N/2, 2 otherwise
constexpr uint32_t band_weight(uint32_t N, uint32_t lo, uint32_t hi) {
    return hi <= lo ? 0 : 2 * (hi - lo) - (lo == 0 ? 1u : 0u) - (hi == N / 2 + 1 ? 1u : 0u);
}

// Z of the header's rule, in double: PLAIN n_frames * N * sum w^2, PHAT the band's weight
inline double normaliser(uint32_t weighting, uint32_t N, uint32_t n_frames, uint32_t lo, uint32_t hi) {
    return weighting == BN_DELAY_PHAT ? (double)band_weight(N, lo, hi) : (double)n_frames * (double)N * window_energy(N);
}

// The plan of (spec, S).  Refuses a NULL spec and a spec_size below the struct's; the frame, hop, S and the bin range are the
// spectral profile's refusals (profile::check_spec); then max_lag above N/2 - 1 and a weighting that is neither.  The spec is read
// through memcpy: any alignment
inline bn_status check_spec(const bn_delay_spec *spec, size_t spec_size, uint64_t S, Plan *out) {
    if (!spec) return set_last_error(BN_ERR_INVALID_ARG, "null delay spec");
    if (spec_size < sizeof(bn_delay_spec)) return set_last_error(BN_ERR_INVALID_ARG, "spec_size is below sizeof(bn_delay_spec)");
    bn_delay_spec s;
    memcpy(&s, spec, sizeof(s));
    bn_profile_spec p{s.frame, s.hop, s.bin_lo, s.bin_hi};
    profile::Plan pp;
    if (bn_status st = profile::check_spec(&p, sizeof(p), S, &pp); st != BN_OK) return st;
    if (s.max_lag > pp.N / 2 - 1)
        return set_last_error(BN_ERR_INVALID_ARG, "max_lag " + std::to_string(s.max_lag) + " is above " + std::to_string(pp.N / 2 - 1) + " (frame / 2 - 1)");
    if (s.weighting != BN_DELAY_PLAIN && s.weighting != BN_DELAY_PHAT)
        return set_last_error(BN_ERR_INVALID_ARG, "weighting " + std::to_string(s.weighting) + " is neither BN_DELAY_PLAIN nor BN_DELAY_PHAT");
    *out = Plan{};
    out->N = pp.N, out->hop = pp.hop, out->lo = pp.lo, out->hi = pp.hi;
    out->max_lag = s.max_lag, out->n_lags = 2 * s.max_lag + 1, out->weighting = s.weighting;
    out->n_frames = pp.n_frames, out->span = pp.span, out->run = pp.run;
    // Z >= 1: the band is not empty
    out->out_scale = (float)((s.weighting == BN_DELAY_PHAT ? 1.0 : 0.25) / normaliser(s.weighting, pp.N, pp.n_frames, pp.lo, pp.hi));
    return BN_OK;
}

// What a workgroup holds in LDS: per wave a row of N/2 + 1 partial cross-spectra (real and imaginary planes), the row of N
// correlations, and per wave its non-finite flag and its best key
constexpr uint32_t lds_bytes(uint32_t N) {
    return WAVES * 2 * (N / 2 + 1) * (uint32_t)sizeof(float) + N * (uint32_t)sizeof(float) + WAVES * (uint32_t)(sizeof(uint32_t) + sizeof(uint64_t));
}

// where r[tau], -N/2 < tau < N/2, lies in the row of N correlations: tau mod N
constexpr uint32_t lag_index(uint32_t N, int32_t tau) { return (uint32_t)(tau + (int32_t)N) & (N - 1); }

// The order of the lags of a window as one number: the greater r wins; among equal values the smaller |tau|, then the negative
// one.  `bits` are r's, with -0.0f already made +0.0f; no NaN reaches here.  |tau| < 2^15
constexpr uint64_t peak_key(uint32_t bits, int32_t tau) {
    const uint32_t ordered = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);  // ascending with the float
    const uint32_t mag = (uint32_t)(tau < 0 ? -tau : tau);
    return ((uint64_t)ordered << 32) | (uint64_t)(((0xffffu - mag) << 1) | (tau < 0 ? 1u : 0u));
}
constexpr int32_t key_lag(uint64_t key) {
    const uint32_t low = (uint32_t)key, mag = 0xffffu - (low >> 1);
    return (low & 1u) ? -(int32_t)mag : (int32_t)mag;
}

// count * n_lags, the floats of out_curve; false if that is not a size_t's worth of bytes
inline bool curve_floats(size_t count, uint32_t n_lags, size_t *out) {
    if (n_lags == 0 || count > SIZE_MAX / sizeof(float) / n_lags) return false;
    *out = count * n_lags;
    return true;
}

// windows per launch: at most 2^20 (band levels' cut), and curves of at most 2^26 floats on the device
constexpr size_t piece_windows(uint32_t n_lags) {
    const size_t by_curve = ((size_t)1 << 26) / (n_lags ? n_lags : 1);
    return by_curve < ((size_t)1 << 20) ? by_curve : ((size_t)1 << 20);
}

// bn_delay_refine: the vertex of the parabola through (peak_lag - 1, before), (peak_lag, peak), (peak_lag + 1, after), in double,
// clamped to peak_lag +- 0.5; peak_lag itself where the three lie on a line or the record is flagged non-finite
inline bn_status refine(const bn_window_delay *w, size_t struct_size, double *lag_out) {
    if (!w || !lag_out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (struct_size < sizeof(bn_window_delay)) return set_last_error(BN_ERR_INVALID_ARG, "struct_size is below sizeof(bn_window_delay)");
    bn_window_delay r;
    memcpy(&r, w, sizeof(r));
    const double before = r.before, peak = r.peak, after = r.after;
    const double den = before - 2.0 * peak + after;
    double off = 0.0;
    if (!(r.flags & BN_LEVEL_NONFINITE) && den != 0.0) off = 0.5 * (before - after) / den;
    if (off != off) off = 0.0;  // fields that are not finite in a record that carries no flag
    if (off < -0.5) off = -0.5;
    if (off > 0.5) off = 0.5;
    *lag_out = (double)r.peak_lag + off;
    return BN_OK;
}

}  // namespace delay
}  // namespace bn
