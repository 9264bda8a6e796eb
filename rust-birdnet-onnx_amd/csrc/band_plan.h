// The host-side arithmetic of band-limited window levels (recording.cpp: bn_recording_band_levels, bn_band_bins; kernel in
// band_levels.hip) that needs neither a device nor the runtime: a spec checked and copied, the frames of a window and the samples
// behind the last one that no frame reads, the last sample a window range reads (what an asynchronous upload is waited for; no sum
// that can wrap is formed), the LDS a workgroup takes, the bins of a band given in hertz, and the tables the kernel reads (periodic
// Hann window and the twiddles, computed in double and rounded to f32 once).  Host code only, so that a stand-alone program can run
// it under a sanitizer (tools/asan_band_plan.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "last_error.h"

namespace bn {
namespace band {

constexpr uint32_t LANES = 256, WAVES = LANES / 64;  // one workgroup per window, wave w takes frames w, w + WAVES, ...
constexpr uint32_t FRAME_MIN = 256, FRAME_MAX = 2048;

inline bool frame_ok(uint32_t n) { return n == 256 || n == 512 || n == 1024 || n == 2048; }

// a checked spec with what follows from it and S
struct Plan {
    uint32_t N = 0, hop = 0, n_bands = 0;
    uint32_t n_frames = 0;  // (S - N) / hop + 1
    uint32_t span = 0;      // window positions [0, span) are read: (n_frames - 1) * hop + N <= S
    uint32_t unread = 0;    // S - span < hop trailing positions no full frame covers
    uint32_t lo[BN_BAND_MAX] = {}, hi[BN_BAND_MAX] = {};  // entries >= n_bands are the empty band [0, 0)
};

// frames of N samples every `hop` inside a window of S >= N samples
inline uint32_t n_frames(uint64_t S, uint32_t N, uint32_t hop) { return (uint32_t)((S - N) / hop) + 1; }

// The plan of (spec, S).  Refuses a NULL spec, a spec_size below the struct's, a frame not in the list, S < frame (S == 0
// included) or S >= 2^32, hop 0 or above the frame, n_bands 0 or above BN_BAND_MAX, and a band that is empty or reaches past bin
// N/2.  The spec is read through memcpy: the caller's pointer may have any alignment
inline bn_status check_spec(const bn_band_spec *spec, size_t spec_size, uint64_t S, Plan *out) {
    if (!spec) return set_last_error(BN_ERR_INVALID_ARG, "null band spec");
    if (spec_size < sizeof(bn_band_spec)) return set_last_error(BN_ERR_INVALID_ARG, "spec_size is below sizeof(bn_band_spec)");
    bn_band_spec s;
    memcpy(&s, spec, sizeof(s));
    if (!frame_ok(s.frame)) return set_last_error(BN_ERR_INVALID_ARG, "frame " + std::to_string(s.frame) + " is not 256, 512, 1024 or 2048");
    if (S > 0xffffffffull) return set_last_error(BN_ERR_INVALID_ARG, "segment_samples must be below 2^32");
    if (S < s.frame)
        return set_last_error(BN_ERR_INVALID_ARG, "segment_samples " + std::to_string(S) + " is below the frame of " + std::to_string(s.frame) + " samples");
    if (s.hop == 0 || s.hop > s.frame) return set_last_error(BN_ERR_INVALID_ARG, "hop " + std::to_string(s.hop) + " is not in 1.." + std::to_string(s.frame));
    if (s.n_bands == 0 || s.n_bands > BN_BAND_MAX)
        return set_last_error(BN_ERR_INVALID_ARG, "n_bands " + std::to_string(s.n_bands) + " is not in 1.." + std::to_string(BN_BAND_MAX));
    *out = Plan{};
    for (uint32_t b = 0; b < s.n_bands; b++) {
        if (s.bin_lo[b] >= s.bin_hi[b] || s.bin_hi[b] > s.frame / 2 + 1)
            return set_last_error(BN_ERR_INVALID_ARG, "band " + std::to_string(b) + ": bins [" + std::to_string(s.bin_lo[b]) + ", " + std::to_string(s.bin_hi[b]) +
                                                          ") are empty or reach past bin " + std::to_string(s.frame / 2));
        out->lo[b] = s.bin_lo[b];
        out->hi[b] = s.bin_hi[b];
    }
    out->N = s.frame, out->hop = s.hop, out->n_bands = s.n_bands;
    out->n_frames = n_frames(S, s.frame, s.hop);
    // (n_frames - 1) * hop <= S - N < 2^32: the product cannot wrap
    out->span = (out->n_frames - 1) * s.hop + s.frame;
    out->unread = (uint32_t)S - out->span;
    return BN_OK;
}

// The last sample of a recording of n samples that any frame of window `last_window` at `step` reads, the window's positions
// [0, span) being read; false if the window does not exist (last_window * step >= n, a product that wraps included).  Neither
// last_window * step nor start + span is formed where it could wrap
inline bool last_sample_read(uint64_t n, uint64_t last_window, uint64_t step, uint64_t span, uint64_t *out) {
    if (n == 0 || step == 0 || span == 0) return false;
    if (last_window > (n - 1) / step) return false;  // so last_window * step <= n - 1
    const uint64_t start = last_window * step, left = n - start;
    *out = start + ((span < left ? span : left) - 1);
    return true;
}

// What a workgroup holds in LDS: per wave the sums and the maxima of the BN_BAND_MAX bands and the total, and its non-finite flag.
// The transform itself runs in registers and cross-lane moves, so the figure does not depend on N
constexpr uint32_t lds_bytes(uint32_t /*N*/) { return WAVES * (2 * (BN_BAND_MAX + 1) * (uint32_t)sizeof(float) + (uint32_t)sizeof(uint32_t)); }

// bn_band_bins: bin k of a frame of N samples at `rate` lies at k * rate / N Hz, k = 0 .. N/2, and belongs to [lo_hz, hi_hz) iff
// that centre does.  k * rate (< 2^43) and hz * N (N a power of two) are exact in double, so every comparison is
inline bn_status bins(uint32_t rate, uint32_t N, double lo_hz, double hi_hz, uint32_t *bin_lo, uint32_t *bin_hi) {
    if (!bin_lo || !bin_hi) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (rate == 0) return set_last_error(BN_ERR_INVALID_ARG, "sample_rate must be positive");
    if (!frame_ok(N)) return set_last_error(BN_ERR_INVALID_ARG, "frame " + std::to_string(N) + " is not 256, 512, 1024 or 2048");
    if (!(lo_hz < hi_hz)) return set_last_error(BN_ERR_INVALID_ARG, "lo_hz must be below hi_hz");
    const uint32_t top = N / 2 + 1;
    // the first bin whose centre is at or above hz, top if none is
    auto first_at = [&](double hz) -> uint32_t {
        const double x = hz * (double)N / (double)rate;
        if (!(x > 0.0)) return 0;
        if (x > (double)top) return top;
        uint32_t k = (uint32_t)std::ceil(x);
        if (k > top) k = top;
        while (k > 0 && (double)(k - 1) * (double)rate >= hz * (double)N) k--;
        while (k < top && (double)k * (double)rate < hz * (double)N) k++;
        return k;
    };
    const uint32_t lo = first_at(lo_hz), hi = first_at(hi_hz);
    if (lo >= hi) return set_last_error(BN_ERR_INVALID_ARG, "the band holds no bin centre");
    *bin_lo = lo, *bin_hi = hi;
    return BN_OK;
}

// The kernel's tables for a frame of N samples, 2 N floats: hann[n] = 0.5 - 0.5 cos(2 pi n / N), n < N, then N / 2 twiddles
// (cos, -sin)(2 pi k / N), k < N / 2, as (re, im) pairs.  Computed in double, rounded to f32 once; the exact values at the
// multiples of a quarter turn are set, not computed.  Returns 1 / (N * sum hann^2) of the DOUBLE window, rounded to f32: the
// scale of the one-sided power
constexpr size_t table_floats(uint32_t N) { return 2 * (size_t)N; }
inline float fill_tables(uint32_t N, float *tab) {
    const double two_pi = 6.283185307179586476925286766559;
    double sum2 = 0.0;
    for (uint32_t n = 0; n < N; n++) {
        double w = 0.5 - 0.5 * std::cos(two_pi * (double)n / (double)N);
        if (n == 0) w = 0.0;
        if (2 * n == N) w = 1.0;
        tab[n] = (float)w;
        sum2 += w * w;
    }
    for (uint32_t k = 0; k < N / 2; k++) {
        double c = std::cos(two_pi * (double)k / (double)N), s = -std::sin(two_pi * (double)k / (double)N);
        if (k == 0) c = 1.0, s = 0.0;
        if (4 * k == N) c = 0.0, s = -1.0;
        tab[N + 2 * k] = (float)c;
        tab[N + 2 * k + 1] = (float)s;
    }
    return (float)(1.0 / ((double)N * sum2));
}

}  // namespace band
}  // namespace bn
