// The host-side arithmetic of FIR filtering (recording.cpp: bn_recording_create_filtered, bn_fir_bandpass; kernel in fir.hip) that
// needs neither a device nor the runtime: the refusals of a tap list, the windowed-sinc designer (double, rounded to f32 once), the
// geometry of a workgroup's chunk -- padded depth, halo, LDS planes -- and the packer that lays the taps out as the Toeplitz operand
// of the matrix instruction.  Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_fir_plan.cpp).
//
// THE PRODUCT.  With c = (n_taps - 1) / 2 the filter is y[n] = sum_t taps[t] x[n + c - t].  A tile is 256 consecutive outputs
// Y[j][i] = y[t0 + 16 i + j] = sum_k A[j][k] B[k][i], j, i < 16, with
//   A[j][k] = taps[j + n_taps - 1 - k]  where that index is in [0, n_taps), else 0          (the taps alone: one image per call)
//   B[k][i] = x[t0 - c + 16 i + k]                                                          (a window of the chunk's samples)
// k = j + n_taps - 1 - t runs over [0, n_taps + 14], so the depth is K = n_taps + 15 rounded up to the instruction's 32.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "last_error.h"
#include "plan_rules.h"

namespace bn {

// modified Bessel function of the first kind, order 0 (the Kaiser window of the resampler's table and of the designer here)
inline double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

namespace fir {

constexpr uint32_t LANES = 256, WAVES = LANES / 64;
constexpr uint32_t TILE = 256;                          // outputs of one 16 x 16 tile
constexpr uint32_t TILES_PER_WAVE = 4;                  // one A fragment read feeds four tiles
constexpr uint32_t CHUNK = TILE * TILES_PER_WAVE * WAVES;  // outputs of a workgroup: 4096
constexpr double KAISER_BETA = 8.6;
static_assert(CHUNK == 4096, "the chunk the documents and BN_FIR_CHUNK name");

inline bool count_ok(size_t n_taps) { return n_taps >= 1 && n_taps <= BN_FIR_MAX_TAPS && n_taps % 2 == 1; }
inline bn_status refuse_count(size_t n_taps) {
    return set_last_error(BN_ERR_INVALID_ARG, "n_taps " + std::to_string(n_taps) + " is not odd and in 1.." + std::to_string(BN_FIR_MAX_TAPS));
}

// the geometry of a checked tap count
constexpr uint32_t depth(uint32_t n_taps) { return (n_taps + 15 + 31) & ~31u; }  // K
constexpr uint32_t steps(uint32_t n_taps) { return depth(n_taps) / 32; }
constexpr uint32_t halo(uint32_t n_taps) { return (n_taps - 1) / 2; }            // c: samples before the chunk's first output
// a plane holds x[c0 - c + p], p < plane_elems: the last tile's last column starts at CHUNK - 16 and reads K deep.  Only
// p < CHUNK + n_taps - 1 meet a tap; the rest meet A's zero padding and are stored as 0
constexpr uint32_t plane_elems(uint32_t n_taps) { return CHUNK - 16 + depth(n_taps); }
constexpr uint32_t live_elems(uint32_t n_taps) { return CHUNK + n_taps - 1; }
constexpr uint32_t lds_bytes(uint32_t n_taps) { return 3 * plane_elems(n_taps) * (uint32_t)sizeof(uint16_t); }
static_assert(lds_bytes(BN_FIR_MAX_TAPS) == 36960 && lds_bytes(BN_FIR_MAX_TAPS) <= 40 * 1024, "three planes of the longest filter");
static_assert(plane_elems(1) % 8 == 0 && live_elems(BN_FIR_MAX_TAPS) <= plane_elems(BN_FIR_MAX_TAPS), "whole 16-byte reads; the live part fits");

// bf16 elements of the packed operand: [step][plane][lane][8], lane (i = lane & 15, g = lane >> 4) holding A[i][32 s + 8 g + e]
constexpr size_t image_elems(uint32_t n_taps) { return (size_t)steps(n_taps) * 3 * 64 * 8; }

// null / count / non-finite refusals of a tap list
inline bn_status check_taps(const float *taps, size_t n_taps) {
    if (!taps) return set_last_error(BN_ERR_INVALID_ARG, "null taps");
    if (!count_ok(n_taps)) return refuse_count(n_taps);
    for (size_t t = 0; t < n_taps; t++)
        if (!std::isfinite(taps[t])) return set_last_error(BN_ERR_INVALID_ARG, "tap " + std::to_string(t) + " is not finite");
    return BN_OK;
}

// The Toeplitz operand of checked taps, split into three bf16 planes on the host (plan_rules.h, split_bf16x3), in the order in which
// the matrix instruction's A fragment wants it: the kernel issues one 16-byte load per lane, plane and step and no split at all
inline std::vector<uint16_t> pack_taps(const float *taps, uint32_t n_taps) {
    const uint32_t S = steps(n_taps);
    std::vector<uint16_t> img(image_elems(n_taps), 0);
    for (uint32_t s = 0; s < S; s++)
        for (uint32_t lane = 0; lane < 64; lane++)
            for (uint32_t e = 0; e < 8; e++) {
                const uint32_t j = lane & 15, k = 32 * s + 8 * (lane >> 4) + e;
                const int64_t t = (int64_t)j + n_taps - 1 - k;
                if (t < 0 || t >= (int64_t)n_taps) continue;
                uint16_t pl[3];
                split_bf16x3(taps[t], pl[0], pl[1], pl[2]);
                for (uint32_t p = 0; p < 3; p++) img[(((size_t)s * 3 + p) * 64 + lane) * 8 + e] = pl[p];
            }
    return img;
}

// bn_fir_bandpass: the linear-phase windowed-sinc design of include/birdnet_hip.h, in double, rounded to f32 once
inline bn_status bandpass(uint32_t rate, double lo_hz, double hi_hz, size_t n_taps, float *out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null taps output");
    if (!count_ok(n_taps)) return refuse_count(n_taps);
    if (rate == 0) return set_last_error(BN_ERR_INVALID_ARG, "sample_rate must be positive");
    const double nyq = 0.5 * (double)rate;
    if (!(lo_hz < hi_hz)) return set_last_error(BN_ERR_INVALID_ARG, "lo_hz must be below hi_hz");
    if (lo_hz >= nyq) return set_last_error(BN_ERR_INVALID_ARG, "lo_hz must be below half the sample rate");
    if (hi_hz <= 0.0) return set_last_error(BN_ERR_INVALID_ARG, "hi_hz must be positive");
    const double pi = 3.14159265358979323846;
    const double lo = lo_hz > 0.0 ? lo_hz : 0.0, hi = hi_hz < nyq ? hi_hz : nyq;
    const double f1 = lo / (double)rate, f2 = hi_hz < nyq ? hi / (double)rate : 0.5, fc = 0.5 * (lo + hi) / (double)rate;
    const double half = 0.5 * (double)(n_taps - 1), i0b = bessel_i0(KAISER_BETA);
    auto lowpass = [&](double f, double tau) {  // 2 f sinc(2 f tau)
        const double x = 2.0 * f * tau;
        return x == 0.0 ? 2.0 * f : 2.0 * f * (std::sin(pi * x) / (pi * x));
    };
    std::vector<double> h(n_taps);
    double gain = 0.0;
    for (size_t t = 0; t < n_taps; t++) {
        const double tau = (double)t - half, u = half > 0.0 ? tau / half : 0.0;
        const double w = bessel_i0(KAISER_BETA * std::sqrt(std::fmax(0.0, 1.0 - u * u))) / i0b;
        // the second half mirrors the first: symmetric bit for bit, whatever the math library does with a negative argument
        h[t] = 2 * t > n_taps - 1 ? h[n_taps - 1 - t] : (lowpass(f2, tau) - lowpass(f1, tau)) * w;
        gain += h[t] * std::cos(2.0 * pi * fc * std::fabs(tau));  // the response at the centre of the pass band
    }
    for (size_t t = 0; t < n_taps; t++) out[t] = (float)(h[t] / gain);
    return BN_OK;
}

}  // namespace fir
}  // namespace bn
