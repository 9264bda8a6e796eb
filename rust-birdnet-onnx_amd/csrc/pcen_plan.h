// The host-side arithmetic of PCEN spectrograms (recording.cpp: bn_recording_pcen, bn_pcen_thresholds; kernels in pcen.hip) that
// needs neither a device nor the runtime: a spec checked and copied, the bytes of the output without a product that can wrap, the
// launch pieces as whole chunks, a chunk's first frame and length, the powers a^n of the carry and the threshold table.
// Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_pcen_plan.cpp).
//
// THE SCAN.  M[t] = a M[t-1] + s x[t] is linear, so over a chunk of frames it is M_end = a^n M_start + S, where S is the same
// recurrence run from 0 and n counts the chunk's finite frames (a non-finite one leaves M alone).  Chunks are CHUNK consecutive
// frames counted from frame 0 of the call: which chunk a frame lies in, and so every bit of its result, depends on its position
// in the call alone, not on the launch pieces.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "spectrogram_plan.h"

namespace bn {
namespace pcen {

constexpr uint32_t CHUNK = 128;      // frames of one chunk ("PCEN")
constexpr uint32_t WAVE_ROWS = 64;   // rows of one wave: a lane owns a row
constexpr uint32_t LANES = 256, WAVES = LANES / 64;
constexpr uint32_t AHEAD = 8;        // frames whose loads are issued ahead of the dependent chain
constexpr uint32_t N_THR = spectro::N_THR;
static_assert(CHUNK % AHEAD == 0, "a full chunk is whole groups of loads");

// a checked spec with what follows from it
struct Plan {
    uint32_t format = 0, elem = 0;  // bytes per element
    float s = 0.0f, a = 0.0f;       // a = 1 - s, rounded once
    float gain = 0.0f, alpha = 0.0f, delta = 0.0f, r = 0.0f, eps = 0.0f, max_value = 0.0f;
};

// the plan of a spec, read through memcpy
inline bn_status check_spec(const bn_pcen_spec *spec, size_t spec_size, Plan *out) {
    if (!spec) return set_last_error(BN_ERR_INVALID_ARG, "null PCEN spec");
    if (spec_size < sizeof(bn_pcen_spec)) return set_last_error(BN_ERR_INVALID_ARG, "pcen_size is below sizeof(bn_pcen_spec)");
    bn_pcen_spec p;
    memcpy(&p, spec, sizeof(p));
    if (p.format != BN_PCEN_F32 && p.format != BN_PCEN_U8) return set_last_error(BN_ERR_INVALID_ARG, "unknown PCEN format " + std::to_string(p.format));
    if (!(p.smooth > 0.0f && p.smooth <= 1.0f)) return set_last_error(BN_ERR_INVALID_ARG, "smooth must lie in (0, 1]");
    if (!(p.gain > 0.0f) || !std::isfinite(p.gain)) return set_last_error(BN_ERR_INVALID_ARG, "gain must be positive and finite");
    if (!(p.alpha >= 0.0f && p.alpha <= 1.0f)) return set_last_error(BN_ERR_INVALID_ARG, "alpha must lie in [0, 1]");
    if (!(p.delta >= 0.0f) || !std::isfinite(p.delta)) return set_last_error(BN_ERR_INVALID_ARG, "delta must be at least 0 and finite");
    if (!(p.r > 0.0f && p.r <= 1.0f)) return set_last_error(BN_ERR_INVALID_ARG, "r must lie in (0, 1]");
    if (!(p.eps > 0.0f) || !std::isfinite(p.eps)) return set_last_error(BN_ERR_INVALID_ARG, "eps must be positive and finite");
    if (p.format == BN_PCEN_U8 && (!(p.max_value > 0.0f) || !std::isfinite(p.max_value)))
        return set_last_error(BN_ERR_INVALID_ARG, "max_value must be positive and finite");
    *out = Plan{};
    out->format = p.format, out->elem = p.format == BN_PCEN_U8 ? 1u : (uint32_t)sizeof(float);
    out->s = p.smooth, out->a = (float)(1.0 - (double)p.smooth);
    out->gain = p.gain, out->alpha = p.alpha, out->delta = p.delta, out->r = p.r, out->eps = p.eps, out->max_value = p.max_value;
    return BN_OK;
}

// n_frames * n_rows * elem, the bytes of the output; false if that is no size_t
inline bool out_bytes(size_t n_frames, uint32_t n_rows, uint32_t elem, size_t *out) { return spectro::out_bytes(n_frames, n_rows, elem, out); }

// frames per launch: whole chunks, at most `limit` frames (spectro::piece_frames(n_rows) in the library), at least one chunk
constexpr size_t piece_frames(size_t limit) { return limit / CHUNK ? limit / CHUNK * CHUNK : CHUNK; }
static_assert(piece_frames(spectro::piece_frames(1025)) == 65408 && piece_frames(spectro::piece_frames(1025)) <= spectro::piece_frames(1025) &&
                  piece_frames(spectro::piece_frames(1)) == (size_t)1 << 24,
              "a piece is one launch of the spectrogram");

// chunks of n frames, the last one partial; the frames of chunk c of them
constexpr size_t chunks(size_t n_frames) { return n_frames / CHUNK + (n_frames % CHUNK ? 1 : 0); }
constexpr uint32_t chunk_len(size_t n_frames, size_t c) { return (uint32_t)(n_frames - c * CHUNK < CHUNK ? n_frames - c * CHUNK : CHUNK); }
// waves of a launch: a wave owns one chunk and WAVE_ROWS consecutive rows
constexpr uint32_t row_blocks(uint32_t n_rows) { return (n_rows + WAVE_ROWS - 1) / WAVE_ROWS; }

// apow[n] = a^n, n = 0 .. CHUNK, with a = 1 - s in double, each rounded once: not a running product.  0^0 is 1
inline void apow(float s, float *out /* CHUNK + 1 */) {
    const double a = 1.0 - (double)s;
    for (uint32_t n = 0; n <= CHUNK; n++) out[n] = (float)std::pow(a, (double)n);
}

// bn_pcen_thresholds: thr[j - 1] = (j - 0.5) * max_value / 255, j = 1 .. 255, in double, rounded once, forced non-decreasing
inline bn_status thresholds(float max_value, float *thr) {
    if (!thr) return set_last_error(BN_ERR_INVALID_ARG, "null thresholds output");
    if (!(max_value > 0.0f) || !std::isfinite(max_value)) return set_last_error(BN_ERR_INVALID_ARG, "max_value must be positive and finite");
    float prev = 0.0f;
    for (uint32_t j = 1; j <= N_THR; j++) {
        float v = (float)(((double)j - 0.5) * (double)max_value / 255.0);
        if (v < prev) v = prev;
        thr[j - 1] = prev = v;
    }
    return BN_OK;
}

}  // namespace pcen
}  // namespace bn
