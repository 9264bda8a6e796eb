// The host-side arithmetic of spectrograms (recording.cpp: bn_recording_spectrogram, bn_filterbank_create, bn_mel_filterbank,
// bn_spectrogram_thresholds; kernels in spectrogram.hip) that needs neither a device nor the runtime: a spec checked and copied,
// the rows and the bytes of the output without a product that can wrap, the last sample a range reads and where a launch piece
// starts (no sum that can wrap), the frames of a piece, the LDS a workgroup takes and its strides, the packer that lays a bank
// out as the matrix instruction's A operand with the K steps each row tile needs, the mel designer and the threshold table.
// Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_spectrogram_plan.cpp).
//
// THE PRODUCT.  A tile is 16 bank rows x 16 frames: E[m][t] = sum_k A[m][k] B[k][t], A = W (the bank), B[k][t] = P[t,k], K = N/2 + 1
// bins padded with zeros to a multiple of the instruction's 32.  Row tile j covers rows [16 j, 16 j + 16) (rows past n_rows are
// zeros) and only the steps [first, first + count) between its first and last non-zero column are packed and multiplied: a zero
// step adds +0.0f products to a non-negative accumulator, which changes no bit, so skipping is exact.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "band_plan.h"
#include "plan_rules.h"

namespace bn {
namespace spectro {

constexpr uint32_t LANES = 256, WAVES = LANES / 64;
constexpr uint32_t TILE_FRAMES = 16;  // a workgroup's frames: one column block of the matrix instruction
constexpr uint32_t TILE_ROWS = 16;    // bank rows of one accumulator
constexpr uint32_t MAX_ROW_TILES = BN_FILTERBANK_MAX_ROWS / TILE_ROWS;
constexpr uint32_t N_THR = 255;  // thresholds of the U8 codes
static_assert(BN_FILTERBANK_MAX_ROWS % TILE_ROWS == 0 && MAX_ROW_TILES == 16, "the tile table is a kernel argument of 16 entries");

// a checked spec with what follows from it and the bank
struct Plan {
    uint32_t N = 0, hop = 0, lo = 0, hi = 0;  // lo == hi == 0 with a bank
    uint32_t n_rows = 0;
    uint32_t format = 0, elem = 0;  // bytes per element
    bool bank = false;
    float ref_power = 0.0f, range_db = 0.0f;
};

// The plan of (spec, bank).  bank_rows == 0: no bank; else the bank's rows and frame.  The spec is read through memcpy
inline bn_status check_spec(const bn_spectrogram_spec *spec, size_t spec_size, size_t bank_rows, uint32_t bank_frame, Plan *out) {
    if (!spec) return set_last_error(BN_ERR_INVALID_ARG, "null spectrogram spec");
    if (spec_size < sizeof(bn_spectrogram_spec)) return set_last_error(BN_ERR_INVALID_ARG, "spec_size is below sizeof(bn_spectrogram_spec)");
    bn_spectrogram_spec s;
    memcpy(&s, spec, sizeof(s));
    if (!band::frame_ok(s.frame)) return set_last_error(BN_ERR_INVALID_ARG, "frame " + std::to_string(s.frame) + " is not 256, 512, 1024 or 2048");
    if (s.hop == 0 || s.hop > s.frame) return set_last_error(BN_ERR_INVALID_ARG, "hop " + std::to_string(s.hop) + " is not in 1.." + std::to_string(s.frame));
    if (s.format != BN_SPECTROGRAM_F32 && s.format != BN_SPECTROGRAM_U8) return set_last_error(BN_ERR_INVALID_ARG, "unknown spectrogram format " + std::to_string(s.format));
    *out = Plan{};
    if (bank_rows) {
        if (s.bin_lo != 0 || s.bin_hi != 0) return set_last_error(BN_ERR_INVALID_ARG, "with a filter bank bin_lo and bin_hi must both be 0");
        if (bank_frame != s.frame)
            return set_last_error(BN_ERR_INVALID_ARG, "the filter bank is of frame " + std::to_string(bank_frame) + ", the spec of frame " + std::to_string(s.frame));
        out->n_rows = (uint32_t)bank_rows, out->bank = true;
    } else {
        if (s.bin_lo >= s.bin_hi || s.bin_hi > s.frame / 2 + 1)
            return set_last_error(BN_ERR_INVALID_ARG, "bins [" + std::to_string(s.bin_lo) + ", " + std::to_string(s.bin_hi) + ") are empty or reach past bin " +
                                                          std::to_string(s.frame / 2));
        out->lo = s.bin_lo, out->hi = s.bin_hi, out->n_rows = s.bin_hi - s.bin_lo;
    }
    if (s.format == BN_SPECTROGRAM_U8) {
        if (!(s.ref_power > 0.0f) || !std::isfinite(s.ref_power)) return set_last_error(BN_ERR_INVALID_ARG, "ref_power must be positive and finite");
        if (!(s.range_db > 0.0f) || !std::isfinite(s.range_db)) return set_last_error(BN_ERR_INVALID_ARG, "range_db must be positive and finite");
    }
    out->N = s.frame, out->hop = s.hop, out->format = s.format, out->elem = s.format == BN_SPECTROGRAM_U8 ? 1u : (uint32_t)sizeof(float);
    out->ref_power = s.ref_power, out->range_db = s.range_db;
    return BN_OK;
}

// n_frames * n_rows * elem, the bytes of the output; false if that is no size_t
inline bool out_bytes(size_t n_frames, uint32_t n_rows, uint32_t elem, size_t *out) {
    const size_t per = (size_t)n_rows * elem;  // <= 1025 * 4
    if (per == 0 || n_frames > SIZE_MAX / per) return false;
    *out = n_frames * per;
    return true;
}

// The sample at which frame `t` of a range that starts at `first` <= n begins, saturated at n (the recording's samples): a frame
// that starts at or past n reads zeros wherever it starts, and so does every frame after it.  first + t * hop is not formed where
// it could wrap
inline uint64_t frame_start(uint64_t n, uint64_t first, uint64_t t, uint32_t hop) {
    const uint64_t room = n - first;  // first <= n
    if (t > room / hop) return n;     // t * hop > room
    return first + t * hop;
}

// The last sample of a recording of n samples that frames [0, n_frames) of N samples every hop from `first` <= n read; false if
// they read none (n_frames == 0 or first == n)
inline bool last_sample_read(uint64_t n, uint64_t first, uint64_t n_frames, uint32_t N, uint32_t hop, uint64_t *out) {
    if (n_frames == 0 || first >= n) return false;
    const uint64_t start = frame_start(n, first, n_frames - 1, hop);  // <= n
    *out = n - start > N ? start + N - 1 : n - 1;
    return true;
}

// frames per launch: whole tiles, an output of at most 2^26 elements on the device, at most 2^20 workgroups
constexpr size_t piece_frames(uint32_t n_rows) {
    const size_t by_out = (((size_t)1 << 26) / (n_rows ? n_rows : 1)) & ~(size_t)(TILE_FRAMES - 1);
    return by_out < ((size_t)1 << 24) ? by_out : ((size_t)1 << 24);
}
static_assert(piece_frames(1025) >= TILE_FRAMES && piece_frames(1025) % TILE_FRAMES == 0 && piece_frames(1) == (size_t)1 << 24, "whole tiles");

// ---- LDS.  Both kernels: the thresholds (256 floats, the last unused) and a flag per frame of the tile, then the frames' rows
constexpr uint32_t HEAD_BYTES = (N_THR + 1 + TILE_FRAMES) * (uint32_t)sizeof(float);
// bins: f32 rows of N/2 + 1 powers, each swizzled as the profile's (profile::lds_index; a wave stores into one row at a time)
constexpr uint32_t bins_row(uint32_t N) { return N / 2 + 1; }
constexpr uint32_t bins_lds_bytes(uint32_t N) { return HEAD_BYTES + TILE_FRAMES * bins_row(N) * (uint32_t)sizeof(float); }
constexpr uint32_t lds_index(uint32_t N, uint32_t k) { return k ^ ((k >> 5) & (N / 64 - 1)); }
// bank: three bf16 planes [frame][stride]; depth() bins are read, the rest of a row is the stride's padding: 16 elements, so that
// a row is 32 bytes mod 64 long and the sixteen lanes of a b128 group fall on sixteen different 16-byte slots (spectrogram.hip)
constexpr uint32_t depth(uint32_t N) { return (N / 2 + 1 + 31) & ~31u; }  // K padded
constexpr uint32_t steps(uint32_t N) { return depth(N) / 32; }
constexpr uint32_t bank_stride(uint32_t N) { return depth(N) + 16; }  // bf16 elements
constexpr uint32_t bank_lds_bytes(uint32_t N) { return HEAD_BYTES + 3 * TILE_FRAMES * bank_stride(N) * (uint32_t)sizeof(uint16_t); }
static_assert(bank_stride(256) * 2 % 64 == 32 && bank_stride(2048) * 2 % 64 == 32 && bank_stride(256) % 8 == 0, "the stride the bank-conflict argument needs");
static_assert(bank_lds_bytes(256) == 17984 && bank_lds_bytes(512) == 30272 && bank_lds_bytes(1024) == 54848 && bank_lds_bytes(2048) == 104000,
              "the figures the documents name");
static_assert(bins_lds_bytes(2048) == 66688 && bins_lds_bytes(1024) == 33920 && bank_lds_bytes(2048) <= 160 * 1024, "frame 2048 needs the opt-in in both kernels");

// ---- the packed bank
// per row tile: the first K step it multiplies, how many, and where its fragments start in the image, in steps (3 KiB each)
struct BankTiles {
    uint32_t first[MAX_ROW_TILES], count[MAX_ROW_TILES], offset[MAX_ROW_TILES];
};
struct PackedBank {
    uint32_t n_tiles = 0;
    BankTiles tiles{};
    std::vector<uint16_t> image;  // [step of the image][plane][lane][8]: lane (i = lane & 15, g = lane >> 4) holds W[16 j + i][32 s + 8 g + e]
};
constexpr size_t STEP_ELEMS = 3 * 64 * 8;

inline bn_status check_bank(uint32_t frame, size_t n_rows, const float *w) {
    if (!w) return set_last_error(BN_ERR_INVALID_ARG, "null filter bank weights");
    if (n_rows == 0 || n_rows > BN_FILTERBANK_MAX_ROWS)
        return set_last_error(BN_ERR_INVALID_ARG, "n_rows " + std::to_string(n_rows) + " is not in 1.." + std::to_string(BN_FILTERBANK_MAX_ROWS));
    if (!band::frame_ok(frame)) return set_last_error(BN_ERR_INVALID_ARG, "frame " + std::to_string(frame) + " is not 256, 512, 1024 or 2048");
    const size_t K = frame / 2 + 1;
    for (size_t m = 0; m < n_rows; m++) {
        bool any = false;
        for (size_t k = 0; k < K; k++) {
            const float v = w[m * K + k];
            if (!std::isfinite(v) || v < 0.0f)
                return set_last_error(BN_ERR_INVALID_ARG, "weight (" + std::to_string(m) + ", " + std::to_string(k) + ") is negative or not finite");
            any |= v > 0.0f;
        }
        if (!any) return set_last_error(BN_ERR_INVALID_ARG, "row " + std::to_string(m) + " of the filter bank is all zeros");
    }
    return BN_OK;
}

// the A operand of a checked bank, split into three bf16 planes on the host (plan_rules.h, split_bf16x3) in fragment order
inline PackedBank pack_bank(uint32_t frame, size_t n_rows, const float *w) {
    const size_t K = frame / 2 + 1;
    PackedBank b;
    b.n_tiles = (uint32_t)((n_rows + TILE_ROWS - 1) / TILE_ROWS);
    uint32_t at = 0;
    for (uint32_t j = 0; j < b.n_tiles; j++) {
        size_t k0 = K, k1 = 0;  // the tile's first and last non-zero column (a checked bank has one in every row)
        for (size_t m = (size_t)j * TILE_ROWS; m < n_rows && m < (size_t)(j + 1) * TILE_ROWS; m++)
            for (size_t k = 0; k < K; k++)
                if (w[m * K + k] > 0.0f) k0 = k < k0 ? k : k0, k1 = k > k1 ? k : k1;
        b.tiles.first[j] = (uint32_t)(k0 / 32), b.tiles.count[j] = (uint32_t)(k1 / 32 - k0 / 32 + 1), b.tiles.offset[j] = at;
        at += b.tiles.count[j];
    }
    b.image.assign((size_t)at * STEP_ELEMS, 0);
    for (uint32_t j = 0; j < b.n_tiles; j++)
        for (uint32_t s = 0; s < b.tiles.count[j]; s++)
            for (uint32_t lane = 0; lane < 64; lane++)
                for (uint32_t e = 0; e < 8; e++) {
                    const size_t m = (size_t)j * TILE_ROWS + (lane & 15), k = 32 * (size_t)(b.tiles.first[j] + s) + 8 * (lane >> 4) + e;
                    if (m >= n_rows || k >= K) continue;
                    uint16_t pl[3];
                    split_bf16x3(w[m * K + k], pl[0], pl[1], pl[2]);
                    for (uint32_t p = 0; p < 3; p++) b.image[(((size_t)(b.tiles.offset[j] + s) * 3 + p) * 64 + lane) * 8 + e] = pl[p];
                }
    return b;
}

// bn_mel_filterbank: HTK mel triangles at the bin centres, in double, rounded to f32 once
inline bn_status mel_bank(uint32_t rate, uint32_t frame, size_t n_mels, double fmin, double fmax, float *out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null weights output");
    if (rate == 0) return set_last_error(BN_ERR_INVALID_ARG, "sample_rate must be positive");
    if (!band::frame_ok(frame)) return set_last_error(BN_ERR_INVALID_ARG, "frame " + std::to_string(frame) + " is not 256, 512, 1024 or 2048");
    if (n_mels == 0 || n_mels > BN_FILTERBANK_MAX_ROWS)
        return set_last_error(BN_ERR_INVALID_ARG, "n_mels " + std::to_string(n_mels) + " is not in 1.." + std::to_string(BN_FILTERBANK_MAX_ROWS));
    if (!(fmin >= 0.0)) return set_last_error(BN_ERR_INVALID_ARG, "fmin_hz must be at least 0");
    if (!(fmin < fmax)) return set_last_error(BN_ERR_INVALID_ARG, "fmin_hz must be below fmax_hz");
    if (!(fmax <= 0.5 * (double)rate)) return set_last_error(BN_ERR_INVALID_ARG, "fmax_hz must not exceed half the sample rate");
    auto mel = [](double f) { return 2595.0 * std::log10(1.0 + f / 700.0); };
    auto hz = [](double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); };
    const double m0 = mel(fmin), m1 = mel(fmax);
    std::vector<double> pt(n_mels + 2);
    for (size_t i = 0; i < n_mels + 2; i++) pt[i] = hz(m0 + (m1 - m0) * (double)i / (double)(n_mels + 1));
    const size_t K = frame / 2 + 1;
    std::vector<float> w(n_mels * K, 0.0f);
    for (size_t m = 0; m < n_mels; m++) {
        const double a = pt[m], b = pt[m + 1], c = pt[m + 2];
        bool any = false;
        for (size_t k = 0; k < K; k++) {
            const double f = (double)k * (double)rate / (double)frame;
            const double v = f <= a || f >= c ? 0.0 : (f <= b ? (f - a) / (b - a) : (c - f) / (c - b));
            w[m * K + k] = (float)v;
            any |= w[m * K + k] > 0.0f;
        }
        if (!any) return set_last_error(BN_ERR_INVALID_ARG, "mel triangle " + std::to_string(m) + " holds no bin centre");
    }
    memcpy(out, w.data(), w.size() * sizeof(float));  // nothing written on a refusal
    return BN_OK;
}

// bn_spectrogram_thresholds: thr[j - 1], j = 1 .. 255, in double, rounded once, forced non-decreasing
inline bn_status thresholds(float ref_power, float range_db, float *thr) {
    if (!thr) return set_last_error(BN_ERR_INVALID_ARG, "null thresholds output");
    if (!(ref_power > 0.0f) || !std::isfinite(ref_power)) return set_last_error(BN_ERR_INVALID_ARG, "ref_power must be positive and finite");
    if (!(range_db > 0.0f) || !std::isfinite(range_db)) return set_last_error(BN_ERR_INVALID_ARG, "range_db must be positive and finite");
    float prev = 0.0f;
    for (uint32_t j = 1; j <= N_THR; j++) {
        const double db = ((double)j - 0.5) * (double)range_db / 255.0 - (double)range_db;
        float v = (float)((double)ref_power * std::pow(10.0, db / 10.0));
        if (v < prev) v = prev;
        thr[j - 1] = prev = v;
    }
    return BN_OK;
}

}  // namespace spectro
}  // namespace bn
