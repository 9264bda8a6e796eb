// The host-side arithmetic of template matching (recording.cpp: bn_templates_create, bn_recording_template_match,
// bn_template_peaks; kernel in template.hip) that needs neither a device nor the runtime: a set's refusals, the packer that lays
// the templates out as the matrix instruction's A operand, each template's K, T1 and dT, the LDS a workgroup takes, the launch
// pieces of a call and their overlap without a product or sum that can wrap, and the peaks helper.  Host code only, so that a
// stand-alone program can run it under a sanitizer (tools/asan_template_plan.cpp).
//
// THE PRODUCT.  A[q][t] = sum_{w, j} tau_q[w][j] s[t + w][j] is a Toeplitz product: 16 templates x 16 offsets per accumulator on
// v_mfma_i32_16x16x64_i8.  K is ordered (frame w, then row j) in UNITS of 16 rows: a frame is U = ceil(R / 16) units, unit
// u = w U + j / 16, a K step is four units, and the rows R .. 16 U - 1 of a frame are zeros on both sides.  A tile of 16 templates
// runs to the step count of its longest member; a shorter member is zeros behind its own W_q U units.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "last_error.h"
#include "spectrogram_plan.h"

namespace bn {
namespace tmatch {

constexpr uint32_t LANES = 256, WAVES = LANES / 64;
constexpr uint32_t TILE_OFFSETS = 64;  // a workgroup's offsets: 16 per wave, one column block of the matrix instruction
constexpr uint32_t TILE_TEMPLATES = 16;
constexpr uint32_t MAX_TILES = BN_TEMPLATE_MAX_COUNT / TILE_TEMPLATES;
constexpr uint32_t UNIT = 16, STEP_UNITS = 4;  // bytes of a unit (one lane's operand), units of a K step
constexpr uint32_t STEP_BYTES = 64 * UNIT;     // a tile's A fragment of one step: 64 lanes x 16 bytes
static_assert(BN_TEMPLATE_MAX_COUNT % TILE_TEMPLATES == 0 && MAX_TILES == 4, "a wave keeps one accumulator per tile, at most four");
// the caps keep every i32 sum below 2^31: |A| and S2 <= 65536 * 128 * 128 = 2^30
static_assert((uint64_t)BN_TEMPLATE_MAX_ELEMS * 128 * 128 == (uint64_t)1 << 30 && BN_TEMPLATE_MAX_FRAMES * BN_TEMPLATE_MAX_ROWS == BN_TEMPLATE_MAX_ELEMS, "the caps");

constexpr uint32_t units(uint32_t n_rows) { return (n_rows + UNIT - 1) / UNIT; }
constexpr uint32_t steps(uint32_t frames, uint32_t n_rows) { return (frames * units(n_rows) + STEP_UNITS - 1) / STEP_UNITS; }

// ---- LDS.  The code image of a tile, bit 7 flipped: LDS_ROWS frame rows `stride` bytes apart, then the exclusive prefixes of the
// rows' sum s and sum s^2 over the tile's 63 + Wmax frames.  A row is 16 U bytes and the stride's padding, so that it is 32 bytes
// mod 64 long and the sixteen lanes of a b128 group fall on sixteen different 16-byte slots (template.hip).  The last step of a tile
// may read up to three units past the longest template (where A is zeros): three spare rows keep those reads inside the image
constexpr uint32_t SPARE_ROWS = 3;
constexpr uint32_t sum_rows(uint32_t wmax) { return TILE_OFFSETS + wmax - 1; }
constexpr uint32_t lds_rows(uint32_t wmax) { return sum_rows(wmax) + SPARE_ROWS; }
constexpr uint32_t stride(uint32_t n_rows) { return UNIT * units(n_rows) + (32u + 64u - UNIT * units(n_rows) % 64u) % 64u; }
constexpr uint32_t PREFIX_ROWS = 192;  // sum_rows(128) + 1 entries of each prefix
constexpr uint32_t PREFIX_BYTES = 2 * PREFIX_ROWS * (uint32_t)sizeof(uint32_t);
// the scores of a tile leave through the image's bytes, [templates][SCORE_LD] floats, once every wave has read its last fragment
constexpr uint32_t SCORE_LD = TILE_OFFSETS + 4;  // the four template groups of an accumulator's lanes write 16 banks apart
constexpr uint32_t score_bytes(uint32_t n_tiles) { return n_tiles * TILE_TEMPLATES * SCORE_LD * (uint32_t)sizeof(float); }
constexpr uint32_t lds_bytes(uint32_t wmax, uint32_t n_rows, uint32_t n_tiles) {
    return PREFIX_BYTES + (lds_rows(wmax) * stride(n_rows) > score_bytes(n_tiles) ? lds_rows(wmax) * stride(n_rows) : score_bytes(n_tiles));
}
static_assert(stride(512) == 544 && stride(1) == 32 && stride(17) == 32 && stride(80) == 96 && stride(48) == 96 && stride(64) == 96, "32 bytes mod 64");
static_assert(sum_rows(BN_TEMPLATE_MAX_FRAMES) + 1 == PREFIX_ROWS && PREFIX_ROWS == 3 * 64, "the prefix is three rows per lane of one wave");
constexpr uint32_t MAX_LDS_BYTES = lds_bytes(BN_TEMPLATE_MAX_FRAMES, BN_TEMPLATE_MAX_ROWS, MAX_TILES);
static_assert(MAX_LDS_BYTES == 194 * 544 + 1536 && MAX_LDS_BYTES <= 160 * 1024 && lds_bytes(1, 1, 4) == 1536 + 17408, "the worst case fits with the opt-in");

// The B operand's walk: the LDS byte address of unit 4 sigma + g of the offset whose first frame is LDS row `row`, sigma = 0, 1, ...
// Four units on are q4 whole frames and r4 units, r4 < U, so one conditional wrap per step and no division (the kernel's loop and
// tools/asan_template_plan.cpp run this one struct)
struct UnitWalk {
    uint32_t ju, addr, r4, inc, wrap, U;
    constexpr UnitWalk(uint32_t row, uint32_t g, uint32_t U_, uint32_t stride_)
        : ju(g % U_), addr((row + g / U_) * stride_ + (g % U_) * UNIT), r4(4 % U_), inc((4 / U_) * stride_ + (4 % U_) * UNIT), wrap(stride_ - U_ * UNIT), U(U_) {}
    constexpr void next() {
        ju += r4, addr += inc;
        if (ju >= U) ju -= U, addr += wrap;
    }
};

// what the kernel needs of one template
struct Meta {
    uint32_t frames;  // W_q
    uint32_t K;       // W_q * R
    int32_t T1;       // sum tau
    uint32_t pad;
    int64_t dT;       // K * T2 - T1^2 > 0
};
// per tile: its step count and where its fragments start in the image, in steps
struct Tiles {
    uint32_t count[MAX_TILES], offset[MAX_TILES];
};
struct Packed {
    uint32_t n_templates = 0, n_rows = 0, n_tiles = 0, max_frames = 0;
    Tiles tiles{};
    std::vector<Meta> meta;      // [16 * n_tiles]; a slot past n_templates is zeros
    std::vector<uint8_t> image;  // [step of the image][lane][16]: lane (i = lane & 15, g = lane >> 4) of tile j, step s, holds
                                 // tau of template 16 j + i, unit 4 s + g
};

// The byte a lane holds: template q's tau (as the int8's byte) at K position (unit u, e), 0 outside the template
inline uint8_t operand_byte(const uint8_t *codes_q, uint32_t frames, uint32_t n_rows, uint32_t u, uint32_t e) {
    const uint32_t U = units(n_rows), w = u / U, j = (u - w * U) * UNIT + e;
    if (w >= frames || j >= n_rows) return 0;
    return (uint8_t)(codes_q[(size_t)w * n_rows + j] ^ 0x80u);
}

// bn_templates_create's refusals, then the packed set
inline bn_status pack(size_t n_templates, size_t n_rows, const uint32_t *n_frames, const uint8_t *codes, Packed *out) {
    if (!n_frames || !codes || !out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (n_templates == 0 || n_templates > BN_TEMPLATE_MAX_COUNT)
        return set_last_error(BN_ERR_INVALID_ARG, "n_templates " + std::to_string(n_templates) + " is not in 1.." + std::to_string(BN_TEMPLATE_MAX_COUNT));
    if (n_rows == 0 || n_rows > BN_TEMPLATE_MAX_ROWS)
        return set_last_error(BN_ERR_INVALID_ARG, "n_rows " + std::to_string(n_rows) + " is not in 1.." + std::to_string(BN_TEMPLATE_MAX_ROWS));
    Packed p;
    p.n_templates = (uint32_t)n_templates, p.n_rows = (uint32_t)n_rows, p.n_tiles = (uint32_t)((n_templates + TILE_TEMPLATES - 1) / TILE_TEMPLATES);
    p.meta.assign((size_t)p.n_tiles * TILE_TEMPLATES, Meta{});
    std::vector<size_t> at(n_templates);
    size_t pos = 0;
    for (size_t q = 0; q < n_templates; q++) {
        const uint32_t W = n_frames[q];
        if (W == 0 || W > BN_TEMPLATE_MAX_FRAMES)
            return set_last_error(BN_ERR_INVALID_ARG, "template " + std::to_string(q) + " has " + std::to_string(W) + " frames, not 1.." + std::to_string(BN_TEMPLATE_MAX_FRAMES));
        const uint64_t K = (uint64_t)W * n_rows;
        if (K > BN_TEMPLATE_MAX_ELEMS)
            return set_last_error(BN_ERR_INVALID_ARG, "template " + std::to_string(q) + " has " + std::to_string(K) + " elements, above " + std::to_string(BN_TEMPLATE_MAX_ELEMS));
        int64_t T1 = 0, T2 = 0;
        for (uint64_t e = 0; e < K; e++) {
            const int64_t v = (int64_t)codes[pos + e] - 128;
            T1 += v, T2 += v * v;
        }
        const int64_t dT = (int64_t)K * T2 - T1 * T1;  // <= 2^16 * 2^30
        if (dT == 0) return set_last_error(BN_ERR_INVALID_ARG, "template " + std::to_string(q) + " is flat: every code is the same, it correlates with nothing");
        p.meta[q] = Meta{W, (uint32_t)K, (int32_t)T1, 0, dT};
        at[q] = pos, pos += (size_t)K;
        p.max_frames = W > p.max_frames ? W : p.max_frames;
    }
    uint32_t off = 0;
    for (uint32_t j = 0; j < p.n_tiles; j++) {
        uint32_t longest = 0;
        for (size_t q = (size_t)j * TILE_TEMPLATES; q < n_templates && q < (size_t)(j + 1) * TILE_TEMPLATES; q++) longest = n_frames[q] > longest ? n_frames[q] : longest;
        p.tiles.count[j] = steps(longest, p.n_rows), p.tiles.offset[j] = off;
        off += p.tiles.count[j];
    }
    p.image.assign((size_t)off * STEP_BYTES, 0);
    for (uint32_t j = 0; j < p.n_tiles; j++)
        for (uint32_t s = 0; s < p.tiles.count[j]; s++)
            for (uint32_t lane = 0; lane < 64; lane++) {
                const size_t q = (size_t)j * TILE_TEMPLATES + (lane & 15);
                if (q >= n_templates) continue;
                uint8_t *dst = &p.image[((size_t)(p.tiles.offset[j] + s) * 64 + lane) * UNIT];
                for (uint32_t e = 0; e < UNIT; e++) dst[e] = operand_byte(codes + at[q], n_frames[q], p.n_rows, STEP_UNITS * s + (lane >> 4), e);
            }
    *out = std::move(p);
    return BN_OK;
}

// ---- a call and its launch pieces
// n_templates * n_offsets, the floats of the output; false if that is no size_t
inline bool out_floats(size_t n_templates, size_t n_offsets, size_t *out) {
    if (n_templates == 0 || n_offsets > SIZE_MAX / n_templates) return false;
    *out = n_templates * n_offsets;
    return true;
}
// n_offsets + wmax - 1, the frames of the image a call reads; false if that is no size_t
inline bool image_frames(size_t n_offsets, uint32_t wmax, size_t *out) {
    if (wmax == 0 || n_offsets > SIZE_MAX - (wmax - 1)) return false;
    *out = n_offsets + (wmax - 1);
    return true;
}
// consecutive pieces re-make the wmax - 1 frames they share
constexpr uint32_t piece_overlap(uint32_t wmax) { return wmax - 1; }
// Offsets per launch piece: whole tiles; the piece's image, offsets + wmax - 1 frames, is one launch of the spectrogram (at most
// 2^26 bytes, spectro::piece_frames) and its scores are at most 2^26 floats
constexpr size_t piece_offsets(uint32_t n_rows, uint32_t wmax, uint32_t n_templates) {
    const size_t by_image = spectro::piece_frames(n_rows) - piece_overlap(wmax), by_scores = ((size_t)1 << 26) / (n_templates ? n_templates : 1);
    return (by_image < by_scores ? by_image : by_scores) & ~(size_t)(TILE_OFFSETS - 1);
}
static_assert(piece_offsets(512, 128, 64) == 130944 && piece_offsets(1, 1, 64) == (size_t)1 << 20 && piece_offsets(1025, 128, 1) >= TILE_OFFSETS, "whole tiles, never none");

// ---- bn_template_peaks
struct Hit {
    uint64_t offset;
    uint32_t template_index;
    float score;
};
// u comes after t in the order "score descending, ties by offset ascending"; a NaN at u never suppresses
inline bool comes_after(float st, size_t t, float su, size_t u) { return su != su || su < st || (su == st && u > t); }

inline bn_status peaks(const float *scores, size_t n_templates, size_t n_offsets, float min_score, size_t radius, void *out, size_t cap, size_t struct_size,
                       size_t *n_out) {
    if (!n_out || (!scores && n_templates && n_offsets) || (!out && cap)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (struct_size < sizeof(Hit)) return set_last_error(BN_ERR_INVALID_ARG, "struct_size is below sizeof(bn_template_hit)");
    if (min_score != min_score) return set_last_error(BN_ERR_INVALID_ARG, "min_score is NaN");
    size_t n = 0;
    for (size_t q = 0; q < n_templates; q++) {
        const float *s = scores + q * n_offsets;
        for (size_t t = 0; t < n_offsets; t++) {
            if (!(s[t] >= min_score)) continue;  // a NaN is never a hit
            const size_t lo = t > radius ? t - radius : 0, hi = n_offsets - 1 - t > radius ? t + radius : n_offsets - 1;
            bool peak = true;
            for (size_t u = lo; u <= hi && peak; u++) peak = u == t || comes_after(s[t], t, s[u], u);
            if (!peak) continue;
            if (n < cap) {
                const Hit h{(uint64_t)t, (uint32_t)q, s[t]};
                memcpy(static_cast<char *>(out) + n * struct_size, &h, sizeof(h));
            }
            n++;
        }
    }
    *n_out = n;
    return BN_OK;
}

}  // namespace tmatch
}  // namespace bn
