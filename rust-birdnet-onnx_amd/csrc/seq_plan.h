// The host-side arithmetic of the sequence search (seq.hip, bn_index_search_seq and its _ids form) that needs neither a device nor the
// runtime: the refusals of its arguments, how many sequences share the 64 query slots of a scan pass, how many passes and rounds a call
// takes, which tiles a workgroup computes beyond its own run, and the dynamic LDS of seq_scan_kernel beyond index_scan.h's Layout<2>.
// Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_seq_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "last_error.h"

namespace bn {
namespace seq {

constexpr int TILE = 64;                   // rows per tile of the scan (index_scan.h; seq.hip asserts they agree)
constexpr int SLOTS = 64;                  // query rows per pass (index_scan.h, LP)
constexpr size_t SCAN_LDS = 141824;        // index_scan.h's Layout<2>::BYTES: the k chunk, TWO planes of window scores, the selection's lists
constexpr size_t LDS_LIMIT = 160 * 1024;   // gfx950: LDS per workgroup
constexpr int ZRING = 3;                   // tiles whose sequence scores are kept: the judged one and its two neighbours
// what one sequence of a pass takes beyond Layout<2>: its line of ZRING planes [TILE] of sequence scores, the id of its first row and
// whether all of its rows are valid
constexpr size_t PER_SEQ = (size_t)ZRING * TILE * sizeof(float) + sizeof(uint32_t) + sizeof(int);
// sequences per pass at most: what fits under the limit.  160 KB - 141 824 B = 22 016 B; / 776 B = 28
constexpr int CAP = (int)((LDS_LIMIT - SCAN_LDS) / PER_SEQ);
static_assert(BN_SEQ_LEN_MAX == SLOTS && BN_SEQ_LEN_MAX <= TILE, "a sequence fills at most one pass, and a start's windows lie in its tile and the next");
static_assert(BN_PEAK_RADIUS_MAX <= TILE, "a start's neighbours lie in its own tile and the two adjacent ones");
static_assert(PER_SEQ == 776 && CAP == 28, "the figures DESIGN.md and the header quote");

// the dynamic LDS of seq_scan_kernel, as byte offsets: Layout<2> first, then
struct Lds {
    static constexpr size_t Z = SCAN_LDS;                                           // float [ZRING][CAP][TILE]: sequence scores, -inf where not eligible
    static constexpr size_t FIRST = Z + (size_t)ZRING * CAP * TILE * sizeof(float);  // uint32 [CAP]: id of a sequence's first row (_ids form)
    static constexpr size_t OK = FIRST + CAP * sizeof(uint32_t);                     // int [CAP]: every row of the sequence is valid
    static constexpr size_t BYTES = OK + CAP * sizeof(int);
};
static_assert(Lds::BYTES == SCAN_LDS + CAP * PER_SEQ && Lds::BYTES == 163552, "the launch size is part of the kernel's contract");
static_assert(Lds::BYTES <= LDS_LIMIT && Lds::BYTES + PER_SEQ > LDS_LIMIT, "CAP is the largest that fits");
static_assert(Lds::Z % 16 == 0 && ((size_t)CAP * TILE) % 32 == 0, "the planes of the ring share their bank phase");

// sequences of seq_len windows per pass: sequence p, window j sits in query slot p * seq_len + j
constexpr int per_pass(size_t seq_len) { return (int)(SLOTS / seq_len) < CAP ? (int)(SLOTS / seq_len) : CAP; }
// passes over the slab that n_seq sequences take
constexpr size_t passes(size_t n_seq, size_t seq_len) { return (n_seq + per_pass(seq_len) - 1) / per_pass(seq_len); }
// the rounds of a call are query_source.h's, with a sequence as the unit

// The tiles [c0, c1) whose window scores the workgroup owning tiles [t0, t1) of n_tiles computes: a start's windows reach into the next
// tile, and with a peak radius the starts of the tile before and of the tile after the run are judged against
struct Computed {
    uint32_t c0, c1;
};
constexpr Computed computed_tiles(uint32_t t0, uint32_t t1, uint32_t n_tiles, size_t peak_radius) {
    if (t0 >= t1) return {t0, t0};
    const uint32_t before = peak_radius ? 1 : 0, after = peak_radius ? 2 : 1;
    return {t0 - (t0 < before ? t0 : before), n_tiles - t1 < after ? n_tiles : t1 + after};
}

// The refusals that need neither the index nor a device, in the order the header lists them.  `queries` is the query rows or the first ids
inline bn_status check_args(const void *queries, size_t n_seq, size_t seq_len, size_t peak_radius, size_t top_m, size_t m_stride, const uint64_t *id_out,
                            const float *score_out, const uint32_t *count_out) {
    if (top_m < 1 || top_m > 256) return set_last_error(BN_ERR_INVALID_ARG, "top_m must be in 1..256, got " + std::to_string(top_m));
    if (m_stride < top_m) return set_last_error(BN_ERR_INVALID_ARG, "m_stride < top_m");
    if (seq_len < 1 || seq_len > BN_SEQ_LEN_MAX)
        return set_last_error(BN_ERR_INVALID_ARG, "seq_len must be in 1.." + std::to_string(BN_SEQ_LEN_MAX) + ", got " + std::to_string(seq_len));
    if (peak_radius > BN_PEAK_RADIUS_MAX)
        return set_last_error(BN_ERR_INVALID_ARG, "peak_radius must be in 0.." + std::to_string(BN_PEAK_RADIUS_MAX) + ", got " + std::to_string(peak_radius));
    if (n_seq && (!queries || !id_out || !score_out || !count_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    return BN_OK;
}

// the _ids form: every sequence [first_id, first_id + seq_len) lies in an index of `size` rows
inline bn_status check_first_ids(const uint64_t *first_ids, size_t n_seq, size_t seq_len, size_t size) {
    for (size_t i = 0; i < n_seq; i++)
        if (first_ids[i] > size || seq_len > size - first_ids[i])
            return set_last_error(BN_ERR_INVALID_ARG, "rows [" + std::to_string(first_ids[i]) + ", +" + std::to_string(seq_len) + ") of sequence " +
                                                          std::to_string(i) + " run past the index's " + std::to_string(size) + " rows");
    return BN_OK;
}

}  // namespace seq
}  // namespace bn
