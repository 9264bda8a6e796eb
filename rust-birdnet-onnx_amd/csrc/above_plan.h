// The host-side arithmetic of the threshold search (above.hip, bn_index_search_above and its _ids form) that needs neither a device nor
// the runtime: the refusals of its arguments, the id range, and the plan of a call -- how the range's tiles are split among workgroups,
// how many staged entries a workgroup keeps per query, and how many queries a pass takes so that staging plus results stay within a
// fixed budget.  Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_above_plan.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "last_error.h"

namespace bn {
namespace above {

constexpr uint32_t TILE = 64;   // rows per tile of the scan (index_scan.h; above.hip asserts they agree)
constexpr int LISTS = 64;       // queries per pass at most (index_scan.h, LP)
constexpr size_t ENTRY = 8;     // bytes of a staged entry: f32 score + u32 id
constexpr size_t RESULT = 12;   // bytes of a result entry on the device: the entry + its u32 tag
// What the staging lists and the device results of ONE PASS may take.  A pass of P queries needs
//     P x (n_wg x cap_wg x ENTRY + max_hits x RESULT) bytes,    cap_wg = min(64 x tiles_per_wg, max_hits),
// and P shrinks from 64 through WIDTHS until that fits; one query per pass is the floor, whatever it takes, which is at most
//     ENTRY x min(rows in the range rounded up to whole workgroups, n_wg x max_hits) + RESULT x max_hits:
// 8 bytes per row against the 512 or more a row takes in the slab, under 2 % of it.  64 MiB: a count or a short list (max_hits up to
// 256 with 256 workgroups) still runs 64 queries per pass, and a device that holds a slab of gigabytes does not notice
// the buffers, which stay with the index once allocated.
constexpr size_t BUDGET = (size_t)64 << 20;
// the widths a pass may have: 64, 48, 32 and 16 fill above_scan_kernel<4 .. 1> exactly; the narrower ones run in <1>
constexpr int WIDTHS[] = {64, 48, 32, 16, 8, 4, 2, 1};

// The refusals that need neither the index nor a device, in the order the header lists them.  `queries` is the query rows or the
// query ids.  The whole of min_score is read before anything else happens
inline bn_status check_args(const void *queries, size_t n_queries, const float *min_score, size_t max_hits, size_t h_stride, const uint64_t *id_out,
                            const float *score_out, const uint32_t *count_out) {
    if (max_hits > BN_ABOVE_MAX_HITS)
        return set_last_error(BN_ERR_INVALID_ARG, "max_hits must be in 0.." + std::to_string(BN_ABOVE_MAX_HITS) + ", got " + std::to_string(max_hits));
    if (h_stride < max_hits) return set_last_error(BN_ERR_INVALID_ARG, "h_stride < max_hits");
    if (n_queries && (!queries || !min_score || !count_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (n_queries && max_hits && (!id_out || !score_out)) return set_last_error(BN_ERR_INVALID_ARG, "null output with max_hits > 0");
    for (size_t i = 0; i < n_queries; i++)
        if (std::isnan(min_score[i])) return set_last_error(BN_ERR_INVALID_ARG, "min_score[" + std::to_string(i) + "] is NaN");
    return BN_OK;
}

// rows [first_id, first_id + n_ids) of an index of `size` rows, n_ids == 0: to the end (bn_head_rank_index's convention) -> [*lo, *hi)
inline bn_status check_range(uint64_t first_id, uint64_t n_ids, size_t size, uint32_t *lo, uint32_t *hi) {
    if (first_id > size || n_ids > size - first_id)
        return set_last_error(BN_ERR_INVALID_ARG, "rows [" + std::to_string(first_id) + ", +" + std::to_string(n_ids) + ") run past the index's " +
                                                      std::to_string(size) + " rows");
    *lo = (uint32_t)first_id;
    *hi = (uint32_t)(n_ids ? first_id + n_ids : size);
    return BN_OK;
}

struct Plan {
    uint32_t tile_lo = 0, tile_hi = 0;       // the 64-row tiles that cover the range
    uint32_t tiles_per_wg = 0, n_wg = 0;     // contiguous runs of tiles, at most max_wg workgroups, none empty
    uint32_t cap_wg = 0;                     // staged entries a workgroup keeps per query; 0 for a count
    int width = 0;                           // queries per pass
    size_t stage_entries = 0;                // of one pass: n_wg x width x cap_wg
    size_t result_entries = 0;               // of one pass: width x max_hits
    size_t bytes() const { return stage_entries * ENTRY + result_entries * RESULT; }
};

// the plan of a call over the non-empty range [lo, hi) on a device that runs max_wg >= 1 workgroups at a time
inline Plan plan(uint32_t lo, uint32_t hi, size_t max_wg, size_t max_hits) {
    Plan p;
    p.tile_lo = lo / TILE;
    p.tile_hi = (uint32_t)(((uint64_t)hi + TILE - 1) / TILE);
    const uint32_t n_tiles = p.tile_hi - p.tile_lo;
    p.tiles_per_wg = (uint32_t)((n_tiles + max_wg - 1) / max_wg);
    p.n_wg = (n_tiles + p.tiles_per_wg - 1) / p.tiles_per_wg;
    const uint64_t rows_wg = (uint64_t)p.tiles_per_wg * TILE;
    p.cap_wg = (uint32_t)(rows_wg < max_hits ? rows_wg : max_hits);
    const size_t per_query = (size_t)p.n_wg * p.cap_wg * ENTRY + max_hits * RESULT;
    p.width = 1;
    for (int w : WIDTHS)
        if ((size_t)w * per_query <= BUDGET) {
            p.width = w;
            break;
        }
    p.stage_entries = (size_t)p.n_wg * p.width * p.cap_wg;
    p.result_entries = (size_t)p.width * max_hits;
    return p;
}

}  // namespace above
}  // namespace bn
