// The host-side arithmetic of the grouped threshold search (group.hip, bn_index_group_above and its _ids form) that needs neither a
// device nor the runtime: the refusals of its arguments and the plan of a call -- the workgroup split of the range's tiles, which is
// the threshold search's (above_plan.h, as is the id range: check_range; the query-id check is query_source.h's), and how many
// queries a pass takes so that the device table of (query, group) records stays within above_plan.h's budget.  Host code only, so that
// a stand-alone program can run it under a sanitizer (tools/asan_group_plan.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>

#include "above_plan.h"
#include "last_error.h"

namespace bn {
namespace group {

// bytes of one (query, group) record in the device table: u32 count, u64 best key, u32 first id, u32 last id
constexpr size_t RECORD = 20;
// What the table of ONE PASS may take: a pass of P queries needs P x n_groups x RECORD bytes, and P shrinks from 64 through
// above::WIDTHS until that fits above::BUDGET.  n_groups <= 65536 keeps one query's records at 1.25 MiB, so the floor of one query
// per pass is never reached; at n_groups = 65536 a pass takes 48 queries (60 MiB).  The finished records (another RECORD bytes each:
// ids leave the device as u32) and their pinned mirror are as large again and outside the budget, like the threshold search's
// pinned results.

// The refusals that need neither the index nor a device, in the order the header lists them.  `queries` is the query rows or the
// query ids.  The whole of min_score is read before anything else happens
inline bn_status check_args(const void *queries, size_t n_queries, const float *min_score, size_t n_groups, size_t g_stride, const uint32_t *count_out,
                            const uint64_t *best_id_out, const float *best_score_out) {
    if (n_groups < 1 || n_groups > BN_INDEX_TAG_LIMIT)
        return set_last_error(BN_ERR_INVALID_ARG, "n_groups must be in 1.." + std::to_string(BN_INDEX_TAG_LIMIT) + ", got " + std::to_string(n_groups));
    if (g_stride < n_groups) return set_last_error(BN_ERR_INVALID_ARG, "g_stride < n_groups");
    if (!best_id_out != !best_score_out) return set_last_error(BN_ERR_INVALID_ARG, "best_id_out and best_score_out come as a pair");
    if (n_queries && (!queries || !min_score || !count_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    for (size_t i = 0; i < n_queries; i++)
        if (std::isnan(min_score[i])) return set_last_error(BN_ERR_INVALID_ARG, "min_score[" + std::to_string(i) + "] is NaN");
    return BN_OK;
}

struct Plan {
    uint32_t tile_lo = 0, tile_hi = 0;    // the 64-row tiles that cover the range
    uint32_t tiles_per_wg = 0, n_wg = 0;  // contiguous runs of tiles, at most max_wg workgroups, none empty
    int width = 0;                        // queries per pass
    size_t records = 0;                   // of one pass: width x n_groups
    size_t bytes() const { return records * RECORD; }
};

// the plan of a call over the non-empty range [lo, hi) on a device that runs max_wg >= 1 workgroups at a time, 1 <= n_groups <= 65536
inline Plan plan(uint32_t lo, uint32_t hi, size_t max_wg, size_t n_groups) {
    const above::Plan a = above::plan(lo, hi, max_wg, 0);  // a count's split: no staging
    Plan p;
    p.tile_lo = a.tile_lo, p.tile_hi = a.tile_hi, p.tiles_per_wg = a.tiles_per_wg, p.n_wg = a.n_wg;
    p.width = 1;
    for (int w : above::WIDTHS)
        if ((size_t)w * n_groups * RECORD <= above::BUDGET) {
            p.width = w;
            break;
        }
    p.records = (size_t)p.width * n_groups;
    return p;
}

}  // namespace group
}  // namespace bn
