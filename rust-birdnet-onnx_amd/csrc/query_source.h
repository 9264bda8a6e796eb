// Where the queries of a search over an index come from, and how a call walks them: every search takes host rows or stored row ids
// (the _ids forms), refuses an id that names no row, and runs in rounds of as many queries as the index's query buffers hold.  The
// staging and the round loop on the device side of this are index.hip's (for_each_round, capi_internal.h).  Host code only, so that a
// stand-alone program can run it under a sanitizer (tools/asan_query_source.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "last_error.h"

namespace bn {

// Host rows [n x unit, dim], or stored ids [n] with the _ids forms' exclude_radius.  With a unit above 1 (seq.hip: a sequence of
// `unit` windows) an id names the first of `unit` consecutive stored rows.  Without ids the radius is -1, so a launch passes
// `radius` as it is
struct QuerySource {
    const float *rows = nullptr;
    const uint64_t *ids = nullptr;
    int64_t radius = -1;
    static QuerySource host(const float *rows) { return {rows, nullptr, -1}; }
    static QuerySource stored(const uint64_t *ids, int64_t exclude_radius) { return {nullptr, ids, ids ? exclude_radius : -1}; }
    const void *data() const { return ids ? (const void *)ids : (const void *)rows; }  // for a null-argument refusal
};

// the _ids forms' refusal of the first id that is not below `limit`: the index's size, or the rows a view (ivf, sq8) covers
enum class IdLimit { INDEX, VIEW };
inline bn_status check_query_ids(const QuerySource &src, size_t n, size_t limit, IdLimit what = IdLimit::INDEX) {
    for (size_t i = 0; src.ids && i < n; i++)
        if (src.ids[i] >= limit)
            return set_last_error(BN_ERR_INVALID_ARG, "query id " + std::to_string(src.ids[i]) +
                                                          (what == IdLimit::INDEX ? " is not in the index" : " is not among the view's " + std::to_string(limit) + " rows"));
    return BN_OK;
}

// f(first, count) for each round of n queries of `unit` rows each, rows_per_round / unit >= 1 of them per round; stops at the first
// status that is not BN_OK
template <class F>
inline bn_status each_round(size_t n, size_t rows_per_round, size_t unit, F &&f) {
    const size_t per = unit ? rows_per_round / unit : 0;
    if (n && !per) return set_last_error(BN_ERR_INVALID_ARG, "a query of " + std::to_string(unit) + " rows does not fit a round of " + std::to_string(rows_per_round));
    for (size_t first = 0; first < n; first += per)
        if (bn_status st = f(first, std::min(per, n - first)); st != BN_OK) return st;
    return BN_OK;
}

}  // namespace bn
