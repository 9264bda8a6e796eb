// The host-side arithmetic of the row copy between indexes (index_copy.hip, bn_index_append_rows and bn_index_append_subset) that needs
// neither a device nor the runtime: the refusals of its arguments, the id range, and the plan of a call -- how many 512-byte units the
// rows are, and how many workgroups walk them.  Host code only, so that a stand-alone program can run it under a sanitizer
// (tools/asan_index_copy_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "last_error.h"

namespace bn {
namespace copy {

constexpr uint32_t UNIT_FLOATS = 128;  // floats of a unit, 512 bytes: what a padded row is a whole number of (index_scan.h, KC; index_copy.hip asserts they agree)
constexpr uint32_t UNIT_LANES = 32;    // lanes that move a unit, 16 bytes each: a wave moves two units per instruction
constexpr uint32_t BLOCK = 256;        // threads of a workgroup: 8 half-waves
constexpr uint32_t IN_FLIGHT = 4;      // units a half-wave loads before it stores the first
constexpr uint32_t STEP_UNITS = BLOCK / UNIT_LANES * IN_FLIGHT;  // consecutive units a workgroup moves per step of its grid-stride loop: 16 KB
constexpr uint32_t WG_PER_CU = 8;      // 32 waves per CU, all it holds: the loads in flight are what hides the latency of the id -> row chain
constexpr size_t MAX_CUS = 1u << 16;   // a bound on the CU count taken from the device, so that the grid stays a launchable number
constexpr uint64_t MAX_ROWS = 0xffffffffull - 64;  // bn_index_create's bound on capacity_rows, 2^32 - 1 - TILE (index_copy.hip asserts the 64 is index_scan.h's TILE)

// the refusals that need neither an index nor a device; `second` names the source handle: "index" or "subset"
inline bn_status check_handles(const void *dst, const void *src, const char *second) {
    if (!dst) return set_last_error(BN_ERR_INVALID_ARG, "null destination index");
    if (!src) return set_last_error(BN_ERR_INVALID_ARG, std::string("null source ") + second);
    return BN_OK;
}

// the refusals of a (dst, src) pair, in the header's order; `borrowed`: src came through a subset
inline bn_status check_pair(const void *dst, const void *src, bool borrowed, size_t dst_dim, size_t src_dim, int dst_device, int src_device) {
    if (dst == src)
        return set_last_error(BN_ERR_INVALID_ARG, borrowed ? "the subset borrows the destination index: a copy needs two indexes"
                                                           : "source and destination are the same index: a copy needs two indexes");
    if (dst_dim != src_dim)
        return set_last_error(BN_ERR_INVALID_ARG, "the source has dim " + std::to_string(src_dim) + ", the destination " + std::to_string(dst_dim));
    if (dst_device != src_device)
        return set_last_error(BN_ERR_INVALID_ARG, "the source lives on device " + std::to_string(src_device) + ", the destination on " +
                                                      std::to_string(dst_device) + ": rows are not copied between devices");
    return BN_OK;
}

// rows [first_id, first_id + n_ids) of a source of `size` rows, n_ids == 0: to the end (bn_index_assign's convention) -> *first, *n
inline bn_status check_range(uint64_t first_id, uint64_t n_ids, size_t size, uint64_t *first, uint64_t *n) {
    if (first_id > size || n_ids > size - first_id)
        return set_last_error(BN_ERR_INVALID_ARG, "the id range [" + std::to_string(first_id) + ", +" + std::to_string(n_ids) + ") is not in the source (" +
                                                      std::to_string(size) + " rows)");
    *first = first_id;
    *n = n_ids ? n_ids : size - first_id;
    return BN_OK;
}

struct Plan {
    uint32_t units_per_row = 0;  // dpad / 128
    uint64_t n_units = 0;        // n x units_per_row
    uint32_t grid = 0;           // workgroups: every one has a step of its own, at most WG_PER_CU per CU
    size_t slab_bytes = 0;       // n x dpad x 4: what the copy reads, and what it writes
};

// the plan of a copy of n >= 1 rows of dpad floats on a device of max_wg >= 1 CUs.  Refused rather than wrapped: a dpad that is not
// whole units, more rows than an index can hold, a byte count beyond size_t
inline bn_status plan(uint64_t n, size_t dpad, size_t max_wg, Plan *out) {
    if (n == 0 || max_wg == 0) return set_last_error(BN_ERR_INVALID_ARG, "copy plan: nothing to plan");
    if (dpad == 0 || dpad % UNIT_FLOATS || dpad / UNIT_FLOATS > 0xffffffffull)
        return set_last_error(BN_ERR_INVALID_ARG, "copy plan: a padded row of " + std::to_string(dpad) + " floats is not whole 512-byte units");
    if (n > MAX_ROWS) return set_last_error(BN_ERR_INVALID_ARG, "copy plan: " + std::to_string(n) + " rows are more than an index holds");
    const uint64_t upr = dpad / UNIT_FLOATS;
    if (n > UINT64_MAX / upr || n * upr > SIZE_MAX / (UNIT_FLOATS * sizeof(float)))
        return set_last_error(BN_ERR_INVALID_ARG, "copy plan: " + std::to_string(n) + " rows of " + std::to_string(dpad) + " floats overflow the byte count");
    Plan p;
    p.units_per_row = (uint32_t)upr;
    p.n_units = n * upr;
    p.slab_bytes = (size_t)p.n_units * UNIT_FLOATS * sizeof(float);
    const uint64_t steps = (p.n_units + STEP_UNITS - 1) / STEP_UNITS;
    const uint64_t most = (uint64_t)(max_wg < MAX_CUS ? max_wg : MAX_CUS) * WG_PER_CU;
    p.grid = (uint32_t)(steps < most ? steps : most);
    *out = p;
    return BN_OK;
}

}  // namespace copy
}  // namespace bn
