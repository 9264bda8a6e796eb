// bn_index_append_rows / bn_index_append_subset behind the C ABI (include/birdnet_hip.h): rows of one index appended to another, device
// to device, with the bits they are stored with, their valid bytes and their tags.  Nothing is normalised again, so the destination
// answers as if its own appends had produced these bits.  The refusals and the plan of a call are index_copy_plan.h's (host only).
//
// Kernel of this file:
//   * index_copy_kernel -- both slabs are padded row-major, dpad a multiple of 128 floats: every row on both sides is a whole number of
//     512-byte units, 16-byte aligned.  The work is numbered flat in units of the DESTINATION (contiguous from the first new row): unit
//     u is piece u % upr of new row u / upr, upr = dpad / 128, and 32 lanes move it with one 16-byte load and one 16-byte store each,
//     so a wave moves two units per instruction and every lane is busy at dim 3 as at dim 1536 (the one-wave-per-row form of
//     index_io.hip leaves 32 of 64 lanes idle at dpad 128 and runs one short row per wave).  The source row of a new row is
//     ids[row] (a subset's list) or first_id + row (ids == NULL): one body, the list or its absence.  The id is read once per
//     unit, by a load all 32 lanes share.  Lane 0 of a row's first unit also carries the row's valid byte and, where the destination has a
//     tag plane, its tag (0 where the source has none): no second pass over the rows.  A workgroup's step is 32 consecutive units (16 KB
//     of the destination): each of its 8 half-waves has 4 units in flight, ids first, then the rows' loads, then the stores, so the
//     id -> row dependency is paid once per four units.  One grid form: at most 8 workgroups per CU in a grid-stride loop over the steps.
//     Plain vector loads and stores, no atomics, no LDS: the same state gives the same bytes.
#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "capi_internal.h"
#include "index_copy_plan.h"
#include "index_scan.h"

namespace {

using bn::check_launch;
using bn::set_last_error;
using bn::copy::BLOCK;
using bn::copy::IN_FLIGHT;
using bn::copy::STEP_UNITS;
using bn::copy::UNIT_LANES;
constexpr uint32_t HALVES = BLOCK / UNIT_LANES;  // half-waves of a workgroup

static_assert(bn::copy::UNIT_FLOATS == (uint32_t)bn::scan::KC, "a padded row is whole units");
static_assert(UNIT_LANES * sizeof(uint4) == bn::copy::UNIT_FLOATS * sizeof(float), "32 lanes x 16 bytes are one unit");
static_assert(bn::copy::MAX_ROWS == 0xffffffffull - bn::scan::TILE, "bn_index_create's bound");

// dst: the first new row; new row j = source row (LIST ? ids[j] : first_id + j), for the n_units / upr new rows.  TAGS: the source has a
// tag plane (and so has the destination); otherwise the new tags are 0, written where dst_tags is not NULL.  The loads of a step are
// straight-line code (a branch between them would make each wait for the one before): a unit past the end repeats the last unit's
// loads and stores nothing, and every lane loads its row's valid byte and tag, which lane 0 of the row's first unit stores
template <bool LIST, bool TAGS>
__global__ __launch_bounds__(BLOCK) void index_copy_kernel(const uint4 *__restrict__ src, const uint8_t *__restrict__ src_valid,
                                                           const uint16_t *__restrict__ src_tags, const uint32_t *__restrict__ ids, uint32_t first_id,
                                                           uint64_t n_units, uint32_t upr, uint4 *__restrict__ dst, uint8_t *__restrict__ dst_valid,
                                                           uint16_t *__restrict__ dst_tags) {
    const uint32_t l = threadIdx.x % UNIT_LANES, h = threadIdx.x / UNIT_LANES;
    for (uint64_t base = (uint64_t)blockIdx.x * STEP_UNITS; base < n_units; base += (uint64_t)gridDim.x * STEP_UNITS) {
        // the step's first unit: uniform, so this division is the scalar unit's; a lane's own unit is at most 31 further
        const uint64_t row0 = base / upr;
        const uint32_t piece0 = (uint32_t)(base - row0 * upr);
        const uint32_t last = (uint32_t)min((uint64_t)(STEP_UNITS - 1), n_units - 1 - base);  // the step's last unit that exists
        uint64_t row[IN_FLIGHT];
        uint32_t piece[IN_FLIGHT], from[IN_FLIGHT];
#pragma unroll
        for (uint32_t k = 0; k < IN_FLIGHT; k++) {
            const uint32_t p = piece0 + min(k * HALVES + h, last);
            row[k] = row0 + p / upr;
            piece[k] = p % upr;
            from[k] = LIST ? ids[row[k]] : first_id + (uint32_t)row[k];
        }
        uint4 v[IN_FLIGHT];
        uint32_t ok[IN_FLIGHT], tag[IN_FLIGHT];
#pragma unroll
        for (uint32_t k = 0; k < IN_FLIGHT; k++) {
            v[k] = src[((uint64_t)from[k] * upr + piece[k]) * UNIT_LANES + l];
            ok[k] = src_valid[from[k]];
            tag[k] = TAGS ? src_tags[from[k]] : 0u;
        }
        // every load of the step is issued before its first store: left alone the compiler sinks each load into the predicated block
        // of its store, and a unit waits for the unit before it.  An empty statement that names the registers; no instruction
#pragma unroll
        for (uint32_t k = 0; k < IN_FLIGHT; k++) asm volatile("" : "+v"(v[k].x), "+v"(v[k].y), "+v"(v[k].z), "+v"(v[k].w), "+v"(ok[k]), "+v"(tag[k]));
#pragma unroll
        for (uint32_t k = 0; k < IN_FLIGHT; k++) {
            const uint32_t o = k * HALVES + h;
            if (o > last) continue;
            dst[(base + o) * UNIT_LANES + l] = v[k];
            if (piece[k] == 0 && l == 0) {
                dst_valid[row[k]] = (uint8_t)ok[k];
                if (dst_tags) dst_tags[row[k]] = (uint16_t)tag[k];
            }
        }
    }
}

// rows of src -> the end of dst, after every refusal that needs no slab: new row j = ids ? ids[j] : first + j, j in [0, n)
bn_status append(bn_index *dst, bn_index *src, const uint32_t *d_ids, uint64_t first, uint64_t n, uint64_t *first_new_id) {
    if (n == 0) {  // no launch
        if (first_new_id) *first_new_id = bn_index_size(dst);
        return BN_OK;
    }
    // the capacity refusal and the plan first: neither changes anything, and index_copy_begin may give dst a tag plane
    size_t dpad = 0;
    int max_wg = 0;
    bn_status st = bn::index_copy_shape(dst, (size_t)n, &dpad, &max_wg);
    if (st != BN_OK) return st;
    bn::copy::Plan p;
    if ((st = bn::copy::plan(n, dpad, (size_t)max_wg, &p)) != BN_OK) return st;
    bn::IndexCopy c;
    if ((st = bn::index_copy_begin(dst, src, (size_t)n, &c)) != BN_OK) return st;
    const auto launch = [&](auto list, auto tags) {
        hipLaunchKernelGGL((index_copy_kernel<decltype(list)::value, decltype(tags)::value>), dim3(p.grid), dim3(BLOCK), 0, c.stream,
                           reinterpret_cast<const uint4 *>(c.src_slab), c.src_valid, c.src_tags, d_ids, (uint32_t)first, p.n_units, p.units_per_row,
                           reinterpret_cast<uint4 *>(c.dst_slab), c.dst_valid, c.dst_tags);
    };
    // one body, four instantiations: the list or its absence, the source's tag plane or its absence
    if (d_ids) c.src_tags ? launch(std::true_type{}, std::true_type{}) : launch(std::true_type{}, std::false_type{});
    else c.src_tags ? launch(std::false_type{}, std::true_type{}) : launch(std::false_type{}, std::false_type{});
    if ((st = check_launch("index copy")) != BN_OK) return st;
    BN_HIP_TRY(hipStreamSynchronize(c.stream));
    bn::index_copy_commit(dst, (size_t)n);
    if (first_new_id) *first_new_id = c.first;
    return BN_OK;
}

bn_status check_pair(const bn_index *dst, const bn_index *src, bool borrowed) {
    return bn::copy::check_pair(dst, src, borrowed, bn_index_dim(dst), bn_index_dim(src), bn::index_device(dst), bn::index_device(src));
}

}  // namespace

extern "C" {

bn_status bn_index_append_rows(bn_index *dst, bn_index *src, uint64_t first_id, uint64_t n_ids, uint64_t *first_new_id) {
    bn_status st = bn::copy::check_handles(dst, src, "index");
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if ((st = check_pair(dst, src, false)) != BN_OK) return st;
    uint64_t first = 0, n = 0;
    if ((st = bn::copy::check_range(first_id, n_ids, bn_index_size(src), &first, &n)) != BN_OK) return st;
    return append(dst, src, nullptr, first, n, first_new_id);
}

bn_status bn_index_append_subset(bn_index *dst, const bn_subset *s, uint64_t *first_new_id) {
    bn_status st = bn::copy::check_handles(dst, s, "subset");
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    const bn::SubsetList list = bn::subset_list(s);
    if ((st = check_pair(dst, list.x, true)) != BN_OK) return st;
    return append(dst, list.x, list.d_ids, 0, list.n, first_new_id);
}

}  // extern "C"
