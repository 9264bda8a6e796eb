// cluster.hip -> ivf.hip: the exact assignment pass and the member lists, so that a view of an index (bn_ivf_*) partitions its rows
// with the very kernels bn_index_assign and bn_index_cluster run.  The kernels stay in cluster.hip; this header is their host side.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "capi_internal.h"

namespace bn {
namespace cluster {

constexpr size_t K_MAX = 1024;  // most centroids of a call

// the centroids [k, dpad] and the running best planes (by row id, whole tiles) one assignment works on
struct AssignBufs {
    DeviceBuf<float> d_cent;
    size_t cent_n = 0;
    DeviceBuf<float> d_best_s;
    DeviceBuf<uint32_t> d_best_i;
    size_t best_n = 0;
};

// rows [id_lo, id_hi) as tiles [tile_lo, tile_hi), tpw tiles to each of n_wg workgroups
struct Range {
    uint32_t id_lo, id_hi, tile_lo, tile_hi, tpw, n_wg;
};

// n_ids == 0: to the end of the index
Range range_of(const IndexScan &s, uint64_t first_id, uint64_t n_ids);
// BN_ERR_INVALID_ARG "`what` element i is not finite"
bn_status check_finite(const float *c, size_t n, const char *what);
// room for k centroids and for planes over the index's rows (a grown plane loses its contents)
bn_status reserve_assign(AssignBufs *b, const IndexScan &s, size_t k);
// host centroids [k, dim], as given, into d_cent [k, dpad] (synchronous)
bn_status upload_centroids(AssignBufs *b, const IndexScan &s, const float *c, size_t k);
// the exact assignment of the range under d_cent[0 .. k) into the planes, on the index's stream.  Every row of the range's tiles
// is written: a row of those tiles outside [id_lo, id_hi) gets (NaN, BN_CLUSTER_NONE)
bn_status enqueue_assign(AssignBufs *b, const IndexScan &s, const Range &r, size_t k);
// offsets[c] = counts[0] + .. + counts[c - 1] (offsets[k]: all), then members[offsets[c] ..) = the ids in [id_lo, id_hi) whose
// best_i is c, ascending; counts must be the sizes of exactly those lists
bn_status enqueue_member_lists(const uint32_t *d_best_i, uint32_t id_lo, uint32_t id_hi, const uint32_t *d_counts, uint32_t k, uint32_t *d_offsets,
                               uint32_t *d_members, hipStream_t stream);

}  // namespace cluster
}  // namespace bn
