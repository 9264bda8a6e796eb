// bn_index_group_above / bn_index_group_above_ids behind the C ABI (include/birdnet_hip.h): the hits of the threshold search grouped by
// row tag -- per (query, group) the number of hits, the best hit, the first and the last id -- without returning a single hit.  A hit
// is bn_index_search_above's, its score has bn_index_search's bits.
//
// Kernels of this file:
//   * group_scan_kernel<QB> -- above_scan_kernel's tile loop written out once more (index_scan.h says why every scan keeps its own):
//     64 queries per pass in LDS, the exact-f32 MFMA v_mfma_f32_16x16x4_f32 with row = A operand and query = B operand, one accumulator
//     per (query, row) over k ascending, the same workgroup-to-tile split and the same masks at the range's ends.  What differs is the
//     tail of a tile.  The tile's 64 tags are read once (lane = row; 0 without a plane).  Wave w takes queries w, w + 4, ...; ONE ballot
//     of the hit predicate, and with an empty mask nothing else happens.  Otherwise the hits update the record (query, tag) of a device
//     table [queries of the pass][n_groups] with INTEGER atomics whose result does not depend on their order: add on the count, max on
//     a u64 key (order-preserving transform of the score bits above ~id: the highest score, then the lowest id), min and max on the
//     id.  Rows of one recorder are contiguous, so the hit lanes of a tile mostly carry ONE tag: then the wave reduces (popcount, a
//     32-bit max and a ballot of the lanes that reach it, the mask's first and last bit) and lane 0 issues the four updates; otherwise
//     every hit lane issues its own.  Hits whose tag is >= n_groups, and all hits, are counted per query in LDS and added to the
//     pass's head once per workgroup.
//   * group_finish_kernel -- one thread per record: the table becomes the output record (count, best id and score unpacked from the
//     key, first, last; the empty record where the count is 0) and goes back to its reset state for the next pass; the head
//     (total, other per query) likewise.  Ids leave the device as u32 (an index holds fewer than 2^32 - 64 rows; 0xffffffff: none).
//   * group_reset_kernel -- the reset state of a table that was just allocated, or that a failed call left behind.
// No floating-point atomics, no scratch.  No workgroup-private LDS table as a second level: DESIGN.md ("Grouped threshold search")
// has the measurement that decided it.
//
// Host side: index.hip's for_each_round stages the queries of either source in rounds of out_lists; a round is one
// run_threshold_passes (shared with above.hip): the round's thresholds go up, then passes of Plan::width queries (group_plan.h), and
// what comes back per pass is one copy per output array the caller asked for.  The buffers belong to the index (GroupState), allocated
// on first need and only ever grown.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "capi_internal.h"
#include "device_common.h"
#include "group_plan.h"
#include "hip_gate.h"
#include "index_scan.h"
#include "topm_select.h"

namespace bn {
struct GroupState {
    DeviceBuf<float> d_thr;      // [out_lists]: min_score of the round's queries
    DeviceBuf<uint32_t> d_head;  // [2][QP]: total hits per query; hits in no group.  Zero between passes
    DeviceBuf<uint32_t> d_tab;   // the table, cap records: count [cap], first [cap], last [cap], key [cap] (u64); reset between passes
    DeviceBuf<uint32_t> d_out;   // the finished records: count, best id, best score, first, last [cap] each, then the head [2][QP]
    PinnedBuf<uint32_t> h_out;   // likewise
    size_t cap = 0;              // records, even
    bool dirty = true;           // the table or the head may not be in the reset state
};
}  // namespace bn

namespace {

using bn::scan::KC;
using bn::scan::QS_LD;
using bn::scan::S_LD;
using bn::scan::TILE;
constexpr int QP = bn::scan::LP;  // queries per scan pass at most
static_assert(bn::above::TILE == TILE && bn::above::LISTS == QP, "above_plan.h restates index_scan.h");
static_assert(bn::group::RECORD == 3 * sizeof(uint32_t) + sizeof(unsigned long long), "group_plan.h's record");

using bn::floatx4;

// AboveLayout, then the hits of each list whose tag names no group
constexpr size_t LDS_OTH = bn::scan::AboveLayout::BYTES;
constexpr size_t GROUP_LDS = LDS_OTH + QP * sizeof(uint32_t);
static_assert(GROUP_LDS <= 64 * 1024, "below the size from which a kernel must opt in");

constexpr uint32_t NO_ROW = 0xffffffffu;  // no id can be it: an index holds fewer than 2^32 - 64 rows

// the table of a pass as the kernels see it; record (query q of the pass, group g) is q * n_groups + g.  Reset state: count 0, key 0,
// first NO_ROW, last 0
struct Table {
    uint32_t *count, *first, *last;
    unsigned long long *key;
};

// score bits -> u32 that orders as the scores do (-0.0 as +0.0; a score is never -0.0: an accumulator starts at +0.0 and a sum is -0.0
// only when both terms are), and back
__device__ inline uint32_t ordered(float s) {
    uint32_t b = __float_as_uint(s);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float unordered(uint32_t t) { return __uint_as_float((t & 0x80000000u) ? (t ^ 0x80000000u) : ~t); }

// Scan of one pass (nq <= QP queries, QB = ceil(nq / 16) query blocks) over rows [id_lo, id_hi).  Workgroup g owns tiles
// [tile_lo + g * tiles_per_wg, ...) below tile_hi.  Operands as in index_scan_kernel: lane l of wave w: A = row (tile row 16w + (l & 15)),
// k = 16s + 4(l >> 4) + c of each KC chunk; B = query 16qb + (l & 15) at the same k.  D: query 16qb + (l & 15), row 16w + 4(l >> 4) + reg.
// Out: the records of `tab`, head[q] += hits of query q, head[QP + q] += those with a tag >= n_groups.
template <int QB>
__global__ __launch_bounds__(256) void group_scan_kernel(const float *__restrict__ slab, const uint8_t *__restrict__ valid, uint32_t id_lo, uint32_t id_hi,
                                                         uint32_t dpad, const float *__restrict__ q, const uint8_t *__restrict__ qvalid, int nq,
                                                         const uint32_t *__restrict__ qid, int64_t radius, const float *__restrict__ min_score,
                                                         uint32_t tile_lo, uint32_t tile_hi, uint32_t tiles_per_wg, const uint16_t *__restrict__ tags,
                                                         uint32_t n_groups, Table tab, uint32_t *__restrict__ head) {
    extern __shared__ __align__(16) char gr_lds[];
    using L = bn::scan::AboveLayout;
    float *Qs = reinterpret_cast<float *>(gr_lds + L::B);          // [QP][QS_LD]: the queries' current k chunk
    float *S = reinterpret_cast<float *>(gr_lds + L::S);           // [QP][S_LD]: scores of the current tile
    float *thr = reinterpret_cast<float *>(gr_lds + L::THR);       // [QP]
    uint32_t *cnt = reinterpret_cast<uint32_t *>(gr_lds + L::CNT);  // [QP]: hits of the list in this workgroup's tiles
    uint32_t *oth = reinterpret_cast<uint32_t *>(gr_lds + LDS_OTH);  // [QP]: those in no group

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r16 = lane & 15, h = lane >> 4;
    for (int i = tid; i < QP; i += 256) {
        cnt[i] = 0;
        oth[i] = 0;
        thr[i] = i < nq ? min_score[i] : __builtin_inff();
    }
    const uint32_t t0 = (uint32_t)min((uint64_t)tile_hi, (uint64_t)tile_lo + (uint64_t)blockIdx.x * tiles_per_wg);
    const uint32_t t1 = (uint32_t)min((uint64_t)tile_hi, (uint64_t)t0 + tiles_per_wg);
    const uint32_t nkc = dpad / KC;
    const uint32_t steps = (t1 - t0) * nkc;

    // step u = (tile t0 + u / nkc, chunk u % nkc); the row chunk and the query chunk of step u + 1 are loaded during step u
    auto row_ptr = [&](uint32_t u) {
        const size_t row = (size_t)(t0 + u / nkc) * TILE + w * 16 + r16;  // < the slab's rows (padded to TILE)
        return slab + row * dpad + (u % nkc) * KC + 4 * h;
    };
    constexpr int QV = QB * 16 * (KC / 4) / 256;  // float4 of the query chunk per thread
    auto load_q = [&](uint32_t u, float4 *qr) {
        const uint32_t c = u % nkc;
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            qr[j] = qq < nq ? *reinterpret_cast<const float4 *>(q + (size_t)qq * dpad + c * KC + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float4 a[8], qr[QV];
    if (steps) {
        const float *rp = row_ptr(0);
#pragma unroll
        for (int s = 0; s < 8; s++) a[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
        load_q(0, qr);
    }
    floatx4 acc[QB];
#pragma unroll
    for (int b = 0; b < QB; b++) acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};

    for (uint32_t u = 0; u < steps; u++) {
        __syncthreads();  // the previous chunk's Qs reads are done
#pragma unroll
        for (int j = 0; j < QV; j++) {
            const int e = tid + 256 * j, qq = e >> 5, kk = (e & 31) * 4;
            *reinterpret_cast<float4 *>(Qs + qq * QS_LD + kk) = qr[j];
        }
        __syncthreads();
        float4 an[8];
        if (u + 1 < steps) {
            const float *rp = row_ptr(u + 1);
#pragma unroll
            for (int s = 0; s < 8; s++) an[s] = *reinterpret_cast<const float4 *>(rp + 16 * s);
            load_q(u + 1, qr);
        }
#pragma unroll
        for (int s = 0; s < 8; s++) {
#pragma unroll
            for (int b = 0; b < QB; b++) {
                const float4 bq = *reinterpret_cast<const float4 *>(Qs + (b * 16 + r16) * QS_LD + 16 * s + 4 * h);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].x, bq.x, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].y, bq.y, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].z, bq.z, acc[b], 0, 0, 0);
                acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s].w, bq.w, acc[b], 0, 0, 0);
            }
        }
        if (u + 1 < steps) {
#pragma unroll
            for (int s = 0; s < 8; s++) a[s] = an[s];
        }
        if ((u + 1) % nkc) continue;

        // ---- end of a tile: scores to LDS, then the hits of each query update their groups (wave w owns queries w, w + 4, ...)
        const uint32_t t = t0 + u / nkc;
#pragma unroll
        for (int b = 0; b < QB; b++) {
#pragma unroll
            for (int r = 0; r < 4; r++) S[(b * 16 + r16) * S_LD + w * 16 + h * 4 + r] = acc[b][r];
            acc[b] = floatx4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const uint32_t base = t * TILE, grow = base + lane;   // grow < the plane's rows: it covers the slab's capacity, padded to TILE
        const bool row_ok = grow >= id_lo && grow < id_hi && valid[grow];
        const uint32_t tag = tags ? tags[grow] : 0u;
        const bool grouped = tag < n_groups;
        for (int qq = w; qq < nq; qq += 4) {
            if (!qvalid[qq]) continue;
            bool ok = row_ok;
            if (radius >= 0) {
                const int64_t d = (int64_t)grow - (int64_t)qid[qq];
                ok = ok && (d > radius || d < -radius);
            }
            const float s = S[qq * S_LD + lane];
            const bool hit = ok && s >= thr[qq];
            const uint64_t m = __ballot(hit);
            if (!m) continue;
            const uint64_t mg = __ballot(hit && grouped);
            if (lane == 0) {  // read again only by this wave, after the next tile's barriers
                cnt[qq] += (uint32_t)__popcll(m);
                if (m != mg) oth[qq] += (uint32_t)__popcll(m & ~mg);
            }
            if (!mg) continue;
            const int lo_lane = __ffsll((unsigned long long)mg) - 1, hi_lane = 63 - __clzll((unsigned long long)mg);
            const uint32_t tag0 = (uint32_t)__shfl((int)tag, lo_lane);
            const bool mine = hit && grouped;
            const uint32_t key = mine ? ordered(s) : 0u;  // of a hit: above 0
            if (!__ballot(mine && tag != tag0)) {
                // one group takes every hit of the tile: reduce in the wave, one lane updates
                uint32_t top = key;
#pragma unroll
                for (int o = 32; o; o >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, o));
                const uint64_t mb = __ballot(mine && key == top);  // not empty: top is the key of a hit lane
                if (lane == 0) {
                    const size_t rec = (size_t)qq * n_groups + tag0;
                    const uint32_t best = base + (uint32_t)(__ffsll((unsigned long long)mb) - 1);
                    atomicAdd(tab.count + rec, (uint32_t)__popcll(mg));
                    atomicMax(tab.key + rec, ((unsigned long long)top << 32) | (uint32_t)~best);
                    atomicMin(tab.first + rec, base + (uint32_t)lo_lane);
                    atomicMax(tab.last + rec, base + (uint32_t)hi_lane);
                }
            } else if (mine) {
                const size_t rec = (size_t)qq * n_groups + tag;
                atomicAdd(tab.count + rec, 1u);
                atomicMax(tab.key + rec, ((unsigned long long)key << 32) | (uint32_t)~grow);
                atomicMin(tab.first + rec, grow);
                atomicMax(tab.last + rec, grow);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < nq; i += 256) {
        if (cnt[i]) atomicAdd(head + i, cnt[i]);
        if (oth[i]) atomicAdd(head + QP + i, oth[i]);
    }
}

// the finished records of a pass, cap apart: count, best id, best score bits, first id, last id; then the head
struct Finished {
    uint32_t *count, *best_id, *best_score, *first, *last, *head;
};

// thread = record i < n of the table -> its output record, and the table's reset state; threads below 2 * QP also move the head
__global__ __launch_bounds__(256) void group_finish_kernel(Table tab, uint32_t *__restrict__ head, size_t n, Finished out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * QP) {
        out.head[i] = head[i];
        head[i] = 0;
    }
    if (i >= n) return;
    const uint32_t c = tab.count[i];
    const unsigned long long k = tab.key[i];
    out.count[i] = c;
    out.best_id[i] = c ? ~(uint32_t)k : NO_ROW;
    out.best_score[i] = c ? __float_as_uint(unordered((uint32_t)(k >> 32))) : 0u;
    out.first[i] = c ? tab.first[i] : NO_ROW;
    out.last[i] = c ? tab.last[i] : NO_ROW;
    if (c) {
        tab.count[i] = 0;
        tab.key[i] = 0;
        tab.first[i] = NO_ROW;
        tab.last[i] = 0;
    }
}

__global__ __launch_bounds__(256) void group_reset_kernel(Table tab, uint32_t *__restrict__ head, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 2 * QP) head[i] = 0;
    if (i >= n) return;
    tab.count[i] = 0;
    tab.key[i] = 0;
    tab.first[i] = NO_ROW;
    tab.last[i] = 0;
}

using bn::check_launch;
using bn::set_last_error;

Table table_of(const bn::GroupState &g) {
    uint32_t *p = g.d_tab.get();
    return Table{p, p + g.cap, p + 2 * g.cap, reinterpret_cast<unsigned long long *>(p + 3 * g.cap)};  // cap is even: 8-byte aligned
}
Finished finished_of(uint32_t *p, size_t cap) { return Finished{p, p + cap, p + 2 * cap, p + 3 * cap, p + 4 * cap, p + 5 * cap}; }

unsigned blocks_for(size_t n) { return (unsigned)((std::max<size_t>(n, 2 * QP) + 255) / 256); }

// the state of an index with room for `records` records, its table in the reset state; the stream is idle when a buffer is replaced
bn_status state_of(bn_index *ix, const bn::IndexScan &x, size_t records, bn::GroupState **out) {
    bn::GroupState **slot = bn::index_group_state(ix);
    if (!*slot) {
        auto s = std::make_unique<bn::GroupState>();
        BN_HIP_TRY(s->d_thr.alloc(x.out_lists * sizeof(float)));
        BN_HIP_TRY(s->d_head.alloc(2 * QP * sizeof(uint32_t)));
        *slot = s.release();
    }
    bn::GroupState &g = **slot;
    if (records > g.cap) {
        BN_HIP_TRY(hipStreamSynchronize(x.stream));  // nothing reads a buffer that is replaced
        const size_t cap = (records + 1) & ~(size_t)1;
        g.cap = 0;
        g.dirty = true;
        BN_HIP_TRY(g.d_tab.alloc(cap * bn::group::RECORD));
        BN_HIP_TRY(g.d_out.alloc((cap * 5 + 2 * QP) * sizeof(uint32_t)));
        BN_HIP_TRY(g.h_out.alloc((cap * 5 + 2 * QP) * sizeof(uint32_t)));
        g.cap = cap;
    }
    if (g.dirty) {
        hipLaunchKernelGGL(group_reset_kernel, dim3(blocks_for(g.cap)), dim3(256), 0, x.stream, table_of(g), g.d_head.get(), g.cap);
        if (bn_status st = check_launch("group reset"); st != BN_OK) return st;
        BN_HIP_TRY(hipStreamSynchronize(x.stream));
        g.dirty = false;
    }
    *out = &g;
    return BN_OK;
}

// the caller's arrays; NULL where the caller passed NULL
struct Outputs {
    uint32_t *count;
    uint64_t *best_id;
    float *best_score;
    uint64_t *first, *last;
    uint32_t *other, *total;
};

inline uint64_t wide(uint32_t id) { return id == NO_ROW ? BN_GROUP_NO_ROW : (uint64_t)id; }

// One pass: the np <= pl.width queries `q` of the staged round, which are queries p0 .. of the round and i0 .. of the call.  Scan,
// finish; one copy per array the caller asked for, then into the caller's arrays at query index i0.  Synchronous
bn_status run_pass(const bn::IndexScan &x, bn::GroupState &g, const bn::group::Plan &pl, uint32_t lo, uint32_t hi, const bn::StagedQueries &q, size_t p0, int np,
                   size_t i0, size_t n_groups, size_t g_stride, const Outputs &o) {
    const size_t n = (size_t)np * n_groups;
    const Table tab = table_of(g);
    const Finished d = finished_of(g.d_out.get(), g.cap), hst = finished_of(g.h_out.get(), g.cap);
    g.dirty = true;
    bn::by_blocks(np, [&](auto qb) {
        hipLaunchKernelGGL(group_scan_kernel<decltype(qb)::value>, dim3(pl.n_wg), dim3(256), GROUP_LDS, x.stream, x.slab, x.valid, lo, hi, (uint32_t)x.dpad,
                           q.d_q, q.d_qvalid, np, q.d_qid, q.radius, g.d_thr + p0, pl.tile_lo, pl.tile_hi, pl.tiles_per_wg, x.tags, (uint32_t)n_groups, tab,
                           g.d_head.get());
    });
    if (bn_status st = check_launch("group scan"); st != BN_OK) return st;
    hipLaunchKernelGGL(group_finish_kernel, dim3(blocks_for(n)), dim3(256), 0, x.stream, tab, g.d_head.get(), n, d);
    if (bn_status st = check_launch("group finish"); st != BN_OK) return st;
    auto back = [&](uint32_t *dst, const uint32_t *src, size_t words) { return hipMemcpyAsync(dst, src, words * sizeof(uint32_t), hipMemcpyDeviceToHost, x.stream); };
    BN_HIP_TRY(back(hst.count, d.count, n));
    if (o.best_id) {
        BN_HIP_TRY(back(hst.best_id, d.best_id, n));
        BN_HIP_TRY(back(hst.best_score, d.best_score, n));
    }
    if (o.first) BN_HIP_TRY(back(hst.first, d.first, n));
    if (o.last) BN_HIP_TRY(back(hst.last, d.last, n));
    if (o.other || o.total) BN_HIP_TRY(back(hst.head, d.head, 2 * QP));
    BN_HIP_TRY(hipStreamSynchronize(x.stream));
    g.dirty = false;
    for (int i = 0; i < np; i++) {
        const size_t from = (size_t)i * n_groups, to = (i0 + i) * g_stride;
        std::copy(hst.count + from, hst.count + from + n_groups, o.count + to);
        if (o.best_id) {
            std::transform(hst.best_id + from, hst.best_id + from + n_groups, o.best_id + to, wide);
            std::memcpy(o.best_score + to, hst.best_score + from, n_groups * sizeof(float));  // the bits as they are
        }
        if (o.first) std::transform(hst.first + from, hst.first + from + n_groups, o.first + to, wide);
        if (o.last) std::transform(hst.last + from, hst.last + from + n_groups, o.last + to, wide);
        if (o.total) o.total[i0 + i] = hst.head[i];
        if (o.other) o.other[i0 + i] = hst.head[QP + i];
    }
    return BN_OK;
}

// every record of the call is the empty record, every count 0: an empty index, an empty range
void write_empty(size_t n_queries, size_t n_groups, size_t g_stride, const Outputs &o) {
    for (size_t i = 0; i < n_queries; i++) {
        const size_t at = i * g_stride;
        std::fill(o.count + at, o.count + at + n_groups, 0u);
        if (o.best_id) {
            std::fill(o.best_id + at, o.best_id + at + n_groups, BN_GROUP_NO_ROW);
            std::fill(o.best_score + at, o.best_score + at + n_groups, 0.0f);
        }
        if (o.first) std::fill(o.first + at, o.first + at + n_groups, BN_GROUP_NO_ROW);
        if (o.last) std::fill(o.last + at, o.last + at + n_groups, BN_GROUP_NO_ROW);
        if (o.other) o.other[i] = 0;
        if (o.total) o.total[i] = 0;
    }
}

bn_status group(bn_index *ix, const bn::QuerySource &src, size_t n_queries, const float *min_score, uint64_t first_id, uint64_t n_ids, size_t n_groups,
                size_t g_stride, const Outputs &o) {
    bn_status st = bn::group::check_args(src.data(), n_queries, min_score, n_groups, g_stride, o.count, o.best_id, o.best_score);
    if (st != BN_OK) return st;
    if ((st = bn::require_any_device()) != BN_OK) return st;
    if (!ix) return set_last_error(BN_ERR_INVALID_ARG, "null index");
    const size_t size = bn_index_size(ix);
    uint32_t lo = 0, hi = 0;
    if ((st = bn::above::check_range(first_id, n_ids, size, &lo, &hi)) != BN_OK) return st;
    if ((st = bn::check_query_ids(src, n_queries, size)) != BN_OK) return st;
    if (lo == hi || n_queries == 0) {  // an empty index, an empty range, no query: no launch
        write_empty(n_queries, n_groups, g_stride, o);
        return BN_OK;
    }
    bn::IndexScan x;
    if ((st = bn::index_scan_state(ix, &x)) != BN_OK) return st;
    const bn::group::Plan pl = bn::group::plan(lo, hi, (size_t)x.max_wg, n_groups);
    bn::GroupState *g = nullptr;
    if ((st = state_of(ix, x, std::min<size_t>(pl.width, n_queries) * n_groups, &g)) != BN_OK) return st;  // the widest pass of this call
    return bn::for_each_round(ix, src, n_queries, 1, [&](size_t q0, size_t nq, const bn::StagedQueries &staged) {
        return bn::run_threshold_passes(x.stream, g->d_thr, min_score + q0, nq, (size_t)pl.width, [&](size_t p0, int np) {
            return run_pass(x, *g, pl, lo, hi, staged.at(p0), p0, np, q0 + p0, n_groups, g_stride, o);
        });
    });
}

}  // namespace

void bn::group_state_free(GroupState *s) { delete s; }

extern "C" {

bn_status bn_index_group_above(bn_index *x, const float *queries, size_t n_queries, const float *min_score, uint64_t first_id, uint64_t n_ids,
                               size_t n_groups, size_t g_stride, uint32_t *count_out, uint64_t *best_id_out, float *best_score_out, uint64_t *first_id_out,
                               uint64_t *last_id_out, uint32_t *other_out, uint32_t *total_out) {
    return group(x, bn::QuerySource::host(queries), n_queries, min_score, first_id, n_ids, n_groups, g_stride,
                 Outputs{count_out, best_id_out, best_score_out, first_id_out, last_id_out, other_out, total_out});
}

bn_status bn_index_group_above_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, const float *min_score,
                                   uint64_t first_id, uint64_t n_ids, size_t n_groups, size_t g_stride, uint32_t *count_out, uint64_t *best_id_out,
                                   float *best_score_out, uint64_t *first_id_out, uint64_t *last_id_out, uint32_t *other_out, uint32_t *total_out) {
    return group(x, bn::QuerySource::stored(query_ids, exclude_radius), n_queries, min_score, first_id, n_ids, n_groups, g_stride,
                 Outputs{count_out, best_id_out, best_score_out, first_id_out, last_id_out, other_out, total_out});
}

}  // extern "C"
