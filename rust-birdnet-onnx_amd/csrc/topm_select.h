// Exact top-M selection shared by the scans that keep per-list candidates (index.hip: cosine search; rank.hip: ranking by a head's
// logits; subset.hip, peaks.hip, ivf.hip, sq8.hip): the candidate, its strict total orders, the merge of a pending list into a sorted
// running list by rank, and the walk that merges the workgroups' sorted lists into the final one.  Device code only; include from a
// .hip file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace bn {
namespace topm {

constexpr int MMAX = 256;  // largest top_m
constexpr int PEND = 128;  // pending candidates per list before they are merged into the running list

struct Cand {
    float s;  // the value returned to the caller (a score, a logit); the order below derives its key from it
    uint32_t id;
};

// The orders: strict and total over candidates with distinct ids and no NaN (the float compare makes -0.0 == +0.0).
struct ScoreDesc {  // s descending, ties by id ascending
    static __device__ inline bool ahead(Cand a, Cand b) { return a.s > b.s || (a.s == b.s && a.id < b.id); }
};
struct AbsAsc {  // |s| ascending, ties by id ascending: s and -s tie
    static __device__ inline bool ahead(Cand a, Cand b) {
        const float x = __builtin_fabsf(a.s), y = __builtin_fabsf(b.s);
        return x < y || (x == y && a.id < b.id);
    }
};

// LDS and global writes of this wave visible to its other lanes
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ inline int lanes_below(uint64_t m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One wave: merge np unordered pending candidates into the sorted running list (len entries), keeping the first M of the union.
// Every element's new position is its rank in the union (the order is strict: ids are distinct).  scratch: MMAX entries of
// LDS; *thr receives the M-th entry when the list is full.  Returns the new length.
template <class Ord>
__device__ inline int merge_pending(const Cand *pend, int np, Cand *list, int len, int M, Cand *scratch, Cand *thr) {
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < len; i += 64) scratch[i] = list[i];
    wave_sync();
    for (int i = lane; i < len; i += 64) {
        const Cand e = scratch[i];
        int r = i;
        for (int j = 0; j < np; j++) r += Ord::ahead(pend[j], e) ? 1 : 0;
        if (r < M) {
            list[r] = e;
            if (r == M - 1) *thr = e;
        }
    }
    for (int p = lane; p < np; p += 64) {
        const Cand e = pend[p];
        int r = 0;
        for (int j = 0; j < np; j++) r += Ord::ahead(pend[j], e) ? 1 : 0;
        int lo = 0, hi = len;  // list entries ahead of e: a prefix of the sorted list
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (Ord::ahead(scratch[mid], e)) lo = mid + 1;
            else hi = mid;
        }
        r += lo;
        if (r < M) {
            list[r] = e;
            if (r == M - 1) *thr = e;
        }
    }
    wave_sync();
    return min(M, len + np);
}

// One wave (a block of 64 threads) per list q: the n_wg workgroups' sorted lists cand[g][q][MMAX] (lengths cand_len[g][q], both
// with `lists` lists per workgroup) -> the final top-M out[q][M], count[q].  Each list is read only while its entries still beat
// the running M-th.
template <class Ord>
__device__ inline void merge_lists(const Cand *__restrict__ cand, const int *__restrict__ cand_len, int lists, int n_wg, int M,
                                   Cand *__restrict__ out, uint32_t *__restrict__ count) {
    __shared__ Cand list[MMAX], scratch[MMAX], pend[PEND];
    __shared__ Cand thr;
    const int q = blockIdx.x, lane = threadIdx.x;
    int len = 0, np = 0;
    for (int g = 0; g < n_wg; g++) {
        const Cand *src = cand + ((size_t)g * lists + q) * MMAX;
        const int lg = cand_len[g * lists + q];
        for (int j = 0; j < lg; j += 64) {
            const bool in = j + lane < lg;
            const Cand e = in ? src[j + lane] : Cand{0.f, 0u};
            const bool pass = in && (len < M || Ord::ahead(e, thr));
            const uint64_t m = __ballot(pass);
            if (!m) break;  // the list is sorted: nothing after a rejected entry can pass
            if (np + 64 > PEND) {
                len = merge_pending<Ord>(pend, np, list, len, M, scratch, &thr);
                np = 0;
            }
            if (pass) pend[np + lanes_below(m)] = e;
            np += __popcll(m);
            wave_sync();
        }
    }
    if (np) len = merge_pending<Ord>(pend, np, list, len, M, scratch, &thr);
    for (int i = lane; i < len; i += 64) out[(size_t)q * M + i] = list[i];
    if (lane == 0) count[q] = (uint32_t)len;
}

}  // namespace topm
}  // namespace bn
