"""bn_index_group_above restated in numpy from include/birdnet_hip.h alone, on top of above_ref.hit_mask (what a hit is) and
index_ref.scores64: per (query, group) the number of hits whose tag is the group, the hit with the highest score (ties: the lowest id;
-0.0 == +0.0), the smallest and the largest id; the hits whose tag is >= n_groups counted apart; the total.  Pure numpy, every query at
once; shared by test_group_above_cpu.py (self-checks against a literal double loop) and test_gpu_group_above.py (the expected value of
every GPU comparison)."""
import numpy as np

import above_ref
import index_ref as ir

NO_ROW = 0xFFFFFFFFFFFFFFFF
NAMES = ("counts", "best_ids", "best_scores", "first_ids", "last_ids", "other", "total")


def records(hit, S, tags, n_groups, g_stride=None):
    """the binding's seven outputs for the hit mask [nq, n]: (counts u32, best_ids u64, best_scores f32, first_ids u64, last_ids u64
    [nq, g_stride], other u32, total u32 [nq]).  Entries past n_groups are as the binding leaves them (count 0, ids NO_ROW, score NaN);
    a group without hits has count 0, ids NO_ROW and score 0.0.  S: scores [nq, n], used as f32; tags: the tag of every row [n], or
    None for an index that never tagged"""
    hit = np.asarray(hit, dtype=bool)
    nq, n = hit.shape
    g_stride = n_groups if g_stride is None else g_stride
    assert 1 <= n_groups <= 65536 and g_stride >= n_groups
    S32 = np.asarray(S).astype(np.float32)
    tags = np.zeros(n, dtype=np.int64) if tags is None else np.asarray(tags).astype(np.int64)
    q, r = np.nonzero(hit)                                   # pairs in (query, id) ascending order
    grouped = tags[r] < n_groups
    total = np.bincount(q, minlength=nq).astype(np.uint32)
    other = np.bincount(q[~grouped], minlength=nq).astype(np.uint32)
    q, r = q[grouped], r[grouped]
    slot = q * n_groups + tags[r]                            # the record of the pair
    slots = nq * n_groups
    s = S32[q, r]
    counts = np.bincount(slot, minlength=slots).astype(np.uint32)
    none = np.uint64(NO_ROW)
    first = np.full(slots, none, dtype=np.uint64)
    last = np.full(slots, none, dtype=np.uint64)
    last[slot] = r                                           # of a repeated index the last value is the one assigned: the largest id
    first[slot[::-1]] = r[::-1]                              # and in reverse the smallest
    top = np.full(slots, -np.inf, dtype=np.float32)
    np.maximum.at(top, slot, s)
    at_top = s == top[slot]                                  # == : -0.0 ties with +0.0
    best = np.full(slots, none, dtype=np.uint64)
    best[slot[at_top][::-1]] = r[at_top][::-1]               # the lowest id among the hits that reach the group's maximum
    best_s = np.zeros(slots, dtype=np.float32)
    have = counts > 0
    best_s[have] = S32[np.arange(slots)[have] // n_groups, best[have].astype(np.int64)]   # that hit's own bits

    def laid(a, fill):
        out = np.full((nq, g_stride), fill, dtype=a.dtype)
        out[:, :n_groups] = a.reshape(nq, n_groups)
        return out

    return laid(counts, 0), laid(best, none), laid(best_s, np.nan), laid(first, none), laid(last, none), other, total


def from_scores(S, qbad, xbad, min_score, n_groups, tags=None, first_id=0, n_ids=0, qid=None, exclude_radius=-1, g_stride=None):
    hit = above_ref.hit_mask(S, qbad, xbad, min_score, first_id, n_ids, qid, exclude_radius)
    return records(hit, S, tags, n_groups, g_stride)


def group_above(Q, X, min_score, n_groups, tags=None, first_id=0, n_ids=0, qid=None, exclude_radius=-1, g_stride=None):
    """the whole contract from rows: float64 scores of Q against X (exact for dyadic rows), then the rule"""
    S, qbad, xbad = ir.scores64(Q, X)
    return from_scores(S, qbad, xbad, min_score, n_groups, tags, first_id, n_ids, qid, exclude_radius, g_stride)


def narrowed(full, hit, tags, n_groups, nq=None, g_stride=None):
    """records(..., n_groups) of the first nq queries from `full` = records(..., 65536) of the same hits: a group is its tag, so the
    records of the groups below n_groups are the same; what changes is which hits belong to no group, counted here from the mask"""
    nq = len(full[5]) if nq is None else nq
    g_stride = n_groups if g_stride is None else g_stride
    tags = np.zeros(hit.shape[1], dtype=np.int64) if tags is None else np.asarray(tags)
    fills = (0, np.uint64(NO_ROW), np.nan, np.uint64(NO_ROW), np.uint64(NO_ROW))
    out = []
    for a, fill in zip(full[:5], fills):
        o = np.full((nq, g_stride), fill, dtype=a.dtype)
        o[:, :n_groups] = a[:nq, :n_groups]
        out.append(o)
    other = hit[:nq][:, tags >= n_groups].sum(axis=1).astype(np.uint32)
    return (*out, other, full[6][:nq].copy())


def assert_same(got, want, what):
    """seven arrays against seven arrays, every byte (NaN fills included)"""
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
            where = np.argwhere(gv != wv)[0]
            raise AssertionError((what, name, "at", tuple(int(i) for i in where), "got", g[tuple(where)], "want", w[tuple(where)]))
