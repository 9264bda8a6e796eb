"""The two rules of bn_index_assign / bn_index_cluster (include/birdnet_hip.h) that need no score arithmetic, in numpy.  The scores
themselves are never computed here: the GPU tests take them from bn_head_apply_host of a head with W = centroids and flags 0."""
import numpy as np

NONE = 0xFFFFFFFF


def assign(Z, valid):
    """Z [n, k] f32 scores, valid [n] bool -> (assign [n] uint32, score [n] f32): the centroid of largest score, ties to the lowest
    index (-0.0 == +0.0), a NaN never wins; an invalid row or one whose scores are all NaN gets (NONE, NaN).  The score keeps the
    winner's own bits."""
    Z = np.asarray(Z, dtype=np.float32)
    n = Z.shape[0]
    nan = np.isnan(Z)
    # the first non-NaN entry equal to the row's maximum over its non-NaN entries (== makes -0.0 and +0.0 equal)
    masked = np.where(nan, -np.inf, Z)
    best = masked.max(axis=1, keepdims=True)
    first = np.argmax((masked == best) & ~nan, axis=1)
    has = np.asarray(valid, dtype=bool) & ~nan.all(axis=1)
    a = np.where(has, first, NONE).astype(np.uint32)
    s = np.where(has, Z[np.arange(n), first], np.float32(np.nan)).astype(np.float32)
    return a, s


def member_sums(S, a, k):
    """float64 sums of the member rows of every cluster, member by member in ascending id order -> (sums [k, dim], counts [k],
    abs sums [k, dim])"""
    S64 = np.asarray(S, dtype=np.float32).astype(np.float64)
    sums = np.zeros((k, S64.shape[1]))
    mags = np.zeros((k, S64.shape[1]))
    counts = np.zeros(k, dtype=np.uint32)
    for c in range(k):
        m = np.flatnonzero(np.asarray(a) == c)
        counts[c] = len(m)
        if len(m):
            sums[c] = np.cumsum(S64[m], axis=0)[-1]  # cumsum adds in order
            mags[c] = np.abs(S64[m]).sum(axis=0)
    return sums, counts, mags


def update(S, a, prev):
    """one centroid update: sum / float64 norm rounded to f32; a cluster with no members, or whose sum has zero or non-finite norm,
    keeps prev's row -> (centroids [k, dim] f32, kept [k] bool)"""
    prev = np.asarray(prev, dtype=np.float32)
    k = prev.shape[0]
    sums, counts, _ = member_sums(S, a, k)
    out = prev.copy()
    kept = np.ones(k, dtype=bool)
    for c in range(k):
        with np.errstate(all="ignore"):
            norm = np.sqrt((sums[c] * sums[c]).sum())
        if counts[c] and norm > 0 and np.isfinite(norm):
            out[c] = (sums[c] / norm).astype(np.float32)
            kept[c] = False
    return out, kept


def update_bound(S, a, k):
    """per component: the float64 centroid c64 and the header's bound 2^-24 |c64| + n_c 2^-52 (sum_members |x|) / |s| (clusters with
    members and a usable norm only; inf elsewhere)"""
    sums, counts, mags = member_sums(S, a, k)
    c64 = np.zeros_like(sums)
    bound = np.full_like(sums, np.inf)
    for c in range(k):
        norm = np.sqrt((sums[c] * sums[c]).sum())
        if counts[c] and norm > 0 and np.isfinite(norm):
            c64[c] = sums[c] / norm
            bound[c] = 2.0 ** -24 * np.abs(c64[c]) + float(counts[c]) * 2.0 ** -52 * mags[c] / norm
    return c64, bound
