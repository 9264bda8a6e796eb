"""The rules of bn_ivf_* (include/birdnet_hip.h) that need no score arithmetic, in numpy: which lists a query probes, and the top-M
of a score matrix restricted to the probed lists' rows.  Scores are never computed here: the GPU tests take centroid scores from
bn_head_apply_host of a head with W = centroids and flags 0, and row scores from index_ref.scores64 (dyadic rows) or from
bn_index_search itself.  Also the skewed-lists data set of tests/test_gpu_ivf.py, so that a CPU test can check its structure."""
import numpy as np

import index_ref as ir

NONE = 0xFFFFFFFF


def probes(Z, nprobe, qvalid=None):
    """Z [nq, k] f32 centroid scores -> probes [nq, nprobe] uint32: the centroids by score descending, ties to the lowest index
    (-0.0 == +0.0), a NaN never; NONE in the slots no centroid reaches and in every slot of an invalid query"""
    Z = np.asarray(Z, dtype=np.float32)
    nq, k = Z.shape
    out = np.full((nq, nprobe), NONE, dtype=np.uint32)
    for q in range(nq):
        if qvalid is not None and not qvalid[q]:
            continue
        ok = np.flatnonzero(~np.isnan(Z[q]))
        order = ok[np.argsort(-(Z[q, ok] + np.float32(0.0)), kind="stable")][:nprobe]  # stable: equal scores stay in index order
        out[q, :len(order)] = order
    return out


def scanned(P, sizes):
    """the probed lists' sizes summed -> [nq] uint64"""
    sizes = np.asarray(sizes, dtype=np.uint64)
    return np.array([sizes[p[p != NONE]].sum() for p in np.asarray(P)], dtype=np.uint64)


def lists_of(assign, k):
    """the member lists of an assignment: per centroid its rows' ids ascending"""
    assign = np.asarray(assign)
    return [np.flatnonzero(assign == c).astype(np.uint64) for c in range(k)]


def restricted_top_m(S, qbad, xbad, assign, P, M, excluded=None, covered=None):
    """index_ref.top_m_from_scores of the score matrix S [nq, n] with only the rows of each query's probed lists eligible: rows whose
    assignment is among P[q], with an id below `covered`, outside excluded[q] (bool [nq, n])"""
    S = np.asarray(S)
    nq, n = S.shape
    assign = np.asarray(assign)
    assert len(assign) == n
    ids = np.zeros((nq, M), dtype=np.uint64)
    scores = np.full((nq, M), np.nan, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    below = np.arange(n) < (n if covered is None else covered)
    for q in range(nq):
        p = P[q][P[q] != NONE]
        out = ~(np.isin(assign, p) & (assign != NONE) & below)
        if excluded is not None:
            out = out | excluded[q]
        i, s, c = ir.top_m_from_scores(S[q:q + 1], qbad[q:q + 1], xbad, M, out[None])
        ids[q], scores[q], counts[q] = i[0], s[0], c[0]
    return ids, scores, counts


# ---- the skewed-lists data set ------------------------------------------------------------------------------------------------
SKEW_K = 12
SKEW_SIZES = (0, 64, 65, 1, 0, 100, 200, 37, 128, 300, 10, 0)  # list 0 takes the rest; lists 4 and 11 stay empty
SKEW_ROWS = 6000


def skewed_case(dim):
    """(X [SKEW_ROWS + 3, dim] raw rows, centroids [12, dim], want sizes [12], Q [70, dim] raw queries).  Centroid c is the unit
    vector e_c; a row of list c is e_c plus noise of norm about 0.3, so its score against its own centroid is near 0.95 and against
    any other below 0.15: no rounding moves a row.  The last three rows are a zero row, a NaN row and an Inf row."""
    rng = np.random.default_rng(4000 + dim)
    sizes = list(SKEW_SIZES)
    sizes[0] = SKEW_ROWS - sum(sizes)
    label = np.repeat(np.arange(SKEW_K), sizes)
    rng.shuffle(label)
    cent = np.zeros((SKEW_K, dim), dtype=np.float32)
    cent[np.arange(SKEW_K), np.arange(SKEW_K)] = 1.0
    X = (cent[label] + rng.standard_normal((SKEW_ROWS, dim)) * (0.3 / np.sqrt(dim))).astype(np.float32)
    X *= rng.uniform(0.5, 2.0, (SKEW_ROWS, 1)).astype(np.float32)
    bad = np.zeros((3, dim), dtype=np.float32)
    bad[1] = X[1]
    bad[1, dim // 2] = np.nan
    bad[2] = X[2]
    bad[2, 0] = np.inf
    X = np.concatenate([X, bad])
    # queries: mixtures of two or three centroid directions, so that the probe order differs from query to query; some stored rows
    w = rng.uniform(0.2, 1.0, (70, SKEW_K)) * (rng.random((70, SKEW_K)) < 0.25)
    w[np.arange(70), rng.integers(0, SKEW_K, 70)] += 1.0
    Q = (w @ cent + rng.standard_normal((70, dim)) * (0.3 / np.sqrt(dim))).astype(np.float32)
    Q[5:15] = X[rng.integers(0, SKEW_ROWS, 10)]
    return X, cent, np.array(sizes, dtype=np.uint32), Q
