"""bn_index_search_peaks restated in numpy from include/birdnet_hip.h alone: given the score of every (query, row) pair and which pairs
are eligible, the peaks of each query and the first M of them.  Pure numpy; shared by test_peaks_cpu.py (self-checks against a brute-force
double loop and the header's stated consequences) and test_gpu_peaks.py (the expected value of every GPU comparison)."""
import numpy as np


def peak_mask(S, eligible, radius):
    """bool [nq, n]: pair (q, i) is eligible and every other eligible row j with 0 < |i - j| <= radius comes after i in the order
    score descending, ties by id ascending (-0.0 == +0.0).  One pass per offset 1..radius, each looking once down and once up."""
    key = np.asarray(S) + np.asarray(S).dtype.type(0.0)          # -0.0 and +0.0 are one score
    el = np.asarray(eligible, dtype=bool)
    assert key.ndim == 2 and el.shape == key.shape
    n = key.shape[1]
    peak = el.copy()
    for d in range(1, min(int(radius), n - 1) + 1):
        # row i - d has the lower id: it comes before i unless its score is strictly smaller
        peak[:, d:] &= ~(el[:, :-d] & (key[:, :-d] >= key[:, d:]))
        # row i + d has the higher id: it comes before i only with a strictly larger score
        peak[:, :-d] &= ~(el[:, d:] & (key[:, d:] > key[:, :-d]))
    return peak


def peaks_top_m(S, eligible, radius, M):
    """-> (ids [nq, M] uint64, scores [nq, M] float32, counts [nq] uint32): the first M peaks of each query by score descending, ties
    by id ascending; count = min(M, peaks); entries past a count as the binding leaves them (id 0, score NaN)."""
    S = np.asarray(S)
    nq = S.shape[0]
    peak = peak_mask(S, eligible, radius)
    ids = np.zeros((nq, M), dtype=np.uint64)
    scores = np.full((nq, M), np.nan, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        c = np.flatnonzero(peak[q])
        key = S[q, c] + S.dtype.type(0.0)
        order = c[np.argsort(-key, kind="stable")][:M]           # stable over ascending ids: equal scores stay in id order
        counts[q] = len(order)
        ids[q, :len(order)] = order
        scores[q, :len(order)] = S[q, order].astype(np.float32)
    return ids, scores, counts


def eligibility(n, qbad, xbad, qid=None, exclude_radius=-1):
    """bool [nq, n]: the pairs bn_index_search (qid None) / bn_index_search_ids may return: query valid, row valid, and the row's id
    outside exclude_radius of the query's own"""
    qbad, xbad = np.asarray(qbad, dtype=bool), np.asarray(xbad, dtype=bool)
    el = ~qbad[:, None] & ~xbad[None, :n]
    if qid is not None and exclude_radius >= 0:
        d = np.arange(n, dtype=np.int64)[None, :] - np.asarray(qid, dtype=np.int64)[:, None]
        el &= np.abs(d) > exclude_radius
    return el
