"""bn_index_search_above restated in numpy from include/birdnet_hip.h alone, on top of index_ref.scores64: per query the ascending ids of
the rows of an id range that are valid, outside the exclusion radius of the query's own id and score at least min_score as an f32
comparison; their f32 scores; the total count; and the first max_hits of them as the binding lays them out.  Pure numpy; shared by
test_above_cpu.py (self-checks against a literal double loop) and test_gpu_above.py (the expected value of every GPU comparison)."""
import numpy as np

import index_ref as ir


def id_range(n, first_id=0, n_ids=0):
    """[lo, hi) of rows [first_id, first_id + n_ids), n_ids == 0: to the end; raises where the call refuses"""
    if first_id > n or n_ids > n - first_id:
        raise ValueError("rows [%d, +%d) run past the index's %d rows" % (first_id, n_ids, n))
    return first_id, first_id + n_ids if n_ids else n


def hit_mask(S, qbad, xbad, min_score, first_id=0, n_ids=0, qid=None, exclude_radius=-1):
    """bool [nq, n]: pair (q, r) is a hit.  S: scores [nq, n] (float64 of exact data, or f32); the comparison is made in f32"""
    S32 = np.asarray(S).astype(np.float32)
    nq, n = S32.shape
    thr = np.broadcast_to(np.asarray(min_score, dtype=np.float32).reshape(-1), (nq,))
    assert not np.isnan(thr).any(), "a NaN min_score is refused"
    lo, hi = id_range(n, first_id, n_ids)
    r = np.arange(n, dtype=np.int64)
    hit = ~np.asarray(qbad, dtype=bool)[:, None] & ~np.asarray(xbad, dtype=bool)[None, :] & ((r >= lo) & (r < hi))[None, :]
    if qid is not None and exclude_radius >= 0:
        hit &= np.abs(r[None, :] - np.asarray(qid, dtype=np.int64)[:, None]) > exclude_radius
    with np.errstate(invalid="ignore"):
        hit &= S32 >= thr[:, None]
    return hit


def hits_from_scores(S, qbad, xbad, min_score, first_id=0, n_ids=0, qid=None, exclude_radius=-1):
    """[(ids int64 ascending, scores f32)] per query: every hit, untruncated"""
    hit = hit_mask(S, qbad, xbad, min_score, first_id, n_ids, qid, exclude_radius)
    S32 = np.asarray(S).astype(np.float32)
    out = []
    for q in range(hit.shape[0]):
        ids = np.flatnonzero(hit[q])
        out.append((ids, S32[q, ids]))
    return out


def layout(hits, max_hits, h_stride=None, tags=None):
    """the binding's outputs for the per-query hit lists: (ids [nq, h_stride] uint64, scores f32, tags uint32, counts [nq] uint32): the
    first max_hits hits of each query; entries past them as the binding leaves them (id 0, score NaN, tag 0); counts untruncated.
    tags: the tag of every row [n], or None for an index that never tagged"""
    h_stride = max_hits if h_stride is None else h_stride
    nq = len(hits)
    ids = np.zeros((nq, h_stride), dtype=np.uint64)
    scores = np.full((nq, h_stride), np.nan, dtype=np.float32)
    tg = np.zeros((nq, h_stride), dtype=np.uint32)
    counts = np.zeros(nq, dtype=np.uint32)
    for q, (i, s) in enumerate(hits):
        counts[q] = len(i)
        k = min(len(i), max_hits)
        ids[q, :k], scores[q, :k] = i[:k], s[:k]
        if tags is not None:
            tg[q, :k] = np.asarray(tags)[i[:k]]
    return ids, scores, tg, counts


def search_above(Q, X, min_score, max_hits, first_id=0, n_ids=0, qid=None, exclude_radius=-1, h_stride=None, tags=None):
    """the whole contract from rows: float64 scores of Q against X (exact for dyadic rows), then the rule"""
    S, qbad, xbad = ir.scores64(Q, X)
    return layout(hits_from_scores(S, qbad, xbad, min_score, first_id, n_ids, qid, exclude_radius), max_hits, h_stride, tags)
