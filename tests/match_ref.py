"""The rules of a match against an attached index (bn_ctx_attach_index / bn_index_match) restated in numpy on top of index_ref.py:
the result is the prefix of the exact top-M list whose f32 scores are >= min_score, and every hit carries the tag of its row.
Pure numpy; shared by test_match_cpu.py, test_gpu_match.py and test_gpu_match_step.py."""
import numpy as np

import index_ref


def prefix(ids, scores, counts, min_score=None, tags=None):
    """The thresholded prefix of top-M lists (ids [nq, M] uint64, scores [nq, M] float32, counts [nq]) as a search returns them,
    score descending: (ids, scores, tags [nq, M] uint32, counts) with entries past a count as the binding leaves them (id 0,
    score NaN, tag 0).  tags: the tag of every row of the index by id, None: all zero."""
    ids, scores, counts = np.array(ids, dtype=np.uint64), np.array(scores, dtype=np.float32), np.array(counts, dtype=np.uint32)
    M = ids.shape[1]
    inside = np.arange(M)[None, :] < counts[:, None]
    if min_score is not None:
        with np.errstate(invalid="ignore"):
            keep = inside & (scores >= np.float32(min_score))
        # the lists are sorted: the kept entries are a prefix
        assert np.array_equal(keep, np.arange(M)[None, :] < keep.sum(axis=1)[:, None])
        inside = keep
    counts = inside.sum(axis=1).astype(np.uint32)
    ids[~inside] = 0
    scores[~inside] = np.nan
    out_tags = np.zeros(ids.shape, dtype=np.uint32)
    if tags is not None:
        out_tags[inside] = np.asarray(tags, dtype=np.uint32)[ids[inside].astype(np.int64)]
    return ids, scores, out_tags, counts


def match_exact(Q, X, M, min_score=None, tags=None, invalid=None):
    """The contract computed in float64: index_ref.top_m_exact, cut where the score falls below min_score, with the rows' tags"""
    return prefix(*index_ref.top_m_exact(Q, X, M, invalid=invalid), min_score=min_score, tags=tags)


def same(got, want):
    """None if two (ids, scores, tags, counts) results agree in counts and, inside them, in ids, score bits and tags; else what differs"""
    gi, gs, gt, gc = got
    wi, ws, wt, wc = want
    if not np.array_equal(gc, wc):
        return "counts differ at %s" % np.flatnonzero(np.asarray(gc) != np.asarray(wc))[:8]
    inside = np.arange(wi.shape[1])[None, :] < np.asarray(wc)[:, None]
    for name, g, w in (("ids", gi, wi), ("score bits", np.asarray(gs, dtype=np.float32).view(np.uint32), np.asarray(ws, dtype=np.float32).view(np.uint32)),
                       ("tags", gt, wt)):
        bad = inside & (np.asarray(g) != np.asarray(w))
        if bad.any():
            return "%s differ at %s" % (name, np.argwhere(bad)[:8].tolist())
    return None
