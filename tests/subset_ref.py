"""bn_subset_* restated in numpy from include/birdnet_hip.h alone: which rows a filter selects, and what a search over a list of
rows returns given the score of every (query, row) pair.  Pure numpy; shared by test_subset_cpu.py (self-checks on hand-made cases)
and test_gpu_subset.py (the expected value of every GPU comparison)."""
import numpy as np

TAG_LIMIT = 65536
EXCLUDE_TAGS = 1


class Filter:
    """bn_index_filter: the id range [first_id, first_id + n_ids) (n_ids 0: to the end of the index), a tag list (None or empty: tags
    are not tested) and flags (0, or EXCLUDE_TAGS: the list names the tags left out)"""

    def __init__(self, first_id=0, n_ids=0, tags=None, flags=0):
        self.first_id, self.n_ids, self.tags, self.flags = int(first_id), int(n_ids), tags, int(flags)


def members(tags, size, f):
    """the ids, ascending (uint64), of the rows of an index of `size` rows with row tags `tags` [size] that filter f selects; raises
    ValueError where the header refuses the filter"""
    tags = np.asarray(tags, dtype=np.int64).reshape(-1)
    if len(tags) != size:
        raise ValueError("one tag per row")
    if f.flags & ~EXCLUDE_TAGS:
        raise ValueError("unknown flags")
    listed = np.zeros(0, dtype=np.int64) if f.tags is None else np.asarray(f.tags, dtype=np.int64).reshape(-1)
    if (listed < 0).any() or (listed >= TAG_LIMIT).any():
        raise ValueError("a listed tag at or above the limit")
    if f.first_id < 0 or f.n_ids < 0 or f.first_id > size or f.n_ids > size - f.first_id:
        raise ValueError("range past the index")
    end = f.first_id + f.n_ids if f.n_ids else size
    ids = np.arange(size, dtype=np.int64)
    keep = (ids >= f.first_id) & (ids < end)
    if len(listed):
        named = np.isin(tags, listed)
        keep &= ~named if f.flags & EXCLUDE_TAGS else named
    return ids[keep].astype(np.uint64)


def restricted_top_m(S, qbad, xbad, members, M, qid=None, radius=-1):
    """What a search over the list `members` returns.  S [nq, n]: the score of every (query, row) pair; qbad [nq] / xbad [n]: the
    invalid queries / rows (never searched with / never returned).  qid [nq] with radius >= 0: rows whose id lies within radius of
    the query's own id are skipped.  -> (ids [nq, M] uint64, scores [nq, M] of S's dtype as f32, counts [nq] uint32): the valid members
    not excluded by score descending (-0.0 == +0.0), ties by id ascending; count = min(M, their number); entries past a count as the
    binding leaves them (id 0, score NaN)."""
    S = np.asarray(S)
    nq = S.shape[0]
    mem = np.sort(np.asarray(members, dtype=np.int64).reshape(-1))
    if len(mem) > 1 and (np.diff(mem) <= 0).any():
        raise ValueError("members are not distinct")
    ids = np.zeros((nq, M), dtype=np.uint64)
    scores = np.full((nq, M), np.nan, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    ok_rows = mem[~np.asarray(xbad, dtype=bool)[mem]] if len(mem) else mem
    for q in range(nq):
        if qbad[q]:
            continue
        c = ok_rows
        if radius >= 0 and qid is not None:
            c = c[np.abs(c - int(qid[q])) > radius]
        key = S[q, c] + S.dtype.type(0.0)                      # -0.0 and +0.0 are one score
        order = c[np.argsort(-key, kind="stable")][:M]         # stable over ascending ids: equal scores stay in id order
        counts[q] = len(order)
        ids[q, :len(order)] = order
        scores[q, :len(order)] = S[q, order].astype(np.float32)
    return ids, scores, counts
