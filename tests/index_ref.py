"""Inputs on which the embedding index's f32 cosine carries no rounding at all, and the exact top-M they imply.

A dyadic row has exactly nnz = 4^j non-zero elements, each +-1: its f32 sum of squares is 4^j, its norm 2^j, every stored
element +-2^-j.  Against a query built the same way every product is +-4^-j and every partial sum, in any order, an integer
multiple of 4^-j of magnitude <= 1: the f32 score equals the float64 score bit for bit, takes one of 2 * nnz + 1 values, and the
expected top-M is a plain sort with ties by id -- compared with ==, never within a tolerance.  Pure numpy; shared by
test_index_ref_cpu.py (which asserts the premise) and test_gpu_index_exact.py."""
import numpy as np

_CHUNK = 32768  # rows per block of the generators and of the float64 reference


def level_shift(nnz):
    """j of nnz = 4^j; raises for any other nnz"""
    j = 0
    while 4 ** j < nnz:
        j += 1
    if nnz < 1 or 4 ** j != nnz:
        raise ValueError("nnz must be a power of 4, got %d" % nnz)
    return j


def stored(X, nnz):
    """what the index stores for valid dyadic rows X: +-2^-j, exactly"""
    return (np.asarray(X, dtype=np.float32) * np.float32(2.0 ** -level_shift(nnz))).astype(np.float32)


def canonical_query(dim, nnz):
    level_shift(nnz)
    if nnz > dim:
        raise ValueError("nnz %d > dim %d" % (nnz, dim))
    q = np.zeros(dim, dtype=np.float32)
    q[:nnz] = 1
    return q


def dyadic_rows(rng, n, dim, nnz):
    """[n, dim] f32 rows of exactly nnz non-zeros, each +-1, at positions uniform over the nnz-subsets of the row"""
    level_shift(nnz)
    if nnz > dim:
        raise ValueError("nnz %d > dim %d" % (nnz, dim))
    X = np.zeros((n, dim), dtype=np.float32)
    for a in range(0, n, _CHUNK):
        b = min(n, a + _CHUNK)
        if nnz == dim:
            pos = np.broadcast_to(np.arange(dim), (b - a, dim))
        else:
            pos = np.argpartition(rng.random((b - a, dim), dtype=np.float32), nnz - 1, axis=1)[:, :nnz]
        sign = rng.integers(0, 2, (b - a, nnz), dtype=np.int8) * 2 - 1
        np.put_along_axis(X[a:b], pos, sign.astype(np.float32), axis=1)
    return X


def rows_at_levels(rng, levels, dim, nnz):
    """Dyadic rows whose score against canonical_query(dim, nnz) is levels[i] / nnz exactly.

    Row i agrees with the query on a positions of its support and disagrees on b, a - b = levels[i]; its other nnz - a - b
    non-zeros (random signs) lie outside the support, which has room for dim - nnz of them.  a + b is the smallest sum that
    fits; the positions are random.  Raises ValueError when a level cannot be reached at this (dim, nnz)."""
    level_shift(nnz)
    if nnz > dim:
        raise ValueError("nnz %d > dim %d" % (nnz, dim))
    lv = np.asarray(levels, dtype=np.int64).reshape(-1)
    n, room = lv.shape[0], dim - nnz
    s = np.maximum(np.abs(lv), nnz - room)      # a + b: at least |level|, and at most `room` non-zeros may leave the support
    s = s + ((s - lv) & 1)                      # a - b = level needs a + b of the level's parity
    bad = s > nnz
    if bad.any():
        raise ValueError("level(s) %s not reachable at dim=%d nnz=%d" % (sorted(set(lv[bad].tolist()))[:8], dim, nnz))
    a, b = (s + lv) // 2, (s - lv) // 2
    X = np.zeros((n, dim), dtype=np.float32)
    for r0 in range(0, n, _CHUNK):
        r1 = min(n, r0 + _CHUNK)
        k = np.arange(nnz)[None, :]
        inside = np.where(k < a[r0:r1, None], 1, np.where(k < s[r0:r1, None], -1, 0)).astype(np.float32)
        X[r0:r1, :nnz] = rng.permuted(inside, axis=1)
        if room:
            k = np.arange(room)[None, :]
            sign = (rng.integers(0, 2, (r1 - r0, room), dtype=np.int8) * 2 - 1).astype(np.float32)
            outside = np.where(k < (nnz - s[r0:r1, None]), sign, np.float32(0))
            X[r0:r1, nnz:] = rng.permuted(outside, axis=1)
    return X


def unit64(A):
    """float64 unit rows and the mask of rows the index may never return or search with: a non-finite element or zero norm"""
    A = np.asarray(A)
    with np.errstate(all="ignore"):
        fin = np.isfinite(A).all(axis=1)
        A64 = A.astype(np.float64)
        A64[~fin] = 0
        nrm = np.sqrt((A64 * A64).sum(axis=1))
        bad = ~fin | (nrm == 0)
        U = A64 / np.where(bad, 1.0, nrm)[:, None]
    U[bad] = 0
    return U, bad


def scores64(Q, X):
    """float64 cosine [nq, n] (zeros where a side is invalid), the invalid-query and the invalid-row masks"""
    Qu, qbad = unit64(Q)
    n = len(X)
    S = np.empty((len(Qu), n), dtype=np.float64)
    xbad = np.empty(n, dtype=bool)
    for a in range(0, n, _CHUNK):
        Xu, xbad[a:a + _CHUNK] = unit64(X[a:a + _CHUNK])
        S[:, a:a + _CHUNK] = Qu @ Xu.T + 0.0                # + 0.0: -0.0 and +0.0 are one score
    return S, qbad, xbad


def top_m_from_scores(S, qbad, xbad, M, excluded=None):
    """top_m_exact from the output of scores64 (so that several searches over one row set share one float64 product)"""
    nq, n = S.shape
    ids = np.zeros((nq, M), dtype=np.uint64)
    scores = np.full((nq, M), np.nan, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        if qbad[q]:
            continue
        out = xbad
        if excluded is not None:
            ex = excluded[q]
            if getattr(ex, "dtype", None) == np.bool_:
                out = xbad | ex
            else:
                out = xbad.copy()
                out[np.asarray(ex, dtype=np.int64)] = True
        key = np.where(out, -np.inf, S[q])
        cand = np.arange(n)
        if n > 4 * M:                                       # only rows at or above the M-th largest key can be returned
            cand = np.flatnonzero(key >= np.partition(key, n - M)[n - M])
        order = cand[np.argsort(-key[cand], kind="stable")][:M]  # stable: equal scores stay in id order
        c = int(min(M, n - int(out.sum())))
        counts[q] = c
        ids[q, :c] = order[:c]
        scores[q, :c] = S[q, order[:c]].astype(np.float32)
    return ids, scores, counts


def top_m_exact(Q, X, M, excluded=None, invalid=None):
    """The index's contract computed in float64: (ids [nq, M] uint64, scores [nq, M] float32, counts [nq] uint32), score
    descending and ties by id ascending, entries past a count left as the binding leaves them (id 0, score NaN).

    Rows with a non-finite element or zero norm are never returned, nor are rows set in `invalid` (bool [n]); a query of that
    kind has count 0.  excluded: bool [nq, n], or one id array per query."""
    S, qbad, xbad = scores64(Q, X)
    if invalid is not None:
        xbad = xbad | np.asarray(invalid, dtype=bool)
    return top_m_from_scores(S, qbad, xbad, M, excluded)


def f32_scores_in_order(Qn, Xn, order):
    """[nq, n] scores of f32 rows accumulated in f32, one rounded product and one rounded add at a time, in the k order given"""
    Qn, Xn = np.asarray(Qn, dtype=np.float32), np.asarray(Xn, dtype=np.float32)
    acc = np.zeros((Qn.shape[0], Xn.shape[0]), dtype=np.float32)
    for k in order:
        acc = acc + Qn[:, k, None] * Xn[None, :, k]
    assert acc.dtype == np.float32
    return acc
