"""The rules of bn_sq8_* (include/birdnet_hip.h) in numpy: the int8 code and the scale of a stored row, the coarse key of a (query,
row) pair, which rows become a query's candidates, and the top-M of a score matrix restricted to them.  Exact scores are never
computed here: the GPU tests take them from bn_index_search itself (or from index_ref.scores64 for dyadic rows)."""
import numpy as np

import index_ref as ir


def codes(stored):
    """stored [n, dim] f32 rows as bn_index_read returns them -> (codes [n, dim] int8, scales [n] f32).  a = max |r[k]|; an all-zero
    row has codes 0 and scale +0.0; otherwise inv = 127 / a in f32, code = clamp(rint(r * inv), -127, 127) with one f32 multiply and
    rint to nearest-even, scale = a / 127 in f32"""
    r = np.ascontiguousarray(stored, dtype=np.float32)
    a = np.abs(r).max(axis=1) if r.shape[1] else np.zeros(len(r), dtype=np.float32)
    ok = a > 0
    with np.errstate(all="ignore"):
        inv = np.where(ok, np.float32(127.0) / np.where(ok, a, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        prod = r * inv[:, None]
    assert prod.dtype == np.float32
    c = np.clip(np.rint(prod), np.float32(-127.0), np.float32(127.0)).astype(np.int8)
    c[~ok] = 0
    scales = np.where(ok, a / np.float32(127.0), np.float32(0.0)).astype(np.float32)
    return c, scales


def keys(qcodes, rcodes, scales):
    """[nq, n] f32: D = sum_k qcode[k] * code[k] in int32, key = (float)D * scale_row (int -> f32 to nearest, then one f32 multiply).
    The integer sum is formed by a float64 matrix product: every product and every partial sum is an integer below 2^31 < 2^53, so
    that product IS the integer sum, in any order; it is then checked to fit int32 and held as int32."""
    q = np.asarray(qcodes, dtype=np.int8).astype(np.float64)
    c = np.asarray(rcodes, dtype=np.int8).astype(np.float64)
    D = np.zeros((q.shape[0], c.shape[0]), dtype=np.int32)
    for a in range(0, c.shape[0], 32768):
        d = q @ c[a:a + 32768].T
        assert (np.abs(d) < 2.0 ** 31).all() and (d == np.rint(d)).all()
        D[:, a:a + 32768] = d.astype(np.int64).astype(np.int32)
    k = D.astype(np.float32) * np.asarray(scales, dtype=np.float32)[None, :]
    assert D.dtype == np.int32 and k.dtype == np.float32
    return k


def candidates(K, eligible, refine):
    """K [nq, n] keys, eligible bool [nq, n] -> (cands [nq, refine] uint64 zero-filled, counts [nq] uint32): the first `refine` eligible
    rows by key descending, ties by id ascending"""
    K = np.asarray(K, dtype=np.float32)
    nq, n = K.shape
    cands = np.zeros((nq, refine), dtype=np.uint64)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        ok = np.flatnonzero(eligible[q])
        order = ok[np.argsort(-(K[q, ok] + np.float32(0.0)), kind="stable")][:refine]  # stable: equal keys stay in id order
        cands[q, :len(order)] = order
        counts[q] = len(order)
    return cands, counts


def eligible(qbad, xbad, n_covered=None, excluded=None):
    """bool [nq, n]: valid query, valid row, id below n_covered, outside excluded [nq, n]"""
    qbad, xbad = np.asarray(qbad, dtype=bool), np.asarray(xbad, dtype=bool)
    e = ~qbad[:, None] & ~xbad[None, :]
    if n_covered is not None:
        e = e & (np.arange(len(xbad)) < n_covered)[None, :]
    if excluded is not None:
        e = e & ~excluded
    return e


def restricted_top_m(S, cands, cand_counts, M):
    """S [nq, n] score matrix -> (ids [nq, M] uint64, scores [nq, M] f32, counts [nq] uint32): the candidates by score descending, ties
    by id ascending; entries past a count as the binding leaves them (id 0, score NaN)"""
    S = np.asarray(S)
    nq = S.shape[0]
    ids = np.zeros((nq, M), dtype=np.uint64)
    scores = np.full((nq, M), np.nan, dtype=np.float32)
    counts = np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        c = np.sort(np.asarray(cands[q, :cand_counts[q]], dtype=np.int64))
        s = S[q, c].astype(np.float32)
        order = c[np.argsort(-(s + np.float32(0.0)), kind="stable")][:M]
        counts[q] = len(order)
        ids[q, :len(order)] = order
        scores[q, :len(order)] = S[q, order].astype(np.float32)
    return ids, scores, counts


class Expected:
    """everything searches should return, from the stored rows [n, dim], the staged queries [nq, dim] and the score matrix S: the
    candidates are computed once at refine = 256, a smaller refine takes their prefix"""

    def __init__(self, stored, qstored, S, n_covered=None, excluded=None):
        stored, qstored = np.asarray(stored, dtype=np.float32), np.asarray(qstored, dtype=np.float32)
        xbad, qbad = ~(stored != 0).any(axis=1), ~(qstored != 0).any(axis=1)
        rc, rs = codes(stored)
        qc, _ = codes(qstored)
        self.S = S
        self.cands, self.cc = candidates(keys(qc, rc, rs), eligible(qbad, xbad, n_covered, excluded), 256)

    def at(self, refine, M):
        """(ids, scores, counts, cands [nq, refine], cand_counts)"""
        cands = self.cands[:, :refine].copy()
        cc = np.minimum(self.cc, refine).astype(np.uint32)
        return restricted_top_m(self.S, cands, cc, M) + (cands, cc)


def expected(stored, qstored, S, refine, M, n_covered=None, excluded=None):
    return Expected(stored, qstored, S, n_covered, excluded).at(refine, M)


def tight_case():
    """6 000 rows and 16 queries of dim 6, all one base vector + 0.02 Gaussian: 8-bit codes cannot tell the rows apart"""
    rng = np.random.default_rng(5)
    base = rng.standard_normal(6)
    X = (base + 0.02 * rng.standard_normal((6000, 6))).astype(np.float32)
    Q = (base + 0.02 * rng.standard_normal((16, 6))).astype(np.float32)
    return X, Q


def normalised(A):
    """f32 unit rows close to what the index stores (not its bits: for CPU-side statements that have room to spare)"""
    U, bad = ir.unit64(A)
    return U.astype(np.float32), bad
