"""bn_ivf_* on the GPU.  Every expected value comes from code older than the feature, or from tests/ivf_ref.py: member lists are cut
from Index.assign; probes are ivf_ref.probes over bn_head_apply_host of a head with W = centroids, no bias and flags 0 (on the
queries read back from a scratch index, or on the stored rows); row scores are index_ref.scores64 for dyadic rows and, for general
rows, the full score matrix bn_index_search itself gives (raw rows added in chunks of 256 to scratch indexes, searched with
top_m = 256 and scattered by id: tests/test_gpu_index_exact.py pins that a score's bits depend neither on position nor on index
size).  Counts, ids, probes, scanned and score bytes are compared with ==."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import cluster_ref
import index_ref as ir
import ivf_ref
import test_gpu_index_exact as exact
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
NONE = ivf_ref.NONE
INVALID_ARG = 1
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def _bn():
    return importlib.import_module("rust-birdnet-onnx_amd")


def twin_scores(bn, cent, rows):
    """the oracle's centroid scores: bn_head_apply_host of a head with W = centroids, no bias, flags 0"""
    return bn.Head(0, np.ascontiguousarray(cent, dtype=np.float32), None, l2norm=False).apply(np.ascontiguousarray(rows, dtype=np.float32))


def as_stored(bn, Q):
    """the queries as the index normalises them (read back from a scratch index) and the mask of the invalid ones"""
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    idx = bn.Index(0, Q.shape[1], len(Q))
    idx.add(Q)
    Qn = idx.read()
    return Qn, ~(Qn != 0).any(axis=1)


def search_matrix(bn, X, Q):
    """[nq, n] f32: the score bn_index_search gives every (query, row) pair; 0 where the row or the query is never returned"""
    S = np.zeros((len(Q), len(X)), dtype=np.float32)
    for a in range(0, len(X), 256):
        idx = bn.Index(0, X.shape[1], 256)
        idx.add(X[a:a + 256])
        ids, sc, cnt = idx.search(Q, 256)
        for q in range(len(Q)):
            S[q, a + ids[q, :cnt[q]].astype(np.int64)] = sc[q, :cnt[q]]
    return S


def assert_lists(ivf, assign, k, what=""):
    want = ivf_ref.lists_of(assign, k)
    sizes = ivf.list_sizes()
    assert sizes.dtype == np.uint32 and sizes.tolist() == [len(w) for w in want], what
    for c in range(k):
        got = ivf.read_list(c)
        assert got.dtype == np.uint64 and np.array_equal(got, want[c]), (what, c)


def assert_search(got, want_top, P, sizes, nq, M, what):
    """got = (ids, scores, counts, probes, scanned) of a search of the first nq queries; want_top the restricted top-256"""
    wi, ws, wc = want_top
    exact.assert_exact(got[:3], (wi[:nq, :M], ws[:nq, :M], np.minimum(wc[:nq], M).astype(np.uint32)), what)
    assert got[3].dtype == np.uint32 and np.array_equal(got[3], P[:nq]), (what, "probes")
    assert got[4].dtype == np.uint64 and np.array_equal(got[4], ivf_ref.scanned(P[:nq], sizes)), (what, "scanned")


# ---- 1. general data, skewed lists ------------------------------------------------------------------------------------------
class Skew:
    def __init__(self, dim):
        bn = _bn()
        self.X, self.cent, self.sizes, self.Q = ivf_ref.skewed_case(dim)
        self.n, self.k = len(self.X), len(self.cent)
        self.idx = bn.Index(0, dim, self.n)
        self.idx.add(self.X)
        self.stored = self.idx.read()
        self.xbad = ~(self.stored != 0).any(axis=1)
        self.assign, _ = self.idx.assign(self.cent)
        self.ivf = bn.Ivf(self.idx, self.cent)
        self.Qn, self.qbad = as_stored(bn, self.Q)
        self.Zq = twin_scores(bn, self.cent, self.Qn)
        self.S = search_matrix(bn, self.X, self.Q)


@functools.lru_cache(maxsize=None)
def skew(dim):
    return Skew(dim)


@pytest.mark.parametrize("dim", [130, 1536])
def test_general_data_skewed_lists(bn, dim):
    s = skew(dim)
    assert len(s.ivf) == s.k and s.ivf.rows == s.n
    assert_lists(s.ivf, s.assign, s.k, dim)
    sizes = s.ivf.list_sizes()
    # the structure the case is built for: many tiles and several segments, exactly one tile, one tile and a row, one row, none
    assert sizes.tolist() == s.sizes.tolist() and sizes[0] > 4900 and sizes[1] == 64 and sizes[2] == 65 and sizes[3] == 1 and sizes[4] == 0
    assert (s.assign[-3:] == NONE).all() and not s.qbad.any()
    for nprobe in (1, 2, 5, 12):
        P = ivf_ref.probes(s.Zq, nprobe, ~s.qbad)
        want = ivf_ref.restricted_top_m(s.S, s.qbad, s.xbad, s.assign, P, 256)
        for nq in (1, 17, 70):
            for M in (1, 64, 100, 256):
                assert_search(s.ivf.search(s.Q[:nq], nprobe, M), want, P, sizes, nq, M, (dim, "nprobe", nprobe, "Q", nq, "M", M))
    assert len(set(P[:, 0].tolist())) > 4, "the queries should not all probe the same list first"


# ---- 2. dyadic rows, heavy ties, many tiles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["constant", "sawtooth", "random"])
def test_dyadic_rows_heavy_ties(bn, order):
    case = exact.ordered_case(bn, order, 128, 64)
    rng = np.random.default_rng(77)
    cent = ir.dyadic_rows(rng, 5, 128, 64)
    assign, _ = case.idx.assign(cent)
    ivf = bn.Ivf(case.idx, cent)
    sizes = ivf.list_sizes()
    assert sizes.tolist() == np.bincount(assign[assign != NONE], minlength=5).tolist() and sizes.max() > 64 * 64
    assert np.array_equal(ivf.read_list(int(np.argmax(sizes))), np.flatnonzero(assign == np.argmax(sizes)))
    Qn, qbad = as_stored(bn, case.Q)
    assert np.array_equal(qbad, case.qbad)
    Zq = twin_scores(bn, cent, Qn)
    for nprobe in (1, 3, 5):
        P = ivf_ref.probes(Zq, nprobe, ~qbad)
        want = ivf_ref.restricted_top_m(case.S, case.qbad, case.xbad, assign, P, 256)
        for nq, M in ((70, 1), (70, 65), (70, 256), (1, 256), (17, 65)):
            assert_search(ivf.search(case.Q[:nq], nprobe, M), want, P, sizes, nq, M, (order, "nprobe", nprobe, "Q", nq, "M", M))


# ---- 3. nprobe == k ------------------------------------------------------------------------------------------------------------
def test_all_lists_probed_equals_the_exact_search(bn):
    s = skew(130)
    qids = [0, 1, 63, 64, 65, 2999, s.n - 4, s.n - 3, s.n - 1]
    for M in (1, 100, 256):
        got = s.ivf.search(s.Q, s.k, M)
        want = s.idx.search(s.Q, M)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want)), M
        assert (got[4] == s.n - 3).all()
        for radius in (-1, 3):
            got = s.ivf.search_ids(qids, s.k, M, exclude_radius=radius)
            want = s.idx.search_ids(qids, M, exclude_radius=radius)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want)), (M, radius)


# ---- 4. search_ids -------------------------------------------------------------------------------------------------------------
def test_search_ids_first_probe_and_exclusion(bn):
    s = skew(130)
    sizes = s.ivf.list_sizes()
    every = np.arange(s.n, dtype=np.uint64)
    ids, sc, cnt, probes, scanned = s.ivf.search_ids(every, 1, 1)
    assert np.array_equal(probes[:, 0], s.assign), "the first probe of a stored row is its assigned list"
    assert not cnt[-3:].any() and not scanned[-3:].any() and np.array_equal(ids[:-3, 0], every[:-3]), "a valid row finds itself first"
    rng = np.random.default_rng(5)
    qids = np.concatenate([[0, 1, 64, s.n - 4, s.n - 2], s.ivf.read_list(1)[:3], s.ivf.read_list(3), rng.integers(0, s.n - 3, 12)]).astype(np.uint64)
    S = search_matrix(bn, s.X, s.X[qids.astype(np.int64)])
    qbad = s.xbad[qids.astype(np.int64)]
    Zq = twin_scores(bn, s.cent, s.stored[qids.astype(np.int64)])
    for nprobe in (1, 3):
        P = ivf_ref.probes(Zq, nprobe, ~qbad)
        for radius in (-1, 0, 3):
            ex = None if radius < 0 else exact.radius_mask(qids, radius, s.n)
            want = ivf_ref.restricted_top_m(S, qbad, s.xbad, s.assign, P, 256, ex)
            for M in (1, 100, 256):
                got = s.ivf.search_ids(qids, nprobe, M, exclude_radius=radius)
                assert_search(got, want, P, sizes, len(qids), M, ("ids", "nprobe", nprobe, "radius", radius, "M", M))


# ---- 5. extend -----------------------------------------------------------------------------------------------------------------
def test_extend_covers_appended_rows(bn):
    s = skew(130)
    half = 2987                                   # inside a tile
    idx = bn.Index(0, 130, s.n)
    idx.add(s.X[:half])
    ivf = bn.Ivf(idx, s.cent)
    idx.add(s.X[half:4000])
    idx.add(s.X[4000:])
    assert ivf.rows == half and len(idx) == s.n
    assert_lists(ivf, s.assign[:half], s.k, "before extend")
    sizes = ivf.list_sizes()
    for nprobe in (2, 12):
        P = ivf_ref.probes(s.Zq, nprobe, ~s.qbad)
        want = ivf_ref.restricted_top_m(s.S, s.qbad, s.xbad, s.assign, P, 256, covered=half)
        got = ivf.search(s.Q, nprobe, 256)
        assert_search(got, want, P, sizes, 70, 256, ("before extend", nprobe))
        assert all((got[0][q, :got[2][q]] < half).all() for q in range(70))
    with pytest.raises(bn.EngineError):
        ivf.search_ids([half], 1, 1)
    ivf.extend()
    assert ivf.rows == s.n
    ivf.extend()                                  # nothing new: nothing changes
    assert_lists(ivf, s.assign, s.k, "after extend")
    for nprobe, M in ((1, 100), (5, 256), (12, 64)):
        got, fresh = ivf.search(s.Q, nprobe, M), s.ivf.search(s.Q, nprobe, M)
        assert all(g.tobytes() == f.tobytes() for g, f in zip(got, fresh)), (nprobe, M)
    got, fresh = ivf.search_ids([half, s.n - 4], 3, 50, exclude_radius=0), s.ivf.search_ids([half, s.n - 4], 3, 50, exclude_radius=0)
    assert all(g.tobytes() == f.tobytes() for g, f in zip(got, fresh))


# ---- 6. invalid queries ----------------------------------------------------------------------------------------------------------
def test_invalid_query(bn):
    s = skew(130)
    Q = s.Q[:5].copy()
    Q[1] = 0.0
    Q[3, 7] = np.nan
    ids, sc, cnt, probes, scanned = s.ivf.search(Q, 3, 10)
    assert cnt[[1, 3]].tolist() == [0, 0] and (probes[[1, 3]] == NONE).all() and scanned[[1, 3]].tolist() == [0, 0]
    assert (probes[[0, 2, 4]] != NONE).all()
    good = s.ivf.search(s.Q[[0, 2, 4]], 3, 10)
    assert all(g[[0, 2, 4]].tobytes() == w.tobytes() for g, w in zip((ids, sc, cnt, probes, scanned), good))


# ---- 7. rows without a list; overflowing centroid scores ---------------------------------------------------------------------
def test_overflowing_centroid_scores_and_rows_without_a_list(bn):
    """Huge finite centroids against +-1 rows, the construction of the clustering tests, with k = 4 and with a single centroid.

    The contract gives a VALID row BN_CLUSTER_NONE when all its centroid scores are NaN, and never probes a NaN score.  Neither can be
    reached through the ABI: a stored component is at most 1 in magnitude and a centroid is finite, so every exact product is finite,
    and the chain's fused multiply-add of a finite product into +-inf stays +-inf: an overflow gives an infinity of one sign and no
    later step turns it into inf - inf.  Measured on an MI355X, bn_index_assign and bn_head_apply_host alike: the row with +1 at
    k = 0, 4, 8, 12 and -1 at k = 1, 5, 9, 13 (dim 14) against a centroid of 3.4e38 (and of FLT_MAX) in every component scores +inf,
    its negative -inf; 64 ones then 64 minus ones in one k chunk, and 128 / 128 across two chunks, score +inf; 24 000 random rows over
    {-1, 0, 1} at dims 4, 8, 14, 16, 33 and 130 against three +-FLT_MAX centroids give 35 560 infinite scores and no NaN; 500 such rows as
    queries of a view leave no probe slot empty.  So this test pins what does happen: the oracle has no NaN for a valid row (if that
    ever changes, the first assertion fails and the NaN rules become testable here); infinite scores order as numbers, +inf ties go
    to the lowest centroid, a row whose only score is -inf is in that list; and the rows that do get BN_CLUSTER_NONE, the invalid
    ones, are in no list and are never returned."""
    dim, n = 14, 200
    fmax = np.finfo(np.float32).max
    rng = np.random.default_rng(12)
    X = rng.choice(np.float32([-1.0, 1.0]), (n, dim)).astype(np.float32)
    X[0] = 0.0
    X[0, [0, 4, 8, 12]] = 1.0                     # one 16x16x4 instruction's four k of the first component of the float4 ...
    X[0, [1, 5, 9, 13]] = -1.0                    # ... and the next instruction's, with the opposite sign
    X[1] = -X[0]
    X[17] = 0.0
    X[130, 2] = np.nan
    cent = np.zeros((4, dim), dtype=np.float32)
    cent[0] = fmax
    cent[1] = fmax                                # a duplicate: +inf ties
    cent[2] = -fmax
    cent[3, 3] = 1.0                              # finite scores
    idx = bn.Index(0, dim, n)
    idx.add(X)
    stored = idx.read()
    valid = (stored != 0).any(axis=1)
    assert np.flatnonzero(~valid).tolist() == [17, 130]
    Z = twin_scores(bn, cent, stored)
    assert not np.isnan(Z[valid]).any(), "a valid row has a NaN centroid score: test the NaN rules of the contract with it"
    assert np.isposinf(Z[0, 0]) and np.isposinf(Z[0, 1]) and np.isneginf(Z[0, 2]) and np.isneginf(Z[1, 0]) and np.isposinf(Z[1, 2])
    assert np.isinf(Z[valid][:, :3]).sum() > 300
    assign, score = idx.assign(cent)
    wa, ws = cluster_ref.assign(Z, valid)
    assert np.array_equal(assign, wa) and score.tobytes() == ws.tobytes()
    assert np.flatnonzero(assign == NONE).tolist() == [17, 130] and assign[0] == 0 and assign[1] == 2

    every = np.arange(n, dtype=np.uint64)
    S = np.zeros((n, n), dtype=np.float32)
    ids, sc, cnt = idx.search_ids(every, 256)
    for q in range(n):
        S[q, ids[q, :cnt[q]].astype(np.int64)] = sc[q, :cnt[q]]
    ivf = bn.Ivf(idx, cent)
    assert_lists(ivf, assign, 4)
    sizes = ivf.list_sizes()
    for nprobe in (1, 2, 4):
        P = ivf_ref.probes(Z, nprobe, valid)
        want = ivf_ref.restricted_top_m(S, ~valid, ~valid, assign, P, 256)
        for M in (1, 256):
            got = ivf.search_ids(every, nprobe, M)
            assert_search(got, want, P, sizes, n, M, ("overflow", nprobe, M))
            assert all(not np.isin(got[0][q, :got[2][q]], [17, 130]).any() for q in range(n))
            host = ivf.search(X, nprobe, M)       # the same rows as host queries: normalised to the stored rows
            assert all(g.tobytes() == h.tobytes() for g, h in zip(got, host))
    assert P[0].tolist() == [0, 1, 3, 2] and P[1].tolist() == [2, 3, 0, 1] and (P[[17, 130]] == NONE).all() and (P[valid] != NONE).all()

    # the single-centroid case: every valid row is in the one list, the rows at -inf included
    for c in (0, 2):
        a1, s1 = idx.assign(cent[c:c + 1])
        assert np.isneginf(s1[valid]).any() and np.isposinf(s1[valid]).any() and np.flatnonzero(a1 == NONE).tolist() == [17, 130]
        one = bn.Ivf(idx, cent[c:c + 1])
        assert_lists(one, a1, 1)
        got = one.search_ids(every, 1, 256)
        want = idx.search_ids(every, 256)         # nothing valid is left out, so this is the exact search
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want))
        assert (got[3][valid, 0] == 0).all() and (got[4][valid] == n - 2).all() and not got[4][~valid].any()


# ---- 8. determinism and independence ---------------------------------------------------------------------------------------------
def test_determinism_and_independence(bn):
    s = skew(130)
    before = s.idx.read().tobytes(), [a.tobytes() for a in s.idx.search(s.Q[:9], 50)], len(s.idx)
    a = s.ivf.search(s.Q, 5, 100)
    b = s.ivf.search(s.Q, 5, 100)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), "the same call twice"
    for q in (0, 7, 33, 69):
        one = s.ivf.search(s.Q[q:q + 1], 5, 100)
        assert all(u[q:q + 1].tobytes() == v.tobytes() for u, v in zip(a, one)), ("one query at a time", q)
    ids_a = s.ivf.search_ids([3, 4000, 64], 2, 256, exclude_radius=1)
    other = np.random.default_rng(2).standard_normal((7, 130)).astype(np.float32)
    s.idx.cluster(4, max_iters=2)
    s.idx.assign(other)
    c = s.ivf.search(s.Q, 5, 100)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, c)), "a clustering and an assignment in between"
    assert all(u.tobytes() == v.tobytes() for u, v in zip(ids_a, s.ivf.search_ids([3, 4000, 64], 2, 256, exclude_radius=1)))
    assert_lists(s.ivf, s.assign, s.k)
    v2 = bn.Ivf(s.idx, s.cent)
    v2.extend()
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, v2.search(s.Q, 5, 100))), "a second view of the same index"
    after = s.idx.read().tobytes(), [x.tobytes() for x in s.idx.search(s.Q[:9], 50)], len(s.idx)
    assert before == after, "build, extend and search leave the index as it was"


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(bn):
    s = skew(130)
    lib, v, k = bn.lib, s.ivf._h, s.k
    cent = s.cent.copy()
    h = C.c_void_p(0x1234)

    def build(x, c, kk, out):
        return lib.bn_ivf_build(x, None if c is None else c.ctypes.data_as(f32p), kk, out)

    bad_nan, bad_inf = cent.copy(), cent.copy()
    bad_nan[3, 9] = np.nan
    bad_inf[11, 129] = -np.inf
    for args in ((None, cent, k), (s.idx._h, None, k), (s.idx._h, cent, 0), (s.idx._h, cent, 1025), (s.idx._h, bad_nan, k), (s.idx._h, bad_inf, k)):
        assert build(*args, C.byref(h)) == INVALID_ARG and bn.last_error(), args[2]
        assert h.value == 0x1234
    assert build(s.idx._h, cent, k, None) == INVALID_ARG
    assert lib.bn_ivf_extend(None) == INVALID_ARG

    sizes = np.full(k, 5, dtype=np.uint32)
    assert lib.bn_ivf_list_sizes(None, sizes.ctypes.data_as(u32p)) == INVALID_ARG and lib.bn_ivf_list_sizes(v, None) == INVALID_ARG
    assert (sizes == 5).all()
    ids = np.full(70, 0xABCDEF, dtype=np.uint64)
    n = C.c_size_t(55)
    assert lib.bn_ivf_read_list(v, k, ids.ctypes.data_as(u64p), 70, C.byref(n)) == INVALID_ARG and n.value == 55
    assert lib.bn_ivf_read_list(None, 0, ids.ctypes.data_as(u64p), 70, C.byref(n)) == INVALID_ARG and n.value == 55
    assert lib.bn_ivf_read_list(v, 1, ids.ctypes.data_as(u64p), 70, None) == INVALID_ARG
    assert lib.bn_ivf_read_list(v, 2, ids.ctypes.data_as(u64p), 64, C.byref(n)) == INVALID_ARG and n.value == 65, "cap too small: the size is reported"
    assert lib.bn_ivf_read_list(v, 1, None, 64, C.byref(n)) == INVALID_ARG
    assert (ids == 0xABCDEF).all()
    assert lib.bn_ivf_read_list(v, 4, None, 0, C.byref(n)) == 0 and n.value == 0, "an empty list needs no buffer"

    nq, stride, nprobe = 2, 4, 2
    q = np.ascontiguousarray(s.Q[:nq])
    qi = np.array([5, 6], dtype=np.uint64)

    def outs():
        return [np.full(nq * stride, 0xABCDEF, dtype=np.uint64), np.full(nq * stride, -7.5, dtype=np.float32), np.full(nq, 77, dtype=np.uint32),
                np.full(nq * nprobe, 0xDEADBEEF, dtype=np.uint32), np.full(nq, 99, dtype=np.uint64)]

    def ptrs(o, null=()):
        ps = [o[0].ctypes.data_as(u64p), o[1].ctypes.data_as(f32p), o[2].ctypes.data_as(u32p), o[3].ctypes.data_as(u32p), o[4].ctypes.data_as(u64p)]
        return [None if i in null else p for i, p in enumerate(ps)]

    cases = [dict(view=None), dict(q=None), dict(nprobe=0), dict(nprobe=k + 1), dict(top_m=0), dict(top_m=257, stride=300), dict(top_m=4, stride=3),
             dict(null=(0,)), dict(null=(1,)), dict(null=(2,))]
    for by_id in (False, True):
        for case in cases + ([dict(ids=[5, s.n]), dict(ids=[1 << 40, 0])] if by_id else []):
            o = outs()
            before = [a.tobytes() for a in o]
            view = case.get("view", v)
            np_, tm, st = case.get("nprobe", nprobe), case.get("top_m", stride), case.get("stride", stride)
            p = ptrs(o, case.get("null", ()))
            if by_id:
                ids_in = np.array(case.get("ids", qi), dtype=np.uint64)
                arg = None if "q" in case else ids_in.ctypes.data_as(u64p)
                status = lib.bn_ivf_search_ids(view, arg, nq, 0, np_, tm, st, *p)
            else:
                arg = None if "q" in case else q.ctypes.data_as(f32p)
                status = lib.bn_ivf_search(view, arg, nq, np_, tm, st, *p)
            assert status == INVALID_ARG and bn.last_error(), (by_id, case)
            assert [a.tobytes() for a in o] == before, (by_id, case)
    # probes_out and scanned_out may be NULL
    o = outs()
    assert lib.bn_ivf_search(v, q.ctypes.data_as(f32p), nq, nprobe, stride, stride, *ptrs(o, (3, 4))) == 0
    full = s.ivf.search(q, nprobe, stride)
    assert o[2].tobytes() == full[2].tobytes() and (o[3] == 0xDEADBEEF).all() and (o[4] == 99).all()
    for i in range(nq):                          # entries past a count stay as the caller left them
        c = int(full[2][i])
        assert np.array_equal(o[0][i * stride:i * stride + c], full[0][i, :c]) and (o[0][i * stride + c:(i + 1) * stride] == 0xABCDEF).all()
        assert o[1][i * stride:i * stride + c].tobytes() == full[1][i, :c].tobytes() and (o[1][i * stride + c:(i + 1) * stride] == -7.5).all()
    # m_stride above top_m: the rows keep their stride and the gap stays untouched
    wide = s.ivf.search(q, nprobe, 2, m_stride=4)
    assert np.array_equal(wide[2], np.minimum(full[2], 2)) and np.array_equal(wide[0][:, :2], full[0][:, :2]) and (wide[0][:, 2:] == 0).all() and np.isnan(wide[1][:, 2:]).all()


# ---- empty index ------------------------------------------------------------------------------------------------------------------
def test_empty_index(bn):
    idx = bn.Index(0, 130, 300)
    cent = ivf_ref.skewed_case(130)[1]
    ivf = bn.Ivf(idx, cent)
    assert len(ivf) == 12 and ivf.rows == 0 and not ivf.list_sizes().any() and all(len(ivf.read_list(c)) == 0 for c in range(12))
    ids, sc, cnt, probes, scanned = ivf.search(cent[:3] + 0.01, 2, 5)
    assert not cnt.any() and not scanned.any() and probes[:, 0].tolist() == [0, 1, 2], "empty lists still use their slots"
    ivf.extend()
    assert ivf.rows == 0


# ---- 5b / 10. a network-filled index: extend after bn_index_add_ctx, and the loop end to end -------------------------------------
def test_network_filled_index_extend_and_loop(bn):
    m = bn.Model(write_model(synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)))
    cfg = m.config
    n_samp, sr, B = int(cfg.sample_count), int(cfg.sample_rate), 4
    rng = np.random.default_rng(8)
    pcm = synth.synthetic_segments(1, n_samp * 3 * B, sr)[0]
    pcm = np.clip(pcm + 0.05 * rng.standard_normal(len(pcm)), -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    ctx = bn.Context(m, B)
    n, k = 3 * B, 3
    idx = bn.Index(0, int(cfg.embedding_dim), n)
    ctx.infer_windows(rec, n_samp, 0, B)
    assert idx.add_context(ctx, B) == 0
    cent0 = idx.read()[[0, 2]] * np.float32(1.25)
    early = bn.Ivf(idx, cent0)                   # built on the first append
    for f in range(B, n, B):
        ctx.infer_windows(rec, n_samp, f, B)
        assert idx.add_context(ctx, B) == f
    got = early.search_ids(np.arange(B), 2, n)   # waits for the pending append itself; still covers B rows
    assert early.rows == B and all((got[0][q, :got[2][q]] < B).all() for q in range(B)) and (got[2] == B).all()
    early.extend()
    fresh = bn.Ivf(idx, cent0)
    assert early.rows == n and np.array_equal(early.list_sizes(), fresh.list_sizes())
    every = np.arange(n, dtype=np.uint64)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(early.search_ids(every, 1, n), fresh.search_ids(every, 1, n)))
    assert all(np.array_equal(early.read_list(c), fresh.read_list(c)) for c in range(2))

    # the loop: cluster -> view -> search by example, against the reference cut from the index's own assignment and search
    cent, assign, score, counts, rep = idx.cluster(k, max_iters=5)
    ivf = bn.Ivf(idx, cent)
    assert_lists(ivf, assign, k)
    assert np.array_equal(ivf.list_sizes(), counts)
    S = np.zeros((n, n), dtype=np.float32)
    ids, sc, cnt = idx.search_ids(every, n)
    assert (cnt == n).all()
    for q in range(n):
        S[q, ids[q].astype(np.int64)] = sc[q]
    Zq = twin_scores(bn, cent, idx.read())
    none = np.zeros(n, dtype=bool)
    for nprobe in (1, 2, 3):
        P = ivf_ref.probes(Zq, nprobe, np.ones(n, dtype=bool))
        for radius in (-1, 0):
            ex = None if radius < 0 else exact.radius_mask(every, radius, n)
            want = ivf_ref.restricted_top_m(S, none, none, assign, P, 256, ex)
            assert_search(ivf.search_ids(every, nprobe, n, exclude_radius=radius), want, P, counts, n, n, ("loop", nprobe, radius))
    assert np.array_equal(ivf.search_ids(every, 1, 1)[3][:, 0], assign)
