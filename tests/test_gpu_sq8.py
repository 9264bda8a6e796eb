"""bn_sq8_* on the GPU.  Codes, scales, keys and candidates come from tests/sq8_ref.py applied to Index.read(); exact scores come from
the score matrix bn_index_search itself gives (test_gpu_ivf.search_matrix) or, for dyadic rows, from index_ref.scores64.  Codes,
scales, candidates, counts, ids and score bytes are compared with ==."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import index_ref as ir
import sq8_ref
import test_gpu_index_exact as exact
from gpu_helpers import write_model
from test_gpu_ivf import as_stored, search_matrix

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
INVALID_ARG = 1
f32p, u32p, u64p, i8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int8)
GRID = ((1, 1), (64, 64), (100, 37), (256, 100), (256, 256))  # (refine, top_m)


def _bn():
    return importlib.import_module("rust-birdnet-onnx_amd")


def assert_search(got, want, nq, what):
    """got = (ids, scores, counts, cands, cand_counts) of a search of the first nq queries; want the same from sq8_ref.expected"""
    wi, ws, wc, wcand, wcc = want
    assert got[4].dtype == np.uint32 and np.array_equal(got[4], wcc[:nq]), (what, "cand counts", got[4][:8], wcc[:8])
    assert got[3].dtype == np.uint64 and got[3].shape == wcand[:nq].shape, (what, "cands")
    if not np.array_equal(got[3], wcand[:nq]):
        q, j = np.argwhere(got[3] != wcand[:nq])[0]
        raise AssertionError((what, "cands: query %d rank %d" % (q, j), got[3][q, max(0, j - 2):j + 3], wcand[q, max(0, j - 2):j + 3]))
    exact.assert_exact(got[:3], (wi[:nq], ws[:nq], wc[:nq]), what)


# ---- 1. codes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 3, 130, 1536])
def test_codes(bn, dim):
    rng = np.random.default_rng(dim)
    for n in (1, 63, 64, 65, 700):
        X = rng.standard_normal((n, dim)).astype(np.float32)
        if n > 1:
            X[n // 2] = 0.0
            X[n - 1, dim // 2] = np.inf                    # stored as zeros
            X[1] = -np.abs(X[1])                           # the maximum is negative
        if n > 10:
            X[5, 0] = np.nan
            X[7] = np.ldexp(np.float32(1.0), -3)           # every element the maximum
        idx = bn.Index(0, dim, n + 9)
        idx.add(X)
        stored = idx.read()
        v = bn.Sq8(idx)
        assert v.rows == n
        wc, ws = sq8_ref.codes(stored)
        gc, gs = v.read()
        assert gc.dtype == np.int8 and gs.dtype == np.float32 and gc.shape == (n, dim)
        assert gc.tobytes() == wc.tobytes() and gs.tobytes() == ws.tobytes(), (dim, n)
        if n > 1:
            assert not gc[n // 2].any() and not gc[n - 1].any() and gs[n // 2].tobytes() == np.float32(0).tobytes()
        for first, count in ((0, 1), (n - 1, 1), (n // 3, n - n // 3), (n, 0)):
            gc, gs = v.read(first, count)
            assert gc.tobytes() == wc[first:first + count].tobytes() and gs.tobytes() == ws[first:first + count].tobytes(), (dim, n, first)


# ---- 2. general rows -----------------------------------------------------------------------------------------------------------
class General:
    def __init__(self, dim):
        bn = _bn()
        rng = np.random.default_rng(9000 + dim)
        self.n = 6000 + 37
        self.X = rng.standard_normal((self.n, dim)).astype(np.float32)
        self.X[100] = 0.0
        self.X[4097, dim // 3] = np.nan
        self.Q = (self.X[rng.integers(0, self.n, 70)] + 0.5 * rng.standard_normal((70, dim))).astype(np.float32)
        self.Q[5:9] = self.X[[0, 63, 64, self.n - 1]]
        self.idx = bn.Index(0, dim, self.n)
        self.idx.add(self.X)
        self.stored = self.idx.read()
        self.view = bn.Sq8(self.idx)
        self.Qn, self.qbad = as_stored(bn, self.Q)
        self.S = search_matrix(bn, self.X, self.Q)


@functools.lru_cache(maxsize=None)
def general(dim):
    return General(dim)


@pytest.mark.parametrize("dim", [130, 1536])
def test_general_rows(bn, dim):
    g = general(dim)
    assert g.view.rows == g.n and g.n % 64 and not g.qbad.any()
    ex = sq8_ref.Expected(g.stored, g.Qn, g.S)
    for refine, M in GRID:
        want = ex.at(refine, M)
        for nq in (1, 17, 70):
            assert_search(g.view.search(g.Q[:nq], refine, M), want, nq, (dim, "refine", refine, "M", M, "Q", nq))
    assert not np.isin([100, 4097], want[3]).any(), "invalid rows are never candidates"


# ---- 3. dyadic rows, heavy ties, many tiles per workgroup ------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["constant", "sawtooth", "random"])
def test_dyadic_rows_heavy_ties(bn, order):
    case = exact.ordered_case(bn, order, 128, 64)
    v = bn.Sq8(case.idx)
    stored = case.idx.read()
    Qn, qbad = as_stored(bn, case.Q)
    assert np.array_equal(qbad, case.qbad)
    # a dyadic row's codes are +-127 on its support, so a key is an integer multiple of one constant: the keys tie as the scores do
    rc, rs = sq8_ref.codes(stored)
    assert set(np.unique(rc).tolist()) <= {-127, 0, 127}
    ex = sq8_ref.Expected(stored, Qn, case.S)
    for refine, M in GRID:
        want = ex.at(refine, M)
        for nq in ((70, 1) if refine == 256 else (17,)):
            assert_search(v.search(case.Q[:nq], refine, M), want, nq, (order, "refine", refine, "M", M, "Q", nq))


# ---- 4. all candidates fit ---------------------------------------------------------------------------------------------------------
def test_all_candidates_fit_equals_the_exact_search(bn):
    rng = np.random.default_rng(4)
    n, dim = 256 + 5, 130
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X[[3, 70, 128, 200, 260]] = 0.0               # 256 valid rows
    Q = rng.standard_normal((20, dim)).astype(np.float32)
    idx = bn.Index(0, dim, n)
    idx.add(X)
    v = bn.Sq8(idx)
    for M in (1, 100, 256):
        got, want = v.search(Q, 256, M), idx.search(Q, M)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want)), M
        assert (got[4] == 256).all()
        qids = [0, 1, 63, 64, 65, 199, 259, 3]
        for radius in (-1, 0, 3):
            got, want = v.search_ids(qids, 256, M, exclude_radius=radius), idx.search_ids(qids, M, exclude_radius=radius)
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got[:3], want)), (M, radius)
            assert got[4][-1] == 0 and got[2][-1] == 0, "the id of an invalid row: nothing"


# ---- 5. the approximation is visible -------------------------------------------------------------------------------------------------
def test_the_approximation_is_visible(bn):
    X, Q = sq8_ref.tight_case()
    idx = bn.Index(0, 6, len(X))
    idx.add(X)
    stored = idx.read()
    v = bn.Sq8(idx)
    Qn, qbad = as_stored(bn, Q)
    S = search_matrix(bn, X, Q)
    true = idx.search(Q, 32)
    assert (true[2] == 32).all()
    differs = 0
    for R in (32, 64, 256):
        want = sq8_ref.expected(stored, Qn, S, R, 32)
        for q in range(len(Q)):
            assert not np.isin(true[0][q], want[3][q]).all(), ("the true top-32 is inside the coarse top-R", R, q)
        got = v.search(Q, R, 32)
        assert_search(got, want, len(Q), ("tight", R))
        differs += int(sum(got[0][q].tobytes() != true[0][q].tobytes() for q in range(len(Q))))
    assert differs > 0, "the case shows nothing: the coarse search equals the exact one"


# ---- 6. extend -------------------------------------------------------------------------------------------------------------------
def test_extend_covers_appended_rows(bn):
    g = general(130)
    n0 = 2987                                     # inside a tile
    idx = bn.Index(0, 130, g.n)
    idx.add(g.X[:n0])
    v = bn.Sq8(idx)
    idx.add(g.X[n0:4000])
    idx.add(g.X[4000:])
    assert v.rows == n0 and len(idx) == g.n
    wc, ws = sq8_ref.codes(g.stored)
    gc, gs = v.read()
    assert gc.tobytes() == wc[:n0].tobytes() and gs.tobytes() == ws[:n0].tobytes()
    with pytest.raises(bn.EngineError):
        v.read(n0, 1)
    for refine, M in ((256, 100), (64, 64)):
        want = sq8_ref.expected(g.stored, g.Qn, g.S, refine, M, n_covered=n0)
        got = v.search(g.Q, refine, M)
        assert_search(got, want, 70, ("before extend", refine))
        assert all((got[3][q, :got[4][q]] < n0).all() for q in range(70))
    with pytest.raises(bn.EngineError):
        v.search_ids([n0], 4, 1)
    assert v.search_ids([n0 - 1], 4, 1)[2][0] == 1
    v.extend()
    assert v.rows == g.n
    v.extend()                                    # nothing new: nothing changes
    gc, gs = v.read()
    fc, fs = g.view.read()
    assert gc.tobytes() == fc.tobytes() == wc.tobytes() and gs.tobytes() == fs.tobytes() == ws.tobytes()
    for refine, M in ((1, 1), (256, 100), (100, 37)):
        got, fresh = v.search(g.Q, refine, M), g.view.search(g.Q, refine, M)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, fresh)), (refine, M)
    got, fresh = v.search_ids([n0, g.n - 1], 200, 50, exclude_radius=0), g.view.search_ids([n0, g.n - 1], 200, 50, exclude_radius=0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, fresh))


# ---- 7. search_ids ---------------------------------------------------------------------------------------------------------------
def test_search_ids_and_exclusion(bn):
    g = general(130)
    rng = np.random.default_rng(6)
    qids = np.concatenate([[0, 1, 63, 64, 100, 4097, g.n - 2, g.n - 1], rng.integers(0, g.n, 12)]).astype(np.uint64)
    qi = qids.astype(np.int64)
    S = search_matrix(bn, g.X, g.X[qi])
    for radius in (-1, 0, 3):
        ex = None if radius < 0 else exact.radius_mask(qids, radius, g.n)
        e = sq8_ref.Expected(g.stored, g.stored[qi], S, excluded=ex)
        for refine, M in ((256, 100), (64, 64), (1, 1)):
            want = e.at(refine, M)
            got = g.view.search_ids(qids, refine, M, exclude_radius=radius)
            assert_search(got, want, len(qids), ("ids", "radius", radius, "refine", refine, "M", M))
            for q in range(len(qids)):
                if radius >= 0:
                    near = np.arange(max(0, qi[q] - radius), min(g.n, qi[q] + radius + 1))
                    assert not np.isin(near, got[3][q, :got[4][q]]).any() and not np.isin(near, got[0][q, :got[2][q]]).any(), (radius, q)
            assert got[4][4] == 0 and got[4][5] == 0, "the id of an invalid row: no candidates"


# ---- 8. invalid queries ------------------------------------------------------------------------------------------------------------
def test_invalid_query(bn):
    g = general(130)
    Q = g.Q[:5].copy()
    Q[1] = 0.0
    Q[3, 7] = np.nan
    ids, sc, cnt, cands, cc = g.view.search(Q, 50, 10)
    assert cnt[[1, 3]].tolist() == [0, 0] and cc[[1, 3]].tolist() == [0, 0]
    assert cnt[[0, 2, 4]].tolist() == [10, 10, 10] and cc[[0, 2, 4]].tolist() == [50, 50, 50]
    good = g.view.search(g.Q[[0, 2, 4]], 50, 10)
    assert all(a[[0, 2, 4]].tobytes() == b.tobytes() for a, b in zip((ids, sc, cnt, cands, cc), good))


# ---- 9. determinism ----------------------------------------------------------------------------------------------------------------
def test_determinism(bn):
    g = general(130)
    before = g.idx.read().tobytes(), [a.tobytes() for a in g.idx.search(g.Q[:9], 50)], len(g.idx)
    a = g.view.search(g.Q, 256, 100)
    b = g.view.search(g.Q, 256, 100)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b)), "the same call twice"
    for q in range(70):
        one = g.view.search(g.Q[q:q + 1], 256, 100)
        assert all(u[q:q + 1].tobytes() == v.tobytes() for u, v in zip(a, one)), ("one query at a time", q)
    wide = g.view.search(g.Q, 256, 100, m_stride=131)
    assert np.array_equal(wide[0][:, :100], a[0]) and wide[1][:, :100].tobytes() == a[1].tobytes() and np.array_equal(wide[2], a[2])
    assert not wide[0][:, 100:].any() and np.isnan(wide[1][:, 100:]).all(), "the gap keeps the binding's sentinels"
    assert all(u.tobytes() == v.tobytes() for u, v in zip(wide[3:], a[3:]))
    v2 = bn.Sq8(g.idx)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, v2.search(g.Q, 256, 100))), "a second view of the same index"
    after = g.idx.read().tobytes(), [x.tobytes() for x in g.idx.search(g.Q[:9], 50)], len(g.idx)
    assert before == after, "build and search leave the index as it was"


# ---- 10. refusals and the empty index ------------------------------------------------------------------------------------------------
def test_refusals(bn):
    g = general(130)
    lib, v = bn.lib, g.view._h
    h = C.c_void_p(0x1234)
    assert lib.bn_sq8_build(None, C.byref(h)) == INVALID_ARG and bn.last_error() and h.value == 0x1234
    assert lib.bn_sq8_build(g.idx._h, None) == INVALID_ARG
    wide = bn.Index(0, 131073, 1)
    assert lib.bn_sq8_build(wide._h, C.byref(h)) == INVALID_ARG and "131072" in bn.last_error() and h.value == 0x1234
    del wide
    assert lib.bn_sq8_extend(None) == INVALID_ARG
    codes = np.full(4 * 130, 55, dtype=np.int8)
    scales = np.full(4, -7.5, dtype=np.float32)
    for view, first, count in ((None, 0, 1), (v, g.n, 1), (v, g.n - 3, 4), (v, g.n + 1, 0), (v, 1 << 63, 1 << 63)):
        assert lib.bn_sq8_read(view, first, count, codes.ctypes.data_as(i8p), scales.ctypes.data_as(f32p)) == INVALID_ARG and bn.last_error()
    assert (codes == 55).all() and (scales == -7.5).all()
    assert lib.bn_sq8_read(v, 5, 2, None, scales.ctypes.data_as(f32p)) == 0 and scales[:2].tobytes() == sq8_ref.codes(g.stored[5:7])[1].tobytes()
    assert lib.bn_sq8_read(v, 5, 2, codes.ctypes.data_as(i8p), None) == 0 and codes[:260].tobytes() == sq8_ref.codes(g.stored[5:7])[0].tobytes()
    assert (codes[260:] == 55).all() and (scales[2:] == -7.5).all()

    nq, stride, refine = 2, 4, 6
    q = np.ascontiguousarray(g.Q[:nq])
    qi = np.array([5, 6], dtype=np.uint64)

    def outs():
        return [np.full(nq * stride, 0xABCDEF, dtype=np.uint64), np.full(nq * stride, -7.5, dtype=np.float32), np.full(nq, 77, dtype=np.uint32),
                np.full(nq * refine, 0xFEDCBA, dtype=np.uint64), np.full(nq, 99, dtype=np.uint32)]

    def ptrs(o, null=()):
        ps = [o[0].ctypes.data_as(u64p), o[1].ctypes.data_as(f32p), o[2].ctypes.data_as(u32p), o[3].ctypes.data_as(u64p), o[4].ctypes.data_as(u32p)]
        return [None if i in null else p for i, p in enumerate(ps)]

    cases = [dict(view=None), dict(q=None), dict(refine=0), dict(refine=257), dict(top_m=0), dict(top_m=refine + 1, stride=refine + 1), dict(top_m=4, stride=3),
             dict(null=(0,)), dict(null=(1,)), dict(null=(2,))]
    for by_id in (False, True):
        for case in cases + ([dict(ids=[5, g.n]), dict(ids=[1 << 40, 0])] if by_id else []):
            o = outs()
            before = [a.tobytes() for a in o]
            view = case.get("view", v)
            rf, tm, st = case.get("refine", refine), case.get("top_m", stride), case.get("stride", stride)
            p = ptrs(o, case.get("null", ()))
            if by_id:
                ids_in = np.array(case.get("ids", qi), dtype=np.uint64)
                arg = None if "q" in case else ids_in.ctypes.data_as(u64p)
                status = lib.bn_sq8_search_ids(view, arg, nq, 0, rf, tm, st, *p)
            else:
                arg = None if "q" in case else q.ctypes.data_as(f32p)
                status = lib.bn_sq8_search(view, arg, nq, rf, tm, st, *p)
            assert status == INVALID_ARG and bn.last_error(), (by_id, case)
            assert [a.tobytes() for a in o] == before, (by_id, case)
    # cand_out and cand_count_out may be NULL
    o = outs()
    assert lib.bn_sq8_search(v, q.ctypes.data_as(f32p), nq, refine, stride, stride, *ptrs(o, (3, 4))) == 0
    full = g.view.search(q, refine, stride)
    assert o[2].tobytes() == full[2].tobytes() and (o[3] == 0xFEDCBA).all() and (o[4] == 99).all()
    assert o[0].tobytes() == full[0].tobytes() and o[1].tobytes() == full[1].tobytes()


def test_empty_index(bn):
    idx = bn.Index(0, 130, 300)
    v = bn.Sq8(idx)
    assert v.rows == 0
    gc, gs = v.read()
    assert gc.shape == (0, 130) and gs.shape == (0,)
    ids, sc, cnt, cands, cc = v.search(np.ones((3, 130), dtype=np.float32), 5, 2)
    assert not cnt.any() and not cc.any()
    v.extend()
    assert v.rows == 0
    idx.add(np.ones((2, 130), dtype=np.float32))
    v.extend()
    ids, sc, cnt, cands, cc = v.search(np.ones((3, 130), dtype=np.float32), 5, 2)
    assert v.rows == 2 and (cnt == 2).all() and (cc == 2).all() and cands[:, :2].tolist() == [[0, 1]] * 3


# ---- 11. a network-filled index ------------------------------------------------------------------------------------------------------
def test_network_filled_index(bn):
    m = bn.Model(write_model(synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)))
    cfg = m.config
    n_samp, sr, B = int(cfg.sample_count), int(cfg.sample_rate), 4
    rng = np.random.default_rng(8)
    pcm = synth.synthetic_segments(1, n_samp * 3 * B, sr)[0]
    pcm = np.clip(pcm + 0.05 * rng.standard_normal(len(pcm)), -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    ctx = bn.Context(m, B)
    n = 3 * B
    idx = bn.Index(0, int(cfg.embedding_dim), n)
    ctx.infer_windows(rec, n_samp, 0, B)
    assert idx.add_context(ctx, B) == 0
    early = bn.Sq8(idx)                           # directly after the append, without a synchronise in between
    assert early.rows == B
    for f in range(B, n, B):
        ctx.infer_windows(rec, n_samp, f, B)
        assert idx.add_context(ctx, B) == f
    late = bn.Sq8(idx)                            # likewise
    stored = idx.read()
    wc, ws = sq8_ref.codes(stored)
    gc, gs = early.read()
    assert gc.tobytes() == wc[:B].tobytes() and gs.tobytes() == ws[:B].tobytes()
    gc, gs = late.read()
    assert late.rows == n and gc.tobytes() == wc.tobytes() and gs.tobytes() == ws.tobytes()
    early.extend()
    every = np.arange(n, dtype=np.uint64)
    S = np.zeros((n, n), dtype=np.float32)
    ids, sc, cnt = idx.search_ids(every, n)
    assert (cnt == n).all()
    for q in range(n):
        S[q, ids[q].astype(np.int64)] = sc[q]
    for refine, M in ((n, n), (5, 3)):
        for radius in (-1, 0):
            ex = None if radius < 0 else exact.radius_mask(every, radius, n)
            want = sq8_ref.expected(stored, stored, S, refine, M, excluded=ex)
            for view in (early, late):
                assert_search(view.search_ids(every, refine, M, exclude_radius=radius), want, n, ("network", refine, M, radius))
