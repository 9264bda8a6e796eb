"""bn_index_search_peaks / bn_index_search_peaks_ids on the GPU.  Expected results come from tests/peaks_ref.peaks_top_m over the score
matrix bn_index_search itself gives (test_gpu_ivf.search_matrix) or, for dyadic rows, over index_ref.scores64, which is exact for them.
Counts, ids and score bytes are compared with ==."""
import ctypes as C
import functools

import numpy as np
import pytest

import index_ref as ir
import peaks_ref
import test_gpu_index_exact as exact
from test_gpu_ivf import search_matrix
from test_gpu_subset import cut, general

pytestmark = pytest.mark.gpu
INVALID_ARG = 1
TILE = exact.TILE
N = exact.N
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def assert_spacing(got, radius, what):
    """two returned ids of one query differ by more than the radius"""
    ids, _, cnt = got
    for q in range(len(cnt)):
        d = np.diff(np.sort(ids[q, :cnt[q]].astype(np.int64)))
        assert (d > radius).all(), (what, "query", q, "ids", radius, "or fewer apart")


# ---- 1. general data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [130, 1536])
def test_general_data(bn, dim):
    g = general(dim)
    Q, qbad = g.Q.copy(), g.qbad.copy()
    Q[10] = 0.0                                              # one invalid query: count 0 (its row of g.S is then never looked at)
    qbad[10] = True
    assert qbad.sum() == 1 and np.array_equal(np.flatnonzero(g.xbad), g.bad)
    el = peaks_ref.eligibility(g.n, qbad, g.xbad)
    full, short = False, False
    for radius in (0, 1, 2, 63, 64):
        want = peaks_ref.peaks_top_m(g.S, el, radius, 256)
        assert want[2][10] == 0
        if radius == 1:
            full = bool((want[2][~qbad] == 256).all())
        if radius == 64:
            short = bool(((want[2][~qbad] < 100) & (want[2][~qbad] > 1)).all())
        for nq in (1, 17, 70):
            for M in (1, 64, 100, 256):
                got = g.idx.search_peaks(Q[:nq], M, radius)
                exact.assert_exact(got, cut(want, nq, M), (dim, "radius", radius, "Q", nq, "M", M))
        assert_spacing(g.idx.search_peaks(Q, 256, radius), radius, (dim, radius))
        assert not np.isin(g.bad, want[0][want[2] > 0]).any()
    assert full and short, "both branches must occur: count == M at radius 1 and count < M at radius 64"


# ---- 2. exact data at many tiles per workgroup ------------------------------------------------------------------------------------
NQ_EXACT = 17     # two query blocks, the second ragged
RADII_EXACT = (1, 37, 64)


@functools.lru_cache(maxsize=1)
def ordered_case(order):
    bn = __import__("importlib").import_module("rust-birdnet-onnx_amd")
    rng = np.random.default_rng([128, 64, exact.ORDERS.index(order)])
    lv = exact.levels(order, N, 64, rng)
    case = exact.Case(bn, ir.rows_at_levels(rng, lv, 128, 64), exact.queries(rng, 128, 64, NQ_EXACT))
    case.levels = lv
    return case


def check_case(case, what, radii=RADII_EXACT, ms=(1, 100, 256), qs=(1, NQ_EXACT)):
    n = len(case.X)
    el = peaks_ref.eligibility(n, case.qbad, case.xbad)
    for radius in radii:
        want = peaks_ref.peaks_top_m(case.S, el, radius, 256)
        for nq in qs:
            for M in ms:
                got = case.idx.search_peaks(case.Q[:nq], M, radius)
                exact.assert_exact(got, cut(want, nq, M), (what, "radius", radius, "Q", nq, "M", M))
    return want


@pytest.mark.parametrize("order", exact.ORDERS)
def test_row_orders_many_tiles_per_workgroup(bn, order):
    """the carried ring, the delayed judgment, the halo at workgroup edges and the ragged last tile, on rows that nearly all tie"""
    exact.require_many_tiles()
    case = ordered_case(order)
    check_case(case, order)
    ids, _, cnt = case.idx.search_peaks(case.Q[:1], 256, 64)
    if order == "constant":
        assert cnt[0] == 1 and ids[0, 0] == 0, "a run of exact ties has one peak, its lowest id"
    if order == "rising":
        top = int(np.flatnonzero(case.levels == case.levels.max())[0])
        assert ids[0, 0] == top and cnt[0] == 129, "rising plateaus: the first row of each of the 129 is a peak, the top one first"
    if order == "falling":
        assert ids[0, 0] == 0 and cnt[0] == 1


def test_equal_best_rows_across_workgroup_and_tile_edges(bn):
    """the two best rows of query 0 sit on either side of an edge with equal scores: exactly the lower id survives"""
    cus = exact.require_many_tiles()
    tpw, n_wg = exact.tiles_per_workgroup(N, cus)
    wg = tpw * TILE
    assert tpw > 3 and n_wg > 3 and (n_wg - 1) * wg < N - 38 - TILE
    rng = np.random.default_rng(59)
    lv = rng.integers(-64, 56, N)                           # everything else lies below the planted level
    pairs = [(3 * TILE - 1, 3 * TILE)] + [(k * wg - 1, k * wg) for k in (1, 2, n_wg - 1)] + [(N - 38, N - 37)]
    for a, b in pairs:
        lv[[a, b]] = 64
    lv[N - 1] = 64                                          # alone at the end: rows past the end do not exist
    case = exact.Case(bn, ir.rows_at_levels(rng, lv, 128, 64), exact.queries(rng, 128, 64, NQ_EXACT))
    check_case(case, "edges")
    ids, sc, cnt = case.idx.search_peaks(case.Q[:1], 256, 1)
    lower = [a for a, _ in pairs] + [N - 1]
    assert ids[0, :len(lower)].tolist() == lower and (sc[0, :len(lower)] == 1.0).all() and sc[0, len(lower)] < 1.0
    assert not np.isin([b for _, b in pairs], ids[0, :cnt[0]]).any(), "the higher id of a tied pair was returned"
    ids, sc, cnt = case.idx.search_peaks(case.Q[:1], 256, 37)
    assert ids[0, :len(pairs)].tolist() == [a for a, _ in pairs] and sc[0, len(pairs)] < 1.0, "row N - 1 lies 37 rows after N - 38, which ties and wins"


# ---- 3. invalid rows and edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 64, 65, 129, 300])
def test_invalid_rows_inside_a_tied_run_and_small_sizes(bn, n):
    rng = np.random.default_rng(61 + n)
    Q = exact.queries(rng, 128, 64, 5)
    # every row the canonical query itself: query 0 ties on all of them; the other queries see random levels of their own
    X = np.repeat(Q[:1], n, axis=0)
    bad = [i for i in (10, 11, 12, 62, 63, 64, 65, 127, 128, 130, 131, 132, 133, 134, 200) + tuple(range(230, 300)) if i < n and n > 1]
    X[bad] = 0.0
    case = exact.Case(bn, X, Q, capacity=n + 70)
    assert np.array_equal(np.flatnonzero(case.xbad), bad)
    want = check_case(case, ("tied run", n), radii=(1, 2, 3, 5, 64), ms=(1, 256), qs=(1, 5))
    el = peaks_ref.eligibility(n, case.qbad, case.xbad)
    if n == 300:
        for radius, peaks in ((1, [0, 13, 66, 129, 135, 201]), (2, [0, 13, 66, 129, 135]), (3, [0, 13, 66, 135]), (64, [0])):
            ids, _, cnt = case.idx.search_peaks(Q[:1], 256, radius)
            assert ids[0, :cnt[0]].tolist() == peaks, (radius, "the row after a gap is a peak exactly when no eligible row lies within the radius before it")
            assert np.flatnonzero(peaks_ref.peak_mask(case.S[:1], el[:1], radius)[0]).tolist() == peaks
    if n == 1:
        assert want[2].tolist() == [1] * 5 and not want[0].any()
    # random levels at the same sizes: ordinary peaks next to the slab's end
    lv = rng.integers(-64, 65, n)
    case = exact.Case(bn, ir.rows_at_levels(rng, lv, 128, 64), Q)
    check_case(case, ("random levels", n), radii=(1, 2, 63, 64), ms=(1, 256), qs=(1, 5))


# ---- 4. search_peaks_ids --------------------------------------------------------------------------------------------------------------
def test_search_peaks_ids_general_data(bn):
    g = general(130)
    rng = np.random.default_rng(67)
    qi = np.concatenate([[0, 1, 63, 64, 65, g.n - 1], g.bad, rng.integers(0, g.n, 70)])[:70].astype(np.int64)
    S = search_matrix(bn, g.X, g.X[qi])
    qbad = g.xbad[qi]
    assert qbad.sum() >= 3
    for ex in (-1, 0, 3):
        el = peaks_ref.eligibility(g.n, qbad, g.xbad, qi, ex)
        want = peaks_ref.peaks_top_m(S, el, 2, 256)
        for nq in (1, 17, 70):
            for M in (1, 100, 256):
                got = g.idx.search_peaks_ids(qi[:nq], M, 2, exclude_radius=ex)
                exact.assert_exact(got, cut(want, nq, M), ("exclude", ex, "Q", nq, "M", M))
        got = g.idx.search_peaks_ids(qi, 256, 2, exclude_radius=ex)
        assert_spacing(got, 2, ("ids", ex))
        assert not got[2][qbad].any(), "the id of an invalid row gives count 0"
        for q in np.flatnonzero(~qbad):
            r = got[0][q, :got[2][q]].astype(np.int64)
            assert got[2][q] == 256 and (ex < 0 or not (np.abs(r - qi[q]) <= ex).any()), (ex, q)
            if ex < 0:
                assert r[0] == qi[q], "the query's own row is its best peak"
        # peak_radius 0 is search_ids
        for a, b in zip(g.idx.search_peaks_ids(qi, 100, 0, exclude_radius=ex), g.idx.search_ids(qi, 100, exclude_radius=ex)):
            assert a.tobytes() == b.tobytes(), ex


def test_excluded_rows_do_not_suppress_their_neighbours_and_bad_ids_are_refused(bn):
    rng = np.random.default_rng(71)
    n = 200
    row = ir.canonical_query(128, 64)
    idx = bn.Index(0, 128, n)
    idx.add(np.repeat(row[None], n, axis=0))                # every pair scores 1.0
    ids, sc, cnt = idx.search_peaks_ids([100, 0, 199, 64], 256, 2, exclude_radius=3)
    assert [ids[q, :cnt[q]].tolist() for q in range(4)] == [[0, 104], [4], [0], [0, 68]] and (sc[cnt[:, None] > np.arange(256)[None]] == 1.0).all()
    ids, sc, cnt = idx.search_peaks_ids([100, 0], 256, 1, exclude_radius=0)
    assert [ids[q, :cnt[q]].tolist() for q in range(2)] == [[0, 101], [1]]
    ids, sc, cnt = idx.search_peaks_ids([100], 256, 8, exclude_radius=3)
    assert ids[0, :cnt[0]].tolist() == [0], "row 96 is within 8 of row 104"
    # a query id >= size: refused, nothing written
    oi, os_, oc = np.full(8, 0xABCDEF, dtype=np.uint64), np.full(8, -7.5, dtype=np.float32), np.full(2, 77, dtype=np.uint32)
    before = (oi.tobytes(), os_.tobytes(), oc.tobytes())
    for radius in (0, 2):
        qi = np.array([5, n], dtype=np.uint64)
        st = bn.lib.bn_index_search_peaks_ids(idx._h, qi.ctypes.data_as(u64p), 2, -1, radius, 4, 4, oi.ctypes.data_as(u64p), os_.ctypes.data_as(f32p),
                                              oc.ctypes.data_as(u32p))
        assert st == INVALID_ARG and str(n) in bn.last_error() and (oi.tobytes(), os_.tobytes(), oc.tobytes()) == before
    q = np.ones(128, dtype=np.float32)
    st = bn.lib.bn_index_search_peaks(idx._h, q.ctypes.data_as(f32p), 1, 65, 4, 4, oi.ctypes.data_as(u64p), os_.ctypes.data_as(f32p), oc.ctypes.data_as(u32p))
    assert st == INVALID_ARG and "peak_radius" in bn.last_error() and (oi.tobytes(), os_.tobytes(), oc.tobytes()) == before
    st = bn.lib.bn_index_search_peaks(None, q.ctypes.data_as(f32p), 1, 2, 4, 4, oi.ctypes.data_as(u64p), os_.ctypes.data_as(f32p), oc.ctypes.data_as(u32p))
    assert st == INVALID_ARG and "null index" in bn.last_error()
    # an empty index: count 0
    empty = bn.Index(0, 128, 10)
    ids, sc, cnt = empty.search_peaks(q[None], 4, 2)
    assert cnt.tolist() == [0] and np.isnan(sc).all()


# ---- 5. no effect on other state ------------------------------------------------------------------------------------------------------
def test_radius_zero_is_the_exact_search_at_many_tiles(bn):
    exact.require_many_tiles()
    case = ordered_case("random")
    for M in (1, 256):
        for a, b in zip(case.idx.search_peaks(case.Q, M, 0), case.idx.search(case.Q, M)):
            assert a.tobytes() == b.tobytes(), M
    qi = [0, 1, N - 1, 77777]
    for a, b in zip(case.idx.search_peaks_ids(qi, 100, 0, exclude_radius=5), case.idx.search_ids(qi, 100, exclude_radius=5)):
        assert a.tobytes() == b.tobytes()


def test_other_searches_tags_and_appends(bn):
    g = general(130)
    before = [a.tobytes() for a in g.idx.search(g.Q, 100)]
    tagged = [a.tobytes() for a in g.idx.search_peaks(g.Q, 100, 8)]
    assert [a.tobytes() for a in g.idx.search(g.Q, 100)] == before, "the two share the candidate buffers"
    assert [a.tobytes() for a in g.idx.search_peaks(g.Q, 100, 0)] == before
    plain = bn.Index(0, 130, g.n)
    plain.add(g.X)
    assert [a.tobytes() for a in plain.search_peaks(g.Q, 100, 8)] == tagged, "tags are not consulted"
    # rows appended after a call are seen by the next one
    rng = np.random.default_rng(73)
    X = ir.rows_at_levels(rng, rng.integers(-64, 65, 333), 128, 64)
    Q = exact.queries(rng, 128, 64, 5)
    S, qbad, xbad = ir.scores64(Q, X)
    idx = bn.Index(0, 128, 400)
    prev = 0
    for n in (100, 128, 129, 333):
        assert idx.add(X[prev:n]) == prev
        prev = n
        for radius in (1, 5, 64):
            want = peaks_ref.peaks_top_m(S[:, :n], peaks_ref.eligibility(n, qbad, xbad), radius, 256)
            exact.assert_exact(idx.search_peaks(Q, 256, radius), want, ("grown to", n, "radius", radius))
