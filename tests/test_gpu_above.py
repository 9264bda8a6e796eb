"""bn_index_search_above / bn_index_search_above_ids on the GPU.  Every comparison uses == on counts, ids, score bytes and tags.  Expected
results come from tests/above_ref.py over index_ref.scores64, which is exact for the dyadic rows used (most rows tie, and thresholds sit
exactly on a score level), or, for general data, from bn_index_search's own lists.

The shapes: dim 128 and N = 8 * 64 * 320 + 37 rows (test_gpu_index_exact.N): at least 8 tiles per workgroup on any device of <= 320
compute units, and a ragged last tile.  require_many_tiles fails loudly on a device where that no longer holds."""
import ctypes as C
import functools

import numpy as np
import pytest

import above_ref
import index_ref as ir
import test_gpu_index_exact as exact

pytestmark = pytest.mark.gpu
INVALID_ARG = 1
TILE = exact.TILE
N = exact.N
NQ = 70                                                      # a pass of 64 and a second pass of 6
ORDERS = ("rising", "tile_rising", "constant", "random")
MAX_HITS = (0, 1, 63, 64, 65, 1000, 65536)                   # 65536: more than the count of some queries
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
INF = float("inf")


def assert_same(got, want, what):
    """(ids, scores, tags, counts) against (ids, scores, tags, counts), every byte"""
    exact.assert_exact((got[0], got[1], got[3]), (want[0], want[1], want[3]), what)
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), (what, "tags")


def thresholds(order, nq=NQ):
    """one min_score per query, each exactly on a score level k / 64.  Query 0 is the canonical query, whose level of every row is known"""
    q = np.arange(nq)
    thr = ((q % 9) - 2) / 32.0
    thr[q % 11 == 10] = 0.5                                  # next to no hits
    thr[0] = 3 / 64 if order == "constant" else 40 / 64       # constant: every row scores exactly 3/64
    return thr.astype(np.float32)


@functools.lru_cache(maxsize=None)
def ordered_case(order):
    bn = __import__("importlib").import_module("rust-birdnet-onnx_amd")
    rng = np.random.default_rng([128, 64, 9, ORDERS.index(order)])
    lv = exact.levels(order, N, 64, rng)
    case = exact.Case(bn, ir.rows_at_levels(rng, lv, 128, 64), exact.queries(rng, 128, 64, NQ))
    case.levels = lv
    case.thr = thresholds(order)
    case.hits = above_ref.hits_from_scores(case.S, case.qbad, case.xbad, case.thr)
    return case


# ---- 1. levels and ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_levels_and_ties_many_tiles_per_workgroup(bn, order):
    """rows equal to the threshold are hits, rows one level below are not; the count is the untruncated total, the list the first max_hits"""
    exact.require_many_tiles()
    case = ordered_case(order)
    s0 = case.S[0].astype(np.float32)
    assert (s0 == case.thr[0]).any(), "no row ties with query 0's threshold"
    if order != "constant":
        assert (s0 == case.thr[0] - np.float32(1 / 64)).any(), "no row sits one level below query 0's threshold"
        assert len(case.hits[0][0]) == int((case.levels >= 40).sum())
    else:
        assert len(case.hits[0][0]) == N
    totals = np.array([len(h[0]) for h in case.hits])
    assert (totals < 1000).any() and (totals > 65536).any() and ((totals > 1000) & (totals < 65536)).any(), "the max_hits grid must cut some lists and not others"
    for nq in (1, 17, 64, 70):
        for max_hits in MAX_HITS:
            got = case.idx.search_above(case.Q[:nq], case.thr[:nq], max_hits)
            assert_same(got, above_ref.layout(case.hits[:nq], max_hits), (order, "Q", nq, "max_hits", max_hits))
        assert np.array_equal(case.idx.count_above(case.Q[:nq], case.thr[:nq]), totals[:nq].astype(np.uint32))
    # a scalar threshold, a stride wider than max_hits
    hits = above_ref.hits_from_scores(case.S[:17], case.qbad[:17], case.xbad, 0.125)
    assert_same(case.idx.search_above(case.Q[:17], 0.125, 65, h_stride=70), above_ref.layout(hits, 65, 70), (order, "stride"))


# ---- 2. truncation at workgroup edges ------------------------------------------------------------------------------------------------
def test_truncation_at_workgroup_edges(bn):
    cus = exact.require_many_tiles()
    tpw, n_wg = exact.tiles_per_workgroup(N, cus)
    wg = tpw * TILE
    assert tpw >= 4 and n_wg > 3 and (n_wg - 1) * wg + 40 < N
    rng = np.random.default_rng(83)
    lv = rng.integers(-64, 1, N)                            # nothing else reaches 0.5
    lv[wg + 10:wg + 160] = 64                               # 150 hits of query 0 in workgroup 1, across three tiles
    lv[2 * wg:2 * wg + 70] = 64                             # 70 at the very start of workgroup 2
    lv[N - 5] = 64
    X = ir.rows_at_levels(rng, lv, 128, 64)
    Q = exact.queries(rng, 128, 64, 3)
    last = np.arange((n_wg - 1) * wg + 3, (n_wg - 1) * wg + 40, 3)
    X[last] = Q[1]                                          # query 1 scores 1.0 on these rows of the last workgroup only
    case = exact.Case(bn, X, Q)
    thr = np.array([0.5, 1.0, -1.0], dtype=np.float32)      # query 2: every row is a hit, workgroup 0 alone exceeds any max_hits below
    hits = above_ref.hits_from_scores(case.S, case.qbad, case.xbad, thr)
    h0 = hits[0][0]
    assert len(h0) >= 221 and h0[:150].tolist() == list(range(wg + 10, wg + 160)) and h0[150:220].tolist() == list(range(2 * wg, 2 * wg + 70))
    assert hits[1][0].min() >= (n_wg - 1) * wg and set(last.tolist()) <= set(hits[1][0].tolist()), "query 1's hits all lie in the last workgroup"
    assert len(hits[2][0]) == N
    # 100: the cut falls inside a tile of workgroup 1; 150: exactly between workgroups 1 and 2; 151 and 220: just after an edge; wg and
    # wg + 1: query 2's cut exactly at the end of workgroup 0 and one entry into workgroup 1; 5: inside query 1's only workgroup
    for max_hits in (1, 5, 64, 100, 149, 150, 151, 219, 220, 221, wg - 1, wg, wg + 1, 2 * wg, 65536):
        for nq in (1, 3):
            got = case.idx.search_above(Q[:nq], thr[:nq], max_hits)
            assert_same(got, above_ref.layout(hits[:nq], max_hits), ("edges", "max_hits", max_hits, "Q", nq))


# ---- 3. range and paging -----------------------------------------------------------------------------------------------------------------
def test_ranges_and_paging(bn):
    cus = exact.require_many_tiles()
    case = ordered_case("random")
    nq = 17
    Q, thr = case.Q[:nq], case.thr[:nq]
    wg = exact.tiles_per_workgroup(N, cus)[0] * TILE
    ranges = [(70, 30), (64, 64), (63, 2), (1, 0), (N - 37, 0), (N - 1, 1), (wg - 5, wg + 11), (1000, 100_003), (3 * wg + 17, 5 * wg + 70), (0, N), (N, 0), (500, 0)]
    for first, n_ids in ranges:
        hits = above_ref.hits_from_scores(case.S[:nq], case.qbad[:nq], case.xbad, thr, first, n_ids)
        for max_hits in (0, 7, 1000):
            got = case.idx.search_above(Q, thr, max_hits, first_id=first, n_ids=n_ids)
            assert_same(got, above_ref.layout(hits, max_hits), ("range", first, n_ids, "max_hits", max_hits))
    # paging: max_hits = 100, the next page starts at the last returned id + 1; the pages are the unpaged list, score bits included
    for q in (0, 1, 5):
        want_ids, want_sc = case.hits[q]
        assert 300 < len(want_ids), "several pages"
        first, end = 1234, 150_001
        keep = (want_ids >= first) & (want_ids < end)
        want_ids, want_sc = want_ids[keep][:2050], want_sc[keep][:2050]
        got_ids, got_sc, pages = [], [], 0
        while len(got_ids) < len(want_ids):
            ids, sc, _, cnt = case.idx.search_above(case.Q[q:q + 1], case.thr[q:q + 1], 100, first_id=first, n_ids=end - first)
            k = min(int(cnt[0]), 100)
            assert k > 0
            got_ids += ids[0, :k].tolist()
            got_sc.append(sc[0, :k])
            first, pages = int(ids[0, k - 1]) + 1, pages + 1
            if cnt[0] <= 100:
                break
        assert pages >= 4 and got_ids[:len(want_ids)] == want_ids.tolist() and np.concatenate(got_sc)[:len(want_ids)].tobytes() == want_sc.tobytes(), q


# ---- 4. general data, against bn_index_search ---------------------------------------------------------------------------------------
class General:
    """Gaussian rows, dim 200 (two k chunks, the second padded), N = 20 000, 70 queries.  For seed 97 the float64 scores of every query
    (and of the 20 stored rows the _ids test draws, at every exclusion radius it uses) drop by more than 0.019 between rank 100 and
    rank 256 (checked on the CPU; an f32 score of unit rows of this dim is within 1e-5 of it), so the rank-256 score lies below the
    rank-100 score and the top 256 hold every row at or above it.  The tests assert that from the search result itself"""

    def __init__(self, bn):
        rng = np.random.default_rng(97)
        self.n, self.dim = 20_000, 200
        self.X = rng.standard_normal((self.n, self.dim), dtype=np.float32)
        self.Q = rng.standard_normal((NQ, self.dim), dtype=np.float32)
        self.idx = bn.Index(0, self.dim, self.n)
        assert self.idx.add(self.X) == 0


@functools.lru_cache(maxsize=1)
def general():
    return General(__import__("importlib").import_module("rust-birdnet-onnx_amd"))


def expect_from_top(top, thr, max_hits):
    """the entries of a top-256 list with score >= thr, re-sorted by id, in the binding's layout"""
    ids, sc, cnt = top
    hits = []
    for q in range(len(cnt)):
        keep = np.flatnonzero(sc[q, :cnt[q]] >= thr[q])
        order = keep[np.argsort(ids[q, keep], kind="stable")]
        hits.append((ids[q, order].astype(np.int64), sc[q, order]))
    return above_ref.layout(hits, max_hits)


def test_general_data_against_the_exact_search(bn):
    g = general()
    top = g.idx.search(g.Q, 256)
    assert (top[2] == 256).all()
    thr = top[1][:, 99].copy()
    assert (top[1][:, 255] < thr).all(), "precondition: the rank-256 score lies below the threshold, so the top 256 hold every hit"
    for nq in (1, 17, 70):
        for max_hits in (0, 50, 100, 256):
            got = g.idx.search_above(g.Q[:nq], thr[:nq], max_hits)
            want = expect_from_top(tuple(a[:nq] for a in top), thr[:nq], max_hits)
            assert_same(got, want, ("general", "Q", nq, "max_hits", max_hits))
            assert (got[3] >= 100).all()
    # the same bits inside a range and for one query alone: the score depends on the query and the row only
    ids, sc, _, cnt = g.idx.search_above(g.Q[5:6], thr[5:6], 256, first_id=777, n_ids=15_000)
    full = expect_from_top(tuple(a[5:6] for a in top), thr[5:6], 256)
    keep = (full[0][0, :full[3][0]] >= 777) & (full[0][0, :full[3][0]] < 15_777)
    assert cnt[0] == keep.sum() and np.array_equal(ids[0, :cnt[0]], full[0][0, :full[3][0]][keep]) and sc[0, :cnt[0]].tobytes() == full[1][0, :full[3][0]][keep].tobytes()


# ---- 5. the _ids form ------------------------------------------------------------------------------------------------------------------
def test_search_above_ids_against_the_reference_and_search_ids(bn):
    exact.require_many_tiles()
    case = ordered_case("rising")
    rng = np.random.default_rng(101)
    top = int(np.flatnonzero(case.levels == 64)[0])          # the best level's rows are near-duplicates of each other for query 0 only
    qi = np.concatenate([[0, 1, 63, 64, 65, N - 1, top, top + 1], rng.integers(0, N, 9)]).astype(np.int64)
    S, qbad, xbad = ir.scores64(case.X[qi], case.X)
    thr = np.full(len(qi), 20 / 64, dtype=np.float32)
    thr[1] = 1.0                                             # only the row itself and exact copies of it
    for ex in (-1, 0, 2):
        hits = above_ref.hits_from_scores(S, qbad, xbad, thr, qid=qi, exclude_radius=ex)
        for max_hits in (0, 10, 5000):
            got = case.idx.search_above_ids(qi, thr, max_hits, exclude_radius=ex)
            assert_same(got, above_ref.layout(hits, max_hits), ("ids", "exclude", ex, "max_hits", max_hits))
        for q in range(len(qi)):
            own = np.abs(hits[q][0] - qi[q]) <= max(ex, 0)
            assert own.any() == (ex < 0), "the query's own row is a hit exactly when nothing is excluded"
        ranged = above_ref.hits_from_scores(S, qbad, xbad, thr, 100, N - 300, qid=qi, exclude_radius=ex)
        assert_same(case.idx.search_above_ids(qi, thr, 40, exclude_radius=ex, first_id=100, n_ids=N - 300), above_ref.layout(ranged, 40), ("ids, range", ex))
    # general data against search_ids: the hits are the entries of its top 256 at or above its rank-100 score
    g = general()
    gi = rng.integers(0, g.n, 20)
    for ex in (-1, 0, 2):
        top256 = g.idx.search_ids(gi, 256, exclude_radius=ex)
        t = top256[1][:, 99].copy()
        assert (top256[2] == 256).all() and (top256[1][:, 255] < t).all()
        assert_same(g.idx.search_above_ids(gi, t, 256, exclude_radius=ex), expect_from_top(top256, t, 256), ("ids, general", ex))


# ---- 6. invalid rows and queries ---------------------------------------------------------------------------------------------------------
def test_invalid_rows_are_never_hits_and_invalid_queries_count_zero(bn):
    cus = exact.require_many_tiles()
    tpw, _ = exact.tiles_per_workgroup(N, cus)
    rng = np.random.default_rng(103)
    X = ir.rows_at_levels(rng, exact.levels("random", N, 64, rng), 128, 64)
    bad = exact.sprinkle_invalid(X, tpw)
    Q = exact.queries(rng, 128, 64, 6)
    Q[2] = 0
    Q[4, 9] = np.inf
    case = exact.Case(bn, X, Q)
    assert np.array_equal(np.flatnonzero(case.xbad), bad) and np.flatnonzero(case.qbad).tolist() == [2, 4]
    thr = np.array([-INF, 0.0, -INF, 0.25, -INF, INF], dtype=np.float32)
    hits = above_ref.hits_from_scores(case.S, case.qbad, case.xbad, thr)
    for first, n_ids in ((0, 0), (5 * TILE - 3, 4 * TILE + 9), (N - 100, 100)):
        hits = above_ref.hits_from_scores(case.S, case.qbad, case.xbad, thr, first, n_ids)
        got = case.idx.search_above(Q, thr, 65536, first_id=first, n_ids=n_ids)
        assert_same(got, above_ref.layout(hits, 65536), ("invalid", first, n_ids))
        lo, hi = above_ref.id_range(N, first, n_ids)
        assert got[3][0] == (hi - lo) - int(case.xbad[lo:hi].sum()), "at -inf the count is the number of valid rows of the range"
        assert got[3].tolist()[2] == 0 and got[3][4] == 0 and got[3][5] == 0, "a zero query, a non-finite query and +inf give count 0"
        assert not np.isin(got[0][0, :min(int(got[3][0]), 65536)], bad).any()
    assert np.array_equal(case.idx.count_above(Q, thr), np.array([len(h[0]) for h in above_ref.hits_from_scores(case.S, case.qbad, case.xbad, thr)], dtype=np.uint32))


# ---- 7. tags ---------------------------------------------------------------------------------------------------------------------------
def test_tags_of_the_hits(bn):
    rng = np.random.default_rng(107)
    n = 5 * TILE + 11
    X = ir.rows_at_levels(rng, rng.integers(-64, 65, n), 128, 64)
    Q = exact.queries(rng, 128, 64, 5)
    case = exact.Case(bn, X, Q, capacity=n + 100)
    hits = above_ref.hits_from_scores(case.S, case.qbad, case.xbad, 0.0)
    got = case.idx.search_above(Q, 0.0, 400)
    assert_same(got, above_ref.layout(hits, 400), "never tagged: zeros")
    assert got[3].min() > 10
    tags = rng.integers(0, 65536, n).astype(np.uint32)
    case.idx.set_tags(0, tags)
    assert np.array_equal(case.idx.tags(), tags)
    for max_hits in (3, 400):
        got = case.idx.search_above(Q, 0.0, max_hits)
        assert_same(got, above_ref.layout(hits, max_hits, tags=tags), ("tagged", max_hits))
        for q in range(5):
            k = min(int(got[3][q]), max_hits)
            assert np.array_equal(got[2][q, :k], tags[got[0][q, :k].astype(np.int64)])
    # tag_out = NULL
    ids, sc, cnt = np.zeros((5, 400), dtype=np.uint64), np.full((5, 400), np.nan, dtype=np.float32), np.zeros(5, dtype=np.uint32)
    thr = np.zeros(5, dtype=np.float32)
    st = bn.lib.bn_index_search_above(case.idx._h, Q.ctypes.data_as(f32p), 5, thr.ctypes.data_as(f32p), 0, 0, 400, 400, ids.ctypes.data_as(u64p),
                                      sc.ctypes.data_as(f32p), None, cnt.ctypes.data_as(u32p))
    assert st == 0 and np.array_equal(ids, got[0]) and sc.tobytes() == got[1].tobytes() and np.array_equal(cnt, got[3])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone_and_empty_cases_are_ok(bn):
    rng = np.random.default_rng(109)
    n = 200
    idx = bn.Index(0, 128, n + 50)
    idx.add(ir.dyadic_rows(rng, n, 128, 64))
    Q = exact.queries(rng, 128, 64, 2)
    qi = np.array([5, 7], dtype=np.uint64)
    thr = np.zeros(2, dtype=np.float32)
    nan = np.array([0.0, np.nan], dtype=np.float32)
    oi, os_, ot, oc = np.full(8, 0xABCDEF, dtype=np.uint64), np.full(8, -7.5, dtype=np.float32), np.full(8, 0xBEEF, dtype=np.uint32), np.full(2, 77, dtype=np.uint32)
    before = tuple(a.tobytes() for a in (oi, os_, ot, oc))
    outs = (oi.ctypes.data_as(u64p), os_.ctypes.data_as(f32p), ot.ctypes.data_as(u32p), oc.ctypes.data_as(u32p))
    qp, qip, tp, np_ = Q.ctypes.data_as(f32p), qi.ctypes.data_as(u64p), thr.ctypes.data_as(f32p), nan.ctypes.data_as(f32p)

    def refused(msg, x, queries, ids, n_q, t, first, n_ids, max_hits, stride, o=outs):
        a = bn.lib.bn_index_search_above(x, queries, n_q, t, first, n_ids, max_hits, stride, *o)
        ma = bn.last_error()
        b = bn.lib.bn_index_search_above_ids(x, ids, n_q, 0, t, first, n_ids, max_hits, stride, *o)
        assert a == INVALID_ARG and b == INVALID_ARG and msg in ma and msg in bn.last_error(), (msg, a, b, ma, bn.last_error())
        assert tuple(z.tobytes() for z in (oi, os_, ot, oc)) == before, msg

    refused("past", idx._h, qp, qip, 2, tp, n + 1, 0, 4, 4)
    refused("past", idx._h, qp, qip, 2, tp, 0, n + 1, 4, 4)
    refused("past", idx._h, qp, qip, 2, tp, n - 1, 2, 4, 4)
    refused("null index", None, qp, qip, 2, tp, 0, 0, 4, 4)
    refused("null", idx._h, None, None, 2, tp, 0, 0, 4, 4)
    refused("null", idx._h, qp, qip, 2, None, 0, 0, 4, 4)
    refused("null", idx._h, qp, qip, 2, tp, 0, 0, 4, 4, (outs[0], outs[1], outs[2], None))
    refused("null", idx._h, qp, qip, 2, tp, 0, 0, 4, 4, (None, outs[1], outs[2], outs[3]))
    refused("null", idx._h, qp, qip, 2, tp, 0, 0, 4, 4, (outs[0], None, outs[2], outs[3]))
    refused("max_hits", idx._h, qp, qip, 2, tp, 0, 0, 65537, 65537)
    refused("h_stride", idx._h, qp, qip, 2, tp, 0, 0, 4, 3)
    refused("NaN", idx._h, qp, qip, 2, np_, 0, 0, 4, 4)
    refused("NaN", idx._h, qp, qip, 2, np_, 0, 0, 0, 0)
    big = np.array([5, n], dtype=np.uint64)
    st = bn.lib.bn_index_search_above_ids(idx._h, big.ctypes.data_as(u64p), 2, -1, tp, 0, 0, 4, 4, *outs)
    assert st == INVALID_ARG and str(n) in bn.last_error() and tuple(z.tobytes() for z in (oi, os_, ot, oc)) == before
    # the legal empty cases
    assert bn.lib.bn_index_search_above(idx._h, None, 0, None, 0, 0, 4, 4, None, None, None, None) == 0
    assert bn.lib.bn_index_search_above_ids(idx._h, None, 0, -1, None, 0, 0, 4, 4, None, None, None, None) == 0
    assert bn.lib.bn_index_search_above(idx._h, qp, 2, tp, n, 0, 4, 4, *outs) == 0 and oc.tolist() == [0, 0], "an empty range at the very end"
    assert tuple(a.tobytes() for a in (oi, os_, ot)) == before[:3]
    empty = bn.Index(0, 128, 10)
    ids, sc, tg, cnt = empty.search_above(Q, -INF, 4)
    assert cnt.tolist() == [0, 0] and np.isnan(sc).all() and not ids.any() and not tg.any()
    assert empty.count_above(Q, -INF).tolist() == [0, 0]
    assert idx.search_above(Q, -INF, 4, first_id=50, n_ids=0)[3].tolist() == [n - 50, n - 50]


# ---- 9. nothing else moves -------------------------------------------------------------------------------------------------------------
def test_other_calls_are_unchanged_and_two_calls_give_the_same_bytes(bn):
    exact.require_many_tiles()
    case = ordered_case("random")
    qi = [0, 1, N - 1, 77777]
    tags = (np.arange(1000) % 65536).astype(np.uint32)
    case.idx.set_tags(5000, tags)

    def others():
        return [a.tobytes() for a in case.idx.search(case.Q, 100)] + [a.tobytes() for a in case.idx.search_ids(qi, 100, exclude_radius=5)] + \
            [case.idx.tags(4990, 1020).tobytes(), case.idx.read(N - 200, 200).tobytes()]

    before = others()
    first = [a.tobytes() for a in case.idx.search_above(case.Q, case.thr, 1000)]
    assert others() == before
    counts = case.idx.count_above(case.Q, case.thr).tobytes()
    by_id = [a.tobytes() for a in case.idx.search_above_ids(qi, 0.25, 65536, exclude_radius=2)]
    assert others() == before
    assert [a.tobytes() for a in case.idx.search_above(case.Q, case.thr, 1000)] == first
    assert case.idx.count_above(case.Q, case.thr).tobytes() == counts
    assert [a.tobytes() for a in case.idx.search_above_ids(qi, 0.25, 65536, exclude_radius=2)] == by_id
    case.idx.fill_tags(5000, 1000, 0)                        # the shared case goes back as it was found
