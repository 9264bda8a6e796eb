"""bn_index_group_above / bn_index_group_above_ids on the GPU.  Every comparison uses == on every output byte.  Expected results come from
tests/group_above_ref.py over index_ref.scores64, which is exact for the dyadic rows used (most rows tie, and thresholds sit exactly on
a score level), or, for general data, from bn_index_search_above's own lists and the tag plane.

The shapes are test_gpu_index_exact's: dim 128 and N = 8 * 64 * 320 + 37 rows, so a workgroup owns several tiles and the last tile is
ragged; 70 queries are a pass of 64 and a pass of 6.  The ordered cases (rows, queries, thresholds, float64 scores, the index) are
test_gpu_above's, built once per session; a test that tags such an index sets the tags back to 0 before it ends."""
import ctypes as C
import itertools

import numpy as np
import pytest

import above_ref
import group_above_ref as gref
import index_ref as ir
import test_gpu_above as above_t
import test_gpu_index_exact as exact

pytestmark = pytest.mark.gpu
INVALID_ARG = 1
TILE = exact.TILE
N = exact.N
NQ = above_t.NQ
ORDERS = above_t.ORDERS
GROUPS = (1, 2, 63, 64, 65, 1000, 65536)
QS = (1, 17, 64, 70)
NO_ROW = gref.NO_ROW
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
INF = float("inf")


def workgroup_rows():
    return exact.tiles_per_workgroup(N, exact.require_many_tiles())[0] * TILE


def tag_pattern(name, rng, wg):
    if name == "runs":
        # uneven contiguous runs: edges inside tiles (37, 100, ...), exactly on a tile edge (6400), inside a workgroup's first tile and
        # exactly on a workgroup edge; tags in and out of every n_groups of the grid; tag 7 comes twice
        edges = sorted({37, 100, 101, 6400, wg + 5, 2 * wg, 3 * wg - 1, 70_000, 70_001, 120_003, N - 40, N - 1})
        tags_of_runs = [0, 1, 62, 63, 64, 7, 65, 999, 1000, 40_000, 65_535, 7, 2]
        assert len(tags_of_runs) == len(edges) + 1
        return np.repeat(np.array(tags_of_runs, dtype=np.uint32), np.diff([0] + edges + [N]))
    if name == "random":
        return rng.integers(0, 65536, N).astype(np.uint32)
    if name == "one":
        return np.full(N, 5, dtype=np.uint32)
    assert name == "few"                                     # neighbours differ, few groups: many per-lane updates of one record
    return rng.integers(0, 3, N).astype(np.uint32) * 32


class Tagged:
    """the shared ordered case with a tag pattern on, every tag back to 0 on the way out"""

    def __init__(self, case, tags):
        self.case, self.tags = case, tags

    def __enter__(self):
        self.case.idx.set_tags(0, self.tags)
        return self.case

    def __exit__(self, *exc):
        self.case.idx.fill_tags(0, N, 0)


# ---- 1. levels and ties ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_levels_and_ties_tag_patterns_groups_and_queries(bn, order):
    wg = workgroup_rows()
    case = above_t.ordered_case(order)
    hit = above_ref.hit_mask(case.S, case.qbad, case.xbad, case.thr)
    s0 = case.S[0].astype(np.float32)
    assert (s0 == case.thr[0]).any(), "no row ties with query 0's threshold"
    rng = np.random.default_rng([7, ORDERS.index(order)])
    seen = set()
    for name in ("runs", "random", "one", "few"):
        tags = tag_pattern(name, rng, wg)
        full = gref.records(hit, case.S, tags, 65536)
        assert np.array_equal(full[6], np.array([len(h[0]) for h in case.hits], dtype=np.uint32)), "the reference's totals are above_ref's"
        seen |= {"empty"} if (full[0] == 0).any() else set()
        seen |= {"single"} if (full[0] == 1).any() else set()
        seen |= {"large"} if (full[0] > 65536).any() else set()
        with Tagged(case, tags):
            for n_groups in GROUPS:
                for nq in QS:
                    got = case.idx.group_above(case.Q[:nq], case.thr[:nq], n_groups)
                    gref.assert_same(got, gref.narrowed(full, hit, tags, n_groups, nq), (order, name, "groups", n_groups, "Q", nq))
            # a stride wider than n_groups: the entries past n_groups keep the binding's fills
            got = case.idx.group_above(case.Q[:17], case.thr[:17], 65, g_stride=70)
            gref.assert_same(got, gref.narrowed(full, hit, tags, 65, 17, 70), (order, name, "stride"))
    assert seen == {"empty", "single", "large"}, seen


# ---- 2. the best hit's tie rule ----------------------------------------------------------------------------------------------------
def test_best_hit_ties_across_tiles_and_workgroups_go_to_the_lowest_id(bn):
    wg = workgroup_rows()
    rng = np.random.default_rng(211)
    lv = rng.integers(-64, 1, N)                             # nothing else reaches the threshold of query 0
    first, n_ids = 70, N - 70 - 5                            # the range: [70, N - 5)
    last = first + n_ids - 1
    # group 3: ties at its maximum (level 48) in three tiles of three workgroups, lower levels at the ends of the range
    top = [2 * wg + 17, 2 * wg + 17 + TILE, 3 * wg + 1, 5 * wg + 63]
    lv[top] = 48
    lv[[first, last]] = 40
    lv[[first - 1, last + 1]] = 64                           # better rows just outside the range
    # group 4: the maximum ties inside one tile and with a row of the next workgroup; one lower row before them
    top4 = [wg - TILE + 9, wg - TILE + 40, wg + 2]
    lv[top4] = 56
    lv[wg - 3 * TILE] = 33
    tags = np.zeros(N, dtype=np.uint32)
    tags[top + [first, last, first - 1, last + 1]] = 3
    tags[top4 + [wg - 3 * TILE]] = 4
    X = ir.rows_at_levels(rng, lv, 128, 64)
    Q = exact.queries(rng, 128, 64, 3)
    case = exact.Case(bn, X, Q)
    case.idx.set_tags(0, tags)
    thr = np.array([32 / 64, -INF, 0.0], dtype=np.float32)
    want = gref.from_scores(case.S, case.qbad, case.xbad, thr, 6, tags, first, n_ids)
    assert want[0][0].tolist() == [0, 0, 0, 6, 4, 0] and want[1][0, 3] == min(top) and want[3][0, 3] == first and want[4][0, 3] == last
    assert want[1][0, 4] == min(top4) and want[3][0, 4] == wg - 3 * TILE and want[4][0, 4] == wg + 2
    assert want[2][0, 3] == np.float32(48 / 64) and want[2][0, 4] == np.float32(56 / 64)
    for nq in (1, 3):
        got = case.idx.group_above(Q[:nq], thr[:nq], 6, first_id=first, n_ids=n_ids)
        gref.assert_same(got, tuple(a[:nq] for a in want), ("tie rule", nq))
    # the whole index: the better rows outside the former range now win, and lie at the ends of group 3
    whole = gref.from_scores(case.S, case.qbad, case.xbad, thr, 6, tags)
    assert whole[1][0, 3] == first - 1 and whole[4][0, 3] == last + 1
    gref.assert_same(case.idx.group_above(Q, thr, 6), whole, "tie rule, whole index")


# ---- 3. ranges and exclusion -----------------------------------------------------------------------------------------------------------
def test_ranges_and_exclusion_and_totals_equal_the_threshold_count(bn):
    wg = workgroup_rows()
    case = above_t.ordered_case("random")
    nq = 17
    Q, thr = case.Q[:nq], case.thr[:nq]
    rng = np.random.default_rng(223)
    tags = tag_pattern("runs", rng, wg)
    ranges = [(70, 30), (64, 64), (63, 2), (1, 0), (N - 37, 0), (N - 1, 1), (wg - 5, wg + 11), (1000, 100_003), (3 * wg + 17, 5 * wg + 70), (0, N), (N, 0), (500, 0)]
    with Tagged(case, tags):
        for first, n_ids in ranges:
            want = gref.from_scores(case.S[:nq], case.qbad[:nq], case.xbad, thr, 66, tags, first, n_ids)
            got = case.idx.group_above(Q, thr, 66, first_id=first, n_ids=n_ids)
            gref.assert_same(got, want, ("range", first, n_ids))
            assert np.array_equal(got[6], case.idx.count_above(Q, thr, first_id=first, n_ids=n_ids)), ("total", first, n_ids)
        # stored rows as queries, with and without their neighbourhood
        top = int(np.flatnonzero(case.levels == 64)[0])
        qi = np.concatenate([[0, 1, 63, 64, 65, N - 1, top, wg, wg - 1], rng.integers(0, N, 8)]).astype(np.int64)
        S, qbad, xbad = ir.scores64(case.X[qi], case.X)
        t = np.full(len(qi), 20 / 64, dtype=np.float32)
        t[1] = 1.0                                           # only the row itself and exact copies of it
        t[2] = -INF
        for ex in (-1, 0, 3):
            for first, n_ids in ((0, 0), (100, N - 300), (wg - 5, wg + 11)):
                want = gref.from_scores(S, qbad, xbad, t, 66, tags, first, n_ids, qid=qi, exclude_radius=ex)
                got = case.idx.group_above_ids(qi, t, 66, exclude_radius=ex, first_id=first, n_ids=n_ids)
                gref.assert_same(got, want, ("ids", ex, first, n_ids))
                count = case.idx.search_above_ids(qi, t, 0, exclude_radius=ex, first_id=first, n_ids=n_ids)[3]
                assert np.array_equal(got[6], count), ("ids, total", ex, first, n_ids)


# ---- 4. general data, against bn_index_search_above -------------------------------------------------------------------------------------
def test_general_data_against_the_threshold_search_and_the_tag_plane(bn):
    g = above_t.general()
    rng = np.random.default_rng(227)
    tags = rng.integers(0, 300, g.n).astype(np.uint32)
    g.idx.set_tags(0, tags)
    try:
        thr = (0.02 * rng.standard_normal(NQ)).astype(np.float32)   # about half of the rows each
        thr[3], thr[4] = 0.2, -INF
        ids, sc, tg, cnt = g.idx.search_above(g.Q, thr, 65536)
        assert cnt.max() <= 65536 and cnt.min() > 0 and cnt[4] == g.n, "every hit must be in the lists"
        plane = g.idx.tags()
        assert np.array_equal(plane, tags)
        for n_groups in (300, 256, 7):
            want = [np.zeros((NQ, n_groups), dtype=np.uint32), np.full((NQ, n_groups), NO_ROW, dtype=np.uint64), np.zeros((NQ, n_groups), dtype=np.float32),
                    np.full((NQ, n_groups), NO_ROW, dtype=np.uint64), np.full((NQ, n_groups), NO_ROW, dtype=np.uint64), np.zeros(NQ, dtype=np.uint32), cnt.copy()]
            for q in range(NQ):
                i, s = ids[q, :cnt[q]].astype(np.int64), sc[q, :cnt[q]]
                t = plane[i].astype(np.int64)
                keep = t < n_groups
                want[5][q] = (~keep).sum()
                i, s, t = i[keep], s[keep], t[keep]
                want[0][q] = np.bincount(t, minlength=n_groups)
                want[4][q][t] = i                            # ids ascend: the last assignment is the largest
                want[3][q][t[::-1]] = i[::-1]
                order = np.lexsort((i, -s.astype(np.float64)))[::-1]   # worst first, so the best is assigned last
                want[1][q][t[order]] = i[order]
                want[2][q][t[order]] = s[order]
            for nq in (1, 17, 70):
                got = g.idx.group_above(g.Q[:nq], thr[:nq], n_groups)
                gref.assert_same(got, tuple(a[:nq] for a in want), ("general", n_groups, nq))
    finally:
        g.idx.fill_tags(0, g.n, 0)


# ---- 5. the tag plane ------------------------------------------------------------------------------------------------------------------
def test_an_untagged_index_is_one_group_and_tagging_regroups(bn):
    rng = np.random.default_rng(229)
    n = 9 * TILE + 11
    X = ir.rows_at_levels(rng, rng.integers(-64, 65, n), 128, 64)
    Q = exact.queries(rng, 128, 64, 5)
    case = exact.Case(bn, X, Q, capacity=n + 100)
    thr = np.array([0.0, 0.25, -INF, INF, -0.5], dtype=np.float32)

    def others():
        return [a.tobytes() for a in case.idx.search(Q, 100)] + [case.idx.count_above(Q, thr).tobytes()] + \
            [a.tobytes() for a in case.idx.search_above(Q, thr, 50)] + [case.idx.read().tobytes()]

    before = others()
    never = case.idx.group_above(Q, thr, 4)
    gref.assert_same(never, gref.from_scores(case.S, case.qbad, case.xbad, thr, 4), "never tagged")
    assert np.array_equal(never[0][:, 0], never[6]) and not never[0][:, 1:].any() and not never[5].any() and never[6][2] == n and never[6][3] == 0
    assert others() == before
    tags = rng.integers(0, 6, n).astype(np.uint32)
    case.idx.set_tags(0, tags)
    tagged = others()
    assert tagged[:4] == before[:4] and tagged[-1] == before[-1], "tags change no search, no count and no row"
    got = case.idx.group_above(Q, thr, 4)
    gref.assert_same(got, gref.from_scores(case.S, case.qbad, case.xbad, thr, 4, tags), "tagged")
    assert got[5].any() and (got[0][:, 1:] > 0).any() and np.array_equal(got[6], never[6])
    assert np.array_equal(case.idx.tags(), tags) and others() == tagged
    case.idx.set_tags(5, np.full(20, 3, dtype=np.uint32))    # the plane as it is at the call
    tags[5:25] = 3
    retagged = others()
    gref.assert_same(case.idx.group_above(Q, thr, 4), gref.from_scores(case.S, case.qbad, case.xbad, thr, 4, tags), "retagged")
    assert others() == retagged and retagged[:4] == before[:4]


# ---- 6. pass width and optional outputs ------------------------------------------------------------------------------------------------
def fresh(nq, g_stride):
    """the seven output arrays filled with sentinels"""
    return [np.full(nq * g_stride, 77, dtype=np.uint32), np.full(nq * g_stride, 0xABCDEF, dtype=np.uint64), np.full(nq * g_stride, -7.5, dtype=np.float32),
            np.full(nq * g_stride, 0xABCDE0, dtype=np.uint64), np.full(nq * g_stride, 0xABCDE1, dtype=np.uint64), np.full(nq, 78, dtype=np.uint32),
            np.full(nq, 79, dtype=np.uint32)]


def raw(bn, idx, Q, thr, n_groups, keep=range(7), by_id=False, radius=-1, first=0, n_ids=0, g_stride=None):
    """the entry point itself, with NULL for the outputs not in `keep`: (status, the seven arrays, sentinels where nothing was written).
    Q: the query rows, or with by_id the query ids; None passes NULL.  thr: None passes NULL, for two queries"""
    nq = 2 if thr is None else len(thr)
    g_stride = n_groups if g_stride is None else g_stride
    arrays = fresh(nq, g_stride)
    ptrs = [a.ctypes.data_as(t) if i in keep else None for i, (a, t) in enumerate(zip(arrays, (u32p, u64p, f32p, u64p, u64p, u32p, u32p)))]
    tp = None if thr is None else np.ascontiguousarray(thr, dtype=np.float32)
    h = idx._h if idx is not None else None
    if by_id:
        ids = None if Q is None else np.ascontiguousarray(Q, dtype=np.uint64)
        st = bn.lib.bn_index_group_above_ids(h, None if ids is None else ids.ctypes.data_as(u64p), nq, radius, None if tp is None else tp.ctypes.data_as(f32p),
                                             first, n_ids, n_groups, g_stride, *ptrs)
    else:
        Q = None if Q is None else np.ascontiguousarray(Q, dtype=np.float32)
        st = bn.lib.bn_index_group_above(h, None if Q is None else Q.ctypes.data_as(f32p), nq, None if tp is None else tp.ctypes.data_as(f32p), first, n_ids,
                                         n_groups, g_stride, *ptrs)
    return st, arrays


def test_pass_width_and_null_outputs(bn):
    wg = workgroup_rows()
    case = above_t.ordered_case("tile_rising")
    rng = np.random.default_rng(233)
    tags = tag_pattern("random", rng, wg)
    with Tagged(case, tags):
        # 65536 groups: 48 queries per pass, so 70 queries are a pass of 48, one of 16 and one of 6
        together = case.idx.group_above(case.Q, case.thr, 65536)
        for q in (0, 1, 47, 48, 63, 64, 69):
            alone = case.idx.group_above(case.Q[q:q + 1], case.thr[q:q + 1], 65536)
            gref.assert_same(alone, tuple(a[q:q + 1] for a in together), ("alone", q))
        assert (together[0] > 0).any() and together[6].max() > 65536
        # the optional outputs in every combination: the pair, first, last, other, total
        st, every = raw(bn, case.idx, case.Q, case.thr, 65)
        assert st == 0
        hit = above_ref.hit_mask(case.S, case.qbad, case.xbad, case.thr)
        want = gref.records(hit, case.S, tags, 65)
        for got, w in zip(every, want):
            assert got.tobytes() == w.tobytes()
        for choice in itertools.product((False, True), repeat=5):
            keep = [0] + [i for c, part in zip(choice, ((1, 2), (3,), (4,), (5,), (6,))) if c for i in part]
            st, some = raw(bn, case.idx, case.Q, case.thr, 65, keep)
            assert st == 0, (keep, bn.last_error())
            for i, sentinel in enumerate(fresh(NQ, 65)):
                assert some[i].tobytes() == (every[i] if i in keep else sentinel).tobytes(), (keep, i)


# ---- 7. refusals and empty cases -------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone_and_empty_cases_are_ok(bn):
    rng = np.random.default_rng(239)
    n = 200
    idx = bn.Index(0, 128, n + 50)
    idx.add(ir.dyadic_rows(rng, n, 128, 64))
    Q = exact.queries(rng, 128, 64, 2)
    qi = np.array([5, 7], dtype=np.uint64)
    thr = np.zeros(2, dtype=np.float32)
    nan = np.array([0.0, np.nan], dtype=np.float32)
    sentinels = [a.tobytes() for a in fresh(2, 4)]

    def refused(msg, x, t, n_groups, g_stride, keep=range(7), first=0, n_ids=0, null_queries=False):
        for by_id in (False, True):
            queries = None if null_queries else qi if by_id else Q
            st, arrays = raw(bn, x, queries, t, n_groups, keep, by_id, 0, first, n_ids, g_stride)
            assert st == INVALID_ARG and msg in bn.last_error(), (msg, by_id, st, bn.last_error())
            assert [a.tobytes() for a in arrays] == [a.tobytes() for a in fresh(2, g_stride)], (msg, by_id)

    refused("past", idx, thr, 4, 4, first=n + 1)
    refused("past", idx, thr, 4, 4, n_ids=n + 1)
    refused("past", idx, thr, 4, 4, first=n - 1, n_ids=2)
    refused("null index", None, thr, 4, 4)
    refused("null", idx, thr, 4, 4, null_queries=True)
    refused("null", idx, None, 4, 4)
    refused("null", idx, thr, 4, 4, keep=(1, 2, 3, 4, 5, 6))
    refused("pair", idx, thr, 4, 4, keep=(0, 1))
    refused("pair", idx, thr, 4, 4, keep=(0, 2, 3))
    refused("n_groups", idx, thr, 0, 4)
    refused("n_groups", idx, thr, 65537, 65537)
    refused("g_stride", idx, thr, 4, 3)
    refused("NaN", idx, nan, 4, 4)
    refused("NaN", idx, nan, 4, 4, keep=(0,))
    st, arrays = raw(bn, idx, np.array([5, n]), thr, 4, by_id=True)
    assert st == INVALID_ARG and str(n) in bn.last_error() and [a.tobytes() for a in arrays] == sentinels

    # the legal empty cases: n_queries == 0 touches nothing; an empty range and an empty index write empty records
    assert bn.lib.bn_index_group_above(idx._h, None, 0, None, 0, 0, 4, 4, None, None, None, None, None, None, None) == 0
    assert bn.lib.bn_index_group_above_ids(idx._h, None, 0, -1, None, 0, 0, 4, 4, None, None, None, None, None, None, None) == 0
    empty_record = [np.zeros((2, 4), dtype=np.uint32), np.full((2, 4), NO_ROW, dtype=np.uint64), np.zeros((2, 4), dtype=np.float32),
                    np.full((2, 4), NO_ROW, dtype=np.uint64), np.full((2, 4), NO_ROW, dtype=np.uint64), np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)]
    gref.assert_same(idx.group_above(Q, -INF, 4, first_id=n, n_ids=0), empty_record, "an empty range at the very end")
    gref.assert_same(idx.group_above_ids(qi, -INF, 4, first_id=n), empty_record, "an empty range, ids")
    gref.assert_same(bn.Index(0, 128, 10).group_above(Q, -INF, 4), empty_record, "an empty index")
    st, arrays = raw(bn, idx, Q, thr, 3, first=n, g_stride=4)   # past n_groups the sentinels stay, also in an empty case
    assert st == 0 and arrays[0].reshape(2, 4)[:, :3].tolist() == [[0] * 3] * 2 and arrays[0].reshape(2, 4)[:, 3].tolist() == [77, 77]
    assert (arrays[1].reshape(2, 4)[:, :3] == NO_ROW).all() and (arrays[1].reshape(2, 4)[:, 3] == 0xABCDEF).all() and arrays[2].reshape(2, 4)[:, 3].tolist() == [-7.5, -7.5]
    got = idx.group_above(Q, -INF, 4, first_id=50)
    assert got[6].tolist() == [n - 50, n - 50] and got[0][:, 0].tolist() == [n - 50, n - 50] and got[3][:, 0].tolist() == [50, 50] and got[4][:, 0].tolist() == [n - 1, n - 1]


# ---- 8. determinism --------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes(bn):
    wg = workgroup_rows()
    case = above_t.ordered_case("random")
    rng = np.random.default_rng(241)
    with Tagged(case, tag_pattern("one", rng, wg)):
        first = case.idx.group_above(case.Q, -INF, 8)
        assert first[0][0, 5] == N - int(case.xbad.sum()) and first[0][0, 5] > 65536 and not first[5].any()
        again = case.idx.group_above(case.Q, -INF, 8)
        gref.assert_same(again, first, "one group, every row a hit")
        want = gref.from_scores(case.S, case.qbad, case.xbad, -INF, 8, np.full(N, 5))
        gref.assert_same(first, want, "one group, every row a hit, against the reference")
    with Tagged(case, tag_pattern("few", rng, wg)):
        a = case.idx.group_above(case.Q, -INF, 65)
        gref.assert_same(case.idx.group_above(case.Q, -INF, 65), a, "three groups, per-lane updates")
