"""bn_index_search_seq / bn_index_search_seq_ids on the GPU.  Expected results come from tests/seq_ref.seq_top_m over the score matrix
bn_index_search itself gives (test_gpu_ivf.search_matrix) or, for dyadic rows, over index_ref.scores64, which is exact for them.
Counts, ids and score bytes are compared with ==; there is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import index_ref as ir
import seq_ref
import test_gpu_index_exact as exact
from test_gpu_ivf import search_matrix
from test_gpu_subset import cut, general

pytestmark = pytest.mark.gpu
INVALID_ARG = 1
TILE = exact.TILE
N = exact.N
CAP = 28                                                     # csrc/seq_plan.h: sequences per pass at most
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def per_pass(L):
    return min(64 // L, CAP)


# ---- 1. general data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [130, 1536])
def test_general_data(bn, dim):
    """sequences cut from the general case's 70 query rows (sequence p is rows 11 + 13 p + j mod 70); row 10 is made invalid"""
    g = general(dim)
    Q, qbad = g.Q.copy(), g.qbad.copy()
    Q[10] = 0.0
    qbad[10] = True
    assert qbad.sum() == 1
    hit = set()
    for L in (1, 2, 5, 33, 64):
        n_max = max(3, per_pass(L) + 1)                      # three sequences are three passes at L = 33 and 64
        rows = np.array([[(11 + 13 * p + j) % 70 for j in range(L)] for p in range(n_max)])
        rows[-1] = [(10 - L // 2 + j) % 70 for j in range(L)]   # the last sequence of the largest call covers the invalid row
        dead = np.array([qbad[r].any() for r in rows])
        assert not dead[0] and dead[-1]
        for R in (0, 1, 64):
            want = seq_ref.seq_top_m(g.S[rows.reshape(-1)], qbad[rows.reshape(-1)], g.xbad, L, R, 256)
            assert not want[2][dead].any() and (want[2][~dead] > 0).all()
            hit.add(bool((want[2][~dead] == 256).all()))
            for n_seq in (1, 3, per_pass(L) + 1):
                for M in (1, 100, 256):
                    got = g.idx.search_seq(Q[rows[:n_seq].reshape(-1)], L, M, R)
                    exact.assert_exact(got, cut(want, n_seq, M), (dim, "L", L, "R", R, "n_seq", n_seq, "M", M))
            for p in np.flatnonzero(~dead):
                assert not np.isin(g.bad, want[0][p, :want[2][p]]).any(), "a start on an invalid row covers it"
    assert hit == {True, False}, "both branches must occur: count == M and count < M"


# ---- 2. many tiles per workgroup ------------------------------------------------------------------------------------------------------
LS = 5            # the planted run
A0 = 300          # where the run that is copied starts: more than 37 ids from every planted start


def edges(cus):
    tpw, n_wg = exact.tiles_per_workgroup(N, cus)
    wg = tpw * TILE
    assert tpw > 3 and n_wg > 3 and (n_wg - 1) * wg < N - 38 - TILE
    return wg, n_wg


@pytest.mark.parametrize("order", exact.ORDERS)
def test_planted_runs_at_tile_and_workgroup_edges(bn, order):
    """an exact copy of rows [A0, A0 + 5) planted so that it STARTS two rows before a tile edge, three workgroup edges and at the last
    possible start: every copy comes back with the score of the run itself, with and without a peak radius"""
    cus = exact.require_many_tiles()
    wg, n_wg = edges(cus)
    rng = np.random.default_rng([128, 64, 5, exact.ORDERS.index(order)])
    X = ir.rows_at_levels(rng, exact.levels(order, N, 64, rng), 128, 64)
    planted = [3 * TILE - 2] + [k * wg - 2 for k in (1, 2, n_wg - 1)] + [N - LS]
    X[A0:A0 + LS] = ir.dyadic_rows(rng, LS, 128, 64)        # a run like no other rows: rows of one extreme level are all the same row
    for s in planted:
        X[s:s + LS] = X[A0:A0 + LS]
    Q = np.concatenate([X[A0:A0 + LS], exact.queries(rng, 128, 64, LS)])     # the run itself, and a sequence of dyadic queries
    case = exact.Case(bn, X, Q)
    S = case.S.astype(np.float32)
    assert np.array_equal(S.astype(np.float64), case.S), "dyadic scores are exact in float32"
    Z, _ = seq_ref.seq_matrix(S, case.qbad, case.xbad, LS)
    run = Z[0, A0]
    assert run == np.float32(LS) * (np.float32(1) / np.float32(LS)) and (Z[0, planted] == run).all()
    assert (np.delete(Z[0], [A0] + planted) < run).all(), "no other start reaches the planted score"
    for R in (0, 37):
        want = seq_ref.seq_top_m(S, case.qbad, case.xbad, LS, R, 256)
        for n_seq in (1, 2):
            for M in (1, 100, 256):
                exact.assert_exact(case.idx.search_seq(Q[:n_seq * LS], LS, M, R), cut(want, n_seq, M), (order, "R", R, "n_seq", n_seq, "M", M))
        ids, sc, cnt = case.idx.search_seq(Q[:LS], LS, 256, R)
        assert ids[0, :6].tolist() == sorted([A0] + planted) and sc[0, :6].tobytes() == run.tobytes() * 6 and sc[0, 6] < run, (order, R)
        # the same run as stored rows, itself excluded
        ids, sc, cnt = case.idx.search_seq_ids([A0], LS, 0, 256, R)
        assert ids[0, :5].tolist() == sorted(planted) and sc[0, :5].tobytes() == run.tobytes() * 5 and sc[0, 5] < run, (order, R, "ids")


def test_equal_best_starts_across_workgroup_and_tile_edges(bn):
    """six rows at the top level make the two starts on either side of an edge score the same: with a radius exactly the lower id survives"""
    cus = exact.require_many_tiles()
    wg, n_wg = edges(cus)
    rng = np.random.default_rng(59)
    lv = rng.integers(-64, 56, N)                           # everything else lies below the planted level
    pairs = [(3 * TILE - 1, 3 * TILE)] + [(k * wg - 1, k * wg) for k in (1, 2, n_wg - 1)] + [(N - LS - 1, N - LS)]
    for a, _ in pairs:
        lv[a:a + LS + 1] = 64
    Q = np.concatenate([np.repeat(ir.canonical_query(128, 64)[None], LS, axis=0), exact.queries(rng, 128, 64, LS)])
    case = exact.Case(bn, ir.rows_at_levels(rng, lv, 128, 64), Q)
    S = case.S.astype(np.float32)
    lower, higher = [a for a, _ in pairs], [b for _, b in pairs]
    for R in (0, 1, 37):
        want = seq_ref.seq_top_m(S, case.qbad, case.xbad, LS, R, 256)
        for M in (1, 256):
            exact.assert_exact(case.idx.search_seq(Q, LS, M, R), cut(want, 2, M), ("edges", "R", R, "M", M))
        ids, sc, cnt = case.idx.search_seq(Q[:LS], LS, 256, R)
        got = ids[0, :cnt[0]]
        if R == 0:
            assert ids[0, :10].tolist() == sorted(lower + higher) and (sc[0, :10] == sc[0, 0]).all() and sc[0, 10] < sc[0, 0]
        else:
            assert ids[0, :5].tolist() == lower and (sc[0, :5] == sc[0, 0]).all() and sc[0, 5] < sc[0, 0], R
            assert not np.isin(higher, got).any(), "the higher id of a tied pair was returned"


# ---- 3. small sizes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 300])
def test_small_sizes_and_invalid_rows_inside_the_best_run(bn, n):
    rng = np.random.default_rng(61 + n)
    for L in sorted({1, 2, 64} | ({n} if n <= 64 else set())):
        X = ir.rows_at_levels(rng, rng.integers(-32, 33, n), 128, 64)   # away from the extreme levels, whose rows are all the same row
        b = max(0, (n - L) // 2)                             # the best run starts here: the first sequence is a copy of it
        first = X[b:b + L] if n >= L else ir.dyadic_rows(rng, L, 128, 64)
        Q = np.concatenate([first, exact.queries(rng, 128, 64, L)])
        case = exact.Case(bn, X, Q, capacity=n + 70)
        S = case.S.astype(np.float32)
        for R in (0, 1, 2, 64):
            want = seq_ref.seq_top_m(S, case.qbad, case.xbad, L, R, 256)
            for M in (1, 256):
                exact.assert_exact(case.idx.search_seq(Q, L, M, R), cut(want, 2, M), (n, "L", L, "R", R, "M", M))
            if n < L:
                assert not want[2].any(), "an index shorter than the sequence has no start"
            if n == L:
                assert want[2].tolist() == [1, 1] and not want[0][:, 0].any(), "one start, row 0"
        if n < L:
            continue
        assert case.idx.search_seq(Q[:L], L, 1)[0][0, 0] == b
        # the same rows with one row inside the best run invalid: exactly the L starts that cover it are gone
        v = b + L // 2
        X2 = X.copy()
        X2[v] = 0.0
        bad = exact.Case(bn, X2, Q, capacity=n + 70)
        assert np.flatnonzero(bad.xbad).tolist() == [v]
        S2 = bad.S.astype(np.float32)
        covered = set(range(max(0, v - L + 1), v + 1))
        for R in (0, 2):
            want = seq_ref.seq_top_m(S2, bad.qbad, bad.xbad, L, R, 256)
            got = bad.idx.search_seq(Q, L, 256, R)
            exact.assert_exact(got, want, (n, "L", L, "R", R, "invalid row", v))
            assert not covered & set(got[0][0, :got[2][0]].tolist())
        ids, _, cnt = bad.idx.search_seq(Q[:L], L, 256, 0)
        if n - L + 1 <= 256:
            assert set(ids[0, :cnt[0]].tolist()) == set(range(n - L + 1)) - covered, "every other start is still there"
        # every row the same row: all starts tie, so with a radius the peaks are start 0 and the first start after the gap
        row = ir.canonical_query(128, 64)
        T = np.repeat(row[None], n, axis=0)
        T[v] = 0.0
        tied = exact.Case(bn, T, np.repeat(row[None], L, axis=0), capacity=n + 70)
        R = min(L, 2)
        got = tied.idx.search_seq(tied.Q, L, 256, R)
        exact.assert_exact(got, seq_ref.seq_top_m(tied.S.astype(np.float32), tied.qbad, tied.xbad, L, R, 256), (n, "L", L, "tied"))
        starts = [s for s in (0, v + 1) if s not in covered and s + L <= n]
        assert got[0][0, :got[2][0]].tolist() == starts, "the removed starts suppress nobody: the first start after them is a peak"


# ---- 4. the _ids form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 5, 64])
def test_search_seq_ids_general_data(bn, L):
    g = general(130)
    first = np.array([0, 2500 - L // 2, 4000, g.n - L], dtype=np.int64)      # the second covers the invalid row 2500
    rows = (first[:, None] + np.arange(L)[None]).reshape(-1)
    S = search_matrix(bn, g.X, g.X[rows])
    qbad = g.xbad[rows]
    assert qbad.sum() == 1
    for ex in (-1, 0, L - 1):
        for R in (0, 2):
            want = seq_ref.seq_top_m(S, qbad, g.xbad, L, R, 256, first, ex)
            assert want[2][1] == 0 and (want[2][[0, 2, 3]] == 256).all()
            for n_seq in (1, 4):
                for M in (1, 100, 256):
                    got = g.idx.search_seq_ids(first[:n_seq], L, ex, M, R)
                    exact.assert_exact(got, cut(want, n_seq, M), ("L", L, "exclude", ex, "R", R, "n_seq", n_seq, "M", M))
            got = g.idx.search_seq_ids(first, L, ex, 256, R)
            for p in (0, 2, 3):
                r = got[0][p].astype(np.int64)
                assert ex < 0 or not (np.abs(r - first[p]) <= ex).any(), (ex, p)
                if ex < 0:
                    assert r[0] == first[p], "the run itself is its best match"


def test_excluded_starts_do_not_suppress_their_neighbours_and_bad_arguments_are_refused(bn):
    n, L = 200, 3
    row = ir.canonical_query(128, 64)
    idx = bn.Index(0, 128, n)
    idx.add(np.repeat(row[None], n, axis=0))                # every start scores the same
    one = np.float32(3) * (np.float32(1) / np.float32(3))
    ids, sc, cnt = idx.search_seq_ids([100, 0, 197, 64], L, 3, 256, 2)
    assert [ids[q, :cnt[q]].tolist() for q in range(4)] == [[0, 104], [4], [0], [0, 68]] and (sc[cnt[:, None] > np.arange(256)[None]] == one).all()
    ids, sc, cnt = idx.search_seq_ids([100, 0], L, 0, 256, 1)
    assert [ids[q, :cnt[q]].tolist() for q in range(2)] == [[0, 101], [1]]
    ids, sc, cnt = idx.search_seq_ids([100], L, 3, 256, 8)
    assert ids[0, :cnt[0]].tolist() == [0], "start 96 is within 8 of start 104"
    ids, sc, cnt = idx.search_seq_ids([100], L, -1, 256, 0)
    assert cnt[0] == n - L + 1 and ids[0, :cnt[0]].tolist() == list(range(n - L + 1)), "starts past size - L do not exist"
    # refusals: nothing written
    oi, os_, oc = np.full(8, 0xABCDEF, dtype=np.uint64), np.full(8, -7.5, dtype=np.float32), np.full(2, 77, dtype=np.uint32)
    before = (oi.tobytes(), os_.tobytes(), oc.tobytes())
    outs = (oi.ctypes.data_as(u64p), os_.ctypes.data_as(f32p), oc.ctypes.data_as(u32p))
    q = np.ones(2 * L * 128, dtype=np.float32)
    qp = q.ctypes.data_as(f32p)

    def refused(st, word):
        return st == INVALID_ARG and word in bn.last_error() and (oi.tobytes(), os_.tobytes(), oc.tobytes()) == before

    for R in (0, 2):
        qi = np.array([5, n - L + 1], dtype=np.uint64)
        assert refused(bn.lib.bn_index_search_seq_ids(idx._h, qi.ctypes.data_as(u64p), 2, L, -1, R, 4, 4, *outs), str(n))
        qi = np.array([n - L, 5], dtype=np.uint64)
        assert bn.lib.bn_index_search_seq_ids(idx._h, qi.ctypes.data_as(u64p), 2, L, -1, R, 4, 4, *outs) == 0, "first_id + seq_len == size is legal"
        oi[:], os_[:], oc[:] = 0xABCDEF, -7.5, 77
        qi = np.array([5, 1 << 63], dtype=np.uint64)
        assert refused(bn.lib.bn_index_search_seq_ids(idx._h, qi.ctypes.data_as(u64p), 2, L, -1, R, 4, 4, *outs), "past")
        assert refused(bn.lib.bn_index_search_seq_ids(None, qi.ctypes.data_as(u64p), 2, L, -1, R, 4, 4, *outs), "null index")
        assert refused(bn.lib.bn_index_search_seq(None, qp, 2, L, R, 4, 4, *outs), "null index")
        for sl in (0, 65):
            assert refused(bn.lib.bn_index_search_seq(idx._h, qp, 2, sl, R, 4, 4, *outs), "seq_len")
            assert refused(bn.lib.bn_index_search_seq_ids(idx._h, qi.ctypes.data_as(u64p), 2, sl, -1, R, 4, 4, *outs), "seq_len")
        assert refused(bn.lib.bn_index_search_seq(idx._h, qp, 2, L, R, 0, 4, *outs), "top_m")
        assert refused(bn.lib.bn_index_search_seq(idx._h, qp, 2, L, R, 257, 300, *outs), "top_m")
        assert refused(bn.lib.bn_index_search_seq(idx._h, qp, 2, L, R, 4, 3, *outs), "m_stride")
        assert refused(bn.lib.bn_index_search_seq(idx._h, None, 2, L, R, 4, 4, *outs), "null")
        assert refused(bn.lib.bn_index_search_seq_ids(idx._h, None, 2, L, -1, R, 4, 4, *outs), "null")
        for null in range(3):
            a = list(outs)
            a[null] = None
            assert refused(bn.lib.bn_index_search_seq(idx._h, qp, 2, L, R, 4, 4, *a), "null")
    assert refused(bn.lib.bn_index_search_seq(idx._h, qp, 2, L, 65, 4, 4, *outs), "peak_radius")
    # an empty index: count 0 for host sequences
    empty = bn.Index(0, 128, 10)
    ids, sc, cnt = empty.search_seq(q.reshape(-1, 128), L, 4, 2)
    assert cnt.tolist() == [0, 0] and np.isnan(sc).all()


# ---- 5. identities ----------------------------------------------------------------------------------------------------------------------
def test_length_one_is_the_peaks_search_and_calls_are_independent(bn):
    g = general(130)
    qi = [0, 1, 63, 64, 65, g.n - 1, 100, 2500, 777, 4097]
    for R in (0, 2):
        for a, b in zip(g.idx.search_seq(g.Q, 1, 100, R), g.idx.search_peaks(g.Q, 100, R)):
            assert a.tobytes() == b.tobytes(), R
        for ex in (-1, 3):
            for a, b in zip(g.idx.search_seq_ids(qi, 1, ex, 100, R), g.idx.search_peaks_ids(qi, 100, R, exclude_radius=ex)):
                assert a.tobytes() == b.tobytes(), (R, ex)
    for a, b in zip(g.idx.search_seq(g.Q, 1, 256), g.idx.search(g.Q, 256)):
        assert a.tobytes() == b.tobytes()
    # one call with n sequences is n calls with one; a second identical call returns the same bytes
    for L, n_seq in ((5, 14), (2, 33)):
        Q = g.Q[np.arange(n_seq * L) % 70]
        for R in (0, 8):
            whole = g.idx.search_seq(Q, L, 100, R)
            again = g.idx.search_seq(Q, L, 100, R)
            assert [a.tobytes() for a in whole] == [a.tobytes() for a in again]
            for p in range(n_seq):
                single = g.idx.search_seq(Q[p * L:(p + 1) * L], L, 100, R)
                for a, b in zip(single, whole):
                    assert a.tobytes() == b[p:p + 1].tobytes(), (L, R, p)


# ---- 6. nothing else moved ------------------------------------------------------------------------------------------------------------
def test_other_searches_appends_and_ivf_extend_are_unchanged(bn):
    rng = np.random.default_rng(83)
    X = rng.standard_normal((700, 130)).astype(np.float32)
    Q = rng.standard_normal((20, 130)).astype(np.float32)
    cent = X[rng.integers(0, 500, 8)]

    def build(with_seq):
        idx = bn.Index(0, 130, 700)
        idx.add(X[:500])
        idx.fill_tags(100, 200, 3)
        ivf = bn.Ivf(idx, cent)
        sub = bn.Subset.select(idx, tags=[3])
        out = []
        for step in range(2):
            if with_seq:
                idx.search_seq(Q, 5, 100, 8)
                idx.search_seq_ids([0, 200], 10, 0, 256)
            out += [a.tobytes() for a in idx.search(Q, 100)] + [a.tobytes() for a in sub.search(Q, 50)]
            out += [a.tobytes() for a in ivf.search(Q, 3, 50)]
            if step == 0:
                assert idx.add(X[500:]) == 500              # an append after sequence searches, then the view catches up
                if with_seq:
                    idx.search_seq(Q, 4, 10)
                ivf.extend()
                assert ivf.rows == 700
        out += [idx.read().tobytes(), idx.tags().tobytes(), ivf.list_sizes().tobytes()]
        return out

    assert build(True) == build(False)
