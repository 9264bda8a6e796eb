"""The index scan and merge (csrc/index.hip) compared EXACTLY -- counts, ids and score bytes with == -- at many 64-row tiles per
workgroup, where index_scan_kernel merges its pending lists inside the tile loop, compares rows with a threshold an earlier
tile set and carries its lists across tile boundaries.

The rows are dyadic (tests/index_ref.py): their f32 cosine has no rounding in any summation order, nearly all of them tie, and
the expected top-M is a float64 sort with ties by id.  The row orders present the pending lists and index_merge_kernel with
their adversarial cases.  Two further tests use general data: the bit pattern of a (query, row) score may not depend on where
the row sits or on how large the index is, and index_normalise_kernel commutes exactly with a power-of-two scale."""
import numpy as np
import pytest

import index_ref as ir

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

pytestmark = pytest.mark.gpu

TILE = 64
N = 8 * TILE * 320 + 37          # 163 877 rows: >= 8 tiles per workgroup on any device of <= 320 CUs, and a ragged last tile
MS = (1, 63, 64, 65, 255, 256)
QS = (1, 17, 40, 64, 70)         # query blocks of 1, 2, 3, 4 x 16, and a second pass of 64
NQ = max(QS)
ORDERS = ("rising", "falling", "tile_rising", "sawtooth", "constant", "random")


def cu_count():
    if torch is None or not torch.cuda.is_available():
        return None
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def tiles_per_workgroup(n, cus):
    """run_search's split: (tiles per workgroup, workgroups)"""
    tiles = (n + TILE - 1) // TILE
    tpw = (tiles + cus - 1) // cus
    return tpw, (tiles + tpw - 1) // tpw


def require_many_tiles(n=N):
    """A card with more CUs must fail loudly, not turn these back into one-tile-per-workgroup tests.  Returns the CU count.
    Where torch cannot tell it, 256 is assumed and nothing is asserted: the expected results do not depend on it, only the
    choice of the ids meant to sit at workgroup edges does, and those ids are then merely ordinary ones."""
    cus = cu_count()
    if cus is None:
        return 256
    assert n > 4 * TILE * cus, "%d rows give a %d-CU device fewer than 4 tiles per workgroup: raise N" % (n, cus)
    return cus


def levels(order, n, nnz, rng):
    """level of query 0 (the canonical query) as a function of the row id"""
    L, i = 2 * nnz + 1, np.arange(n, dtype=np.int64)       # L is odd
    k = {"rising": lambda: i * L // n,
         "falling": lambda: L - 1 - i * L // n,
         "tile_rising": lambda: (i // TILE) % L,
         "sawtooth": lambda: i % L,
         "constant": lambda: np.full(n, nnz + 3),
         "random": lambda: rng.integers(0, L, n)}[order]()
    return k - nnz


def queries(rng, dim, nnz, nq=NQ):
    """query 0 is the canonical one, the others random dyadic queries (their scores against the same rows simply tie heavily)"""
    return np.concatenate([ir.canonical_query(dim, nnz)[None], ir.dyadic_rows(rng, nq - 1, dim, nnz)])


def assert_exact(got, want, what):
    (gi, gs, gc), (wi, ws, wc) = got, want
    assert gi.shape == wi.shape and gs.shape == ws.shape and gc.shape == wc.shape, what
    assert np.array_equal(gc, wc), (what, "counts", np.flatnonzero(gc != wc)[:8], gc[gc != wc][:8], wc[gc != wc][:8])
    if not np.array_equal(gi, wi):
        q, j = np.argwhere(gi != wi)[0]
        raise AssertionError((what, "ids: query %d rank %d" % (q, j), gi[q, max(0, j - 2):j + 3], wi[q, max(0, j - 2):j + 3]))
    if gs.tobytes() != ws.tobytes():
        q, j = np.argwhere(gs.view(np.uint32) != ws.view(np.uint32))[0]
        raise AssertionError((what, "score bits: query %d rank %d" % (q, j), gs[q, j], ws[q, j]))


class Case:
    """an index over X and the float64 product that every expected result of it is cut from"""

    def __init__(self, bn, X, Q, capacity=None):
        self.X, self.Q = X, Q
        self.idx = bn.Index(0, X.shape[1], capacity or len(X))
        assert self.idx.add(X) == 0 and len(self.idx) == len(X)
        self.S, self.qbad, self.xbad = ir.scores64(Q, X)
        self._top = {}

    def want(self, M, nq):
        """expected search(Q[:nq], M): the first M of the top 256 (no exclusion)"""
        if 256 not in self._top:
            self._top[256] = ir.top_m_from_scores(self.S, self.qbad, self.xbad, 256)
        ids, sc, cnt = self._top[256]
        return ids[:nq, :M], sc[:nq, :M], np.minimum(cnt[:nq], M).astype(np.uint32)

    def check_grid(self, what, ms=MS, qs=QS):
        for nq in qs:
            for M in ms:
                assert_exact(self.idx.search(self.Q[:nq], M), self.want(M, nq), (what, "Q", nq, "M", M))

    def check_stored(self, nnz):
        want = ir.stored(self.X, nnz)
        want[self.xbad] = 0
        assert self.idx.read().tobytes() == want.tobytes(), "stored rows are not the +-2^-j rows"


def ordered_case(bn, order, dim, nnz, n=N):
    rng = np.random.default_rng([dim, nnz, ORDERS.index(order)])
    lv = levels(order, n, nnz, rng)
    case = Case(bn, ir.rows_at_levels(rng, lv, dim, nnz), queries(rng, dim, nnz))
    case.levels = lv
    return case


@pytest.mark.parametrize("order", ORDERS)
def test_row_orders_dim_128(bn, order):
    require_many_tiles()
    case = ordered_case(bn, order, 128, 64)
    case.check_stored(64)
    case.check_grid(order)
    # query 0 by construction: the best level's rows in id order
    lv = case.levels
    ids, scores, _ = case.idx.search(case.Q[:1], 256)
    top = np.flatnonzero(lv == lv.max())
    if len(top) >= 256:
        assert np.array_equal(ids[0], top[:256]) and np.all(scores[0] == np.float32(lv.max() / 64))
    if order == "constant":
        assert np.array_equal(ids[0], np.arange(256))


@pytest.mark.parametrize("order", ["rising", "tile_rising", "random"])
@pytest.mark.parametrize("dim,nnz", [(200, 64), (300, 256)])
def test_row_orders_with_a_k_tail(bn, order, dim, nnz):
    """two and three k chunks per tile, the last one zero-padded"""
    require_many_tiles()
    case = ordered_case(bn, order, dim, nnz)
    case.check_stored(nnz)
    case.check_grid((order, dim, nnz))


@pytest.mark.parametrize("dim,nnz", [(1, 1), (5, 4)])
def test_tiny_dims(bn, dim, nnz):
    rng = np.random.default_rng(dim)
    n = 1000
    lv = np.array([-1, 1])[rng.integers(0, 2, n)] if dim == 1 else rng.integers(-nnz, nnz + 1, n)
    case = Case(bn, ir.rows_at_levels(rng, lv, dim, nnz), queries(rng, dim, nnz))
    case.check_stored(nnz)
    case.check_grid((dim, nnz))


def sprinkle_invalid(X, tpw):
    """zero, NaN and +-inf rows through X: whole tiles (the first of a workgroup among them), first and last rows of tiles, the
    first and last row of the slab.  Returns their ids."""
    n = len(X)
    wg = tpw * TILE
    whole = [np.arange(t * TILE, (t + 1) * TILE) for t in (0, 5, 6, tpw, 3 * tpw - 1, (n - 1) // TILE - 1)]
    edges = np.array([7 * TILE, 8 * TILE - 1, 8 * TILE, 2 * wg - 1, 2 * wg, 5 * wg - 1, 5 * wg + 63, 5 * wg + 64, n - 38, n - 37, n - 1, 1000, 1001, 77777])
    bad = np.unique(np.concatenate(whole + [edges]))
    for j, i in enumerate(bad):
        kind = j % 4
        if kind == 0:
            X[i] = 0
        else:
            X[i, (7 * j) % X.shape[1]] = (np.nan, np.inf, -np.inf)[kind - 1]
    return bad


def test_invalid_rows_are_counted_stored_as_zeros_and_never_returned(bn):
    cus = require_many_tiles()
    tpw, _ = tiles_per_workgroup(N, cus)
    rng = np.random.default_rng(41)
    lv = levels("rising", N, 64, rng)
    X = ir.rows_at_levels(rng, lv, 128, 64)
    first_best = int(np.flatnonzero(lv == 64)[0])
    bad = sprinkle_invalid(X, tpw)
    # and the rows that would win: the first 100 of the best level, then every second one of the next 200
    more = np.concatenate([np.arange(first_best, first_best + 100), np.arange(first_best + 100, first_best + 300, 2)])
    X[more[::2]] = 0
    X[more[1::2], 5] = np.nan
    bad = np.union1d(bad, more)
    Q = queries(rng, 128, 64)
    Q[3] = 0                    # invalid queries: count 0
    Q[20, 9] = np.inf
    case = Case(bn, X, Q)
    assert len(case.idx) == N and np.array_equal(np.flatnonzero(case.xbad), bad) and list(np.flatnonzero(case.qbad)) == [3, 20]
    case.check_stored(64)
    assert not case.idx.read()[bad].any()
    case.check_grid("invalid rows")
    ids, _, counts = case.idx.search(Q, 256)
    assert counts[3] == 0 and counts[20] == 0 and not np.isin(ids[counts > 0], bad).any()


def radius_mask(qids, radius, n):
    d = np.arange(n, dtype=np.int64)[None, :] - np.asarray(qids, dtype=np.int64)[:, None]
    return np.abs(d) <= radius


@pytest.mark.parametrize("order", ["constant", "rising"])
def test_search_ids_with_exclusion(bn, order):
    """the queries are stored rows, so the rows a radius excludes are exactly the ones that would win: the row itself and, where
    neighbours are identical (constant: every row is the canonical one; rising: the best level's rows are), its neighbours"""
    cus = require_many_tiles()
    tpw, n_wg = tiles_per_workgroup(N, cus)
    wg = tpw * TILE
    rng = np.random.default_rng(43)
    lv = np.full(N, 64) if order == "constant" else levels("rising", N, 64, rng)
    X = ir.rows_at_levels(rng, lv, 128, 64)
    invalid = [5 * TILE, 1000, wg + 1]
    X[invalid[0]] = 0
    X[invalid[1], 3] = np.nan
    X[invalid[2], 100] = -np.inf
    g0 = int(np.flatnonzero(lv == 64)[0])   # first row of the best level
    qids = [0, 1, 63, 64, 65, 100, wg - 1, wg, 2 * wg - 1, 2 * wg, (n_wg - 1) * wg - 1, (n_wg - 1) * wg, N - 38, N - 37, N - 1,
            g0, g0 + 1, g0 + 100, 64, 0, N - 1] + invalid
    assert max(qids) < N
    case = Case(bn, X, X[qids])
    assert list(np.flatnonzero(case.qbad)) == [len(qids) - 3, len(qids) - 2, len(qids) - 1]
    for radius in (-1, 0, 1, 100, N, 1 << 40):
        ex = None if radius < 0 else radius_mask(qids, radius, N)
        ids, sc, cnt = ir.top_m_from_scores(case.S, case.qbad, case.xbad, 256, ex)
        for M in (1, 64, 256):
            got = case.idx.search_ids(qids, M, exclude_radius=radius)
            assert_exact(got, (ids[:, :M], sc[:, :M], np.minimum(cnt, M)), (order, "radius", radius, "M", M))
            if radius >= N:
                assert not got[2].any()
    got = case.idx.search_ids(qids, 256, exclude_radius=100)
    assert not got[2][-3:].any(), "the id of an invalid row must give count 0"
    if order == "constant":
        assert np.array_equal(got[0][0], np.setdiff1d(np.arange(101, 360), invalid)[:256])


def test_growth_between_searches(bn):
    """search, append a ragged block (a partial tile fills, the tiles per workgroup change), search again: three times"""
    cus = require_many_tiles()
    sizes = [100_037, 132_027, 152_040, N]
    assert len({tiles_per_workgroup(n, cus)[0] for n in sizes}) == len(sizes), "the appends no longer change the tiles per workgroup"
    rng = np.random.default_rng(47)
    X = ir.rows_at_levels(rng, levels("random", N, 64, rng), 128, 64)
    Q = queries(rng, 128, 64)
    S, qbad, xbad = ir.scores64(Q, X)
    idx = bn.Index(0, 128, N)
    prev, prev_n = None, 0
    for n in sizes:
        assert idx.add(X[prev_n:n]) == prev_n and len(idx) == n
        want = ir.top_m_from_scores(S[:, :n], qbad, xbad[:n], 256)
        got = idx.search(Q, 256)
        assert_exact(got, want, ("grown to", n))
        assert_exact(idx.search(Q[:17], 65), (want[0][:17, :65], want[1][:17, :65], np.minimum(want[2][:17], 65)), ("grown to", n, "M 65"))
        if prev is not None:
            for q in range(NQ):
                old = got[0][q] < prev_n
                k = int(old.sum())
                assert np.array_equal(got[0][q][old], prev[0][q, :k]) and got[1][q][old].tobytes() == prev[1][q, :k].tobytes(), (n, q)
        prev, prev_n = got, n
    assert idx.read().tobytes() == ir.stored(X, 64).tobytes()


def test_host_plumbing_rounds_and_stride(bn):
    """1030 queries are two rounds of the host loop; with m_stride = top_m + 3 rows sit at the stride and the three trailing
    slots keep the binding's sentinels (id 0, score NaN)"""
    rng = np.random.default_rng(53)
    n, nq, M = 1000, 1030, 10
    X = ir.dyadic_rows(rng, n, 128, 64)
    Q = queries(rng, 128, 64, nq)
    Q[1025] = 0                                   # count 0: the whole row keeps its sentinels
    case = Case(bn, X, Q)
    ids, sc, cnt = ir.top_m_from_scores(case.S, case.qbad, case.xbad, M)
    wi, ws = np.zeros((nq, M + 3), dtype=np.uint64), np.full((nq, M + 3), np.nan, dtype=np.float32)
    wi[:, :M], ws[:, :M] = ids, sc
    assert_exact(case.idx.search(Q, M, m_stride=M + 3), (wi, ws, cnt), "search, stride")
    assert_exact(case.idx.search(Q, M), (ids, sc, cnt), "search")
    qids = rng.integers(0, n, nq)
    S, qbad, xbad = ir.scores64(X[qids], X)
    ex = radius_mask(qids, 2, n)
    ids, sc, cnt = ir.top_m_from_scores(S, qbad, xbad, M, ex)
    wi[:, :M], ws[:, :M] = ids, sc
    assert_exact(case.idx.search_ids(qids, M, exclude_radius=2, m_stride=M + 3), (wi, ws, cnt), "search_ids, stride")


def gaussian_chunks(rng, n, dim, chunk=8192):
    """n Gaussian rows in chunks, cheaply: one Gaussian block, rotated along k by the chunk number (each row stays Gaussian)"""
    block = rng.standard_normal((chunk, dim), dtype=np.float32)
    for c, a in enumerate(range(0, n, chunk)):
        yield a, np.roll(block, c, axis=1)[:min(chunk, n - a)].copy()


@pytest.mark.parametrize("dim", [37, 1536])
def test_score_bits_do_not_depend_on_row_position_or_index_size(bn, dim):
    """general data: 256 copies of one Gaussian row planted among N Gaussian rows -- every residue mod 64, both ends of
    workgroups' ranges, the ragged last tile -- come back as exactly those ids in ascending order with ONE score bit pattern, the
    one the row gives when stored alone, in a 100-row index, with Q = 1 and as query 63 of 64"""
    cus = require_many_tiles()
    tpw, n_wg = tiles_per_workgroup(N, cus)
    wg = tpw * TILE
    rng = np.random.default_rng(dim)
    r = rng.standard_normal(dim, dtype=np.float32)
    qv = (r + 0.1 * rng.standard_normal(dim, dtype=np.float32)).astype(np.float32)
    special = [g * wg for g in (0, 1, 2, n_wg // 2, n_wg - 1)] + [(g + 1) * wg - 1 for g in (0, 1, n_wg // 2, n_wg - 2)] + [N - 37, N - 19, N - 1]
    planted = set(special)
    for res in range(TILE):                        # every residue mod 64, in tiles spread over the slab
        if not any(p % TILE == res for p in planted):
            planted.add(int(rng.integers(0, N // TILE)) * TILE + res)
    while len(planted) < 256:
        planted.add(int(rng.integers(0, N)))
    planted = np.array(sorted(planted))
    assert len(planted) == 256 and planted.max() < N and len(set((planted % TILE).tolist())) == TILE
    idx = bn.Index(0, dim, N)
    for a, X in gaussian_chunks(rng, N, dim):
        mine = planted[(planted >= a) & (planted < a + len(X))] - a
        X[mine] = r
        assert idx.add(X) == a
    assert len(idx) == N
    ids, scores, counts = idx.search(qv[None], 256)
    assert counts[0] == 256 and np.array_equal(ids[0], planted), "the top 256 are not the planted ids in ascending order"
    bits = scores[0, :1].tobytes()
    assert scores[0].tobytes() == bits * 256, ("one row, several score bit patterns", np.unique(scores[0]))
    Q64 = rng.standard_normal((64, dim), dtype=np.float32)
    Q64[63] = qv
    ids, scores, counts = idx.search(Q64, 256)
    assert counts[63] == 256 and np.array_equal(ids[63], planted) and scores[63].tobytes() == bits * 256
    alone = bn.Index(0, dim, 1)
    alone.add(r[None])
    ids, scores, counts = alone.search(qv[None], 1)
    assert counts[0] == 1 and ids[0, 0] == 0 and scores[0].tobytes() == bits, (scores[0], np.frombuffer(bits, np.float32))
    hundred = bn.Index(0, dim, 100)
    X = rng.standard_normal((100, dim), dtype=np.float32)
    X[57] = r
    hundred.add(X)
    for Q in (qv[None], Q64):
        ids, scores, counts = hundred.search(Q, 1)
        assert ids[-1, 0] == 57 and scores[-1].tobytes() == bits, (scores[-1], np.frombuffer(bits, np.float32))


@pytest.mark.parametrize("dim", [37, 1536])
def test_normalisation_commutes_with_a_power_of_two_scale(bn, dim):
    """x -> 2^e x scales every fmaf of the sum of squares by 2^2e, its square root by 2^e and leaves x / norm alone, exactly, as
    long as nothing overflows or goes subnormal.  When the sum overflows, or every square underflows to zero, the row is invalid."""
    rng = np.random.default_rng(dim + 1)
    n = 2 * TILE + 2
    X = rng.standard_normal((n, dim), dtype=np.float32)
    X = (np.where(X < 0, -1, 1) * np.clip(np.abs(X), 2.0 ** -10, 8.0)).astype(np.float32)
    Q = rng.standard_normal((5, dim), dtype=np.float32)
    base = bn.Index(0, dim, n)
    base.add(X)
    stored, result = base.read(), base.search(Q, n)
    X64 = X.astype(np.float64)
    assert np.all(result[2] == n) and np.abs(stored - X64 / np.sqrt((X64 * X64).sum(axis=1, keepdims=True))).max() <= 1e-6
    for e in (-40, -13, -1, 1, 20, 40):
        scaled = bn.Index(0, dim, n)
        scaled.add(np.ldexp(X, e))
        assert scaled.read().tobytes() == stored.tobytes(), e
        for a, b in zip(scaled.search(Q, n), result):
            assert a.tobytes() == b.tobytes(), e
    # invalid at both ends, stored as zeros, never returned -- also from an index that holds valid rows
    mixed = bn.Index(0, dim, 3 * n)
    mixed.add(np.concatenate([np.ldexp(X, 64), X, np.ldexp(X, -80)]))
    assert len(mixed) == 3 * n
    got = mixed.read()
    assert not got[:n].any() and not got[2 * n:].any() and got[n:2 * n].tobytes() == stored.tobytes()
    ids, scores, counts = mixed.search(Q, 256)
    assert np.all(counts == n)
    assert np.array_equal(ids[:, :n], result[0] + np.uint64(n)) and scores[:, :n].tobytes() == result[1].tobytes()
    for e in (64, -80):
        dead = bn.Index(0, dim, n)
        dead.add(np.ldexp(X, e))
        assert len(dead) == n and not dead.read().any() and not dead.search(Q, 4)[2].any(), e
        assert not dead.search_ids([0, n - 1], 4)[2].any(), e


def test_the_four_scan_routes_give_a_vector_and_row_the_same_score_bits(bn):
    """index_scan_kernel, subset_scan_kernel, peaks_scan_kernel and rank_scan_kernel each write out the same tile loop over one LDS
    layout (csrc/index_scan.h): for the same (vector, row) each must give the bits bn_index_search gives.  General data, dim 130 (two k chunks, the second with a k
    tail), many tiles per workgroup and a ragged last tile, 17 queries (two query blocks), M = 256.  No tolerance anywhere."""
    require_many_tiles()
    dim, nq, M = 130, 17, 256
    rng = np.random.default_rng(130)
    idx = bn.Index(0, dim, N)
    for a, X in gaussian_chunks(rng, N, dim):
        assert idx.add(X) == a
    Q = rng.standard_normal((nq, dim), dtype=np.float32)
    want = idx.search(Q, M)
    assert np.all(want[2] == M)

    everything = bn.Subset.select(idx)
    assert len(everything) == N
    assert_exact(everything.search(Q, M), want, "a subset over all rows")

    # the peaks are some of the rows, in the search's order: a search over exactly those rows returns the same lists
    ids, scores, counts = idx.search_peaks(Q, M, 1)
    assert counts.min() > 0
    for q in range(nq):
        k = int(counts[q])
        only = bn.Subset.from_ids(idx, np.sort(ids[q, :k]))
        si, ss, sc = only.search(Q[q:q + 1], M)
        assert sc[0] == k and np.array_equal(si[0, :k], ids[q, :k]) and ss[0, :k].tobytes() == scores[q, :k].tobytes(), ("peaks", q)
        both = np.isin(ids[q, :k], want[0][q])            # and where a peak is among the search's own top M, directly
        at = np.array([np.flatnonzero(want[0][q] == i)[0] for i in ids[q, :k][both]], dtype=np.int64)
        assert both.any() and scores[q, :k][both].tobytes() == want[1][q][at].tobytes(), ("peaks in the top M", q)

    # the head's weight rows are the query rows as the search stores them (normalised by the same kernel), its bias is zero
    stored = bn.Index(0, dim, nq)
    stored.add(Q)
    head = bn.Head(0, stored.read(), np.zeros(nq, dtype=np.float32), l2norm=True)
    ri, rl, rc = head.rank_index(idx, M)
    assert np.array_equal(rc, want[2]) and np.array_equal(ri, want[0])
    assert np.array_equal(rl, want[1]), "logits differ from the scores"      # ==: a logit is score + 0.0, so -0.0 may come back +0.0
