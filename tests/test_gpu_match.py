"""bn_index_match on the GPU (csrc/match.hip): the kernels a step runs against an attached index, on host rows.

Bit identity with bn_index_search (counts, ids and score bytes ==), the threshold against float64 on rows whose f32 cosine is exact,
the selection with overflowing pending lists at >= 8 tiles per workgroup, tags, and the independence of a score's bits from the
query's position, the batch and the number of rows searched."""
import numpy as np
import pytest

import index_ref as ir
import match_ref

pytestmark = pytest.mark.gpu

TILE = 64


def match_ranges(n_rows):
    """match.hip's split rule (bn::match_ranges): the smallest R with R^2 >= 64 * tiles, at most 256 and at most tiles;
    returns (tiles per workgroup, workgroups)"""
    tiles = (n_rows + TILE - 1) // TILE
    if tiles == 0:
        return 1, 0
    r = 1
    while r < 256 and r < tiles and r * r < 64 * tiles:
        r += 1
    tpw = (tiles + r - 1) // r
    return tpw, (tiles + tpw - 1) // tpw


def general(rng, n, dim):
    return (rng.standard_normal((n, dim)) * rng.uniform(0.1, 10, (n, 1))).astype(np.float32)


def check(got, want, what):
    why = match_ref.same(got, want)
    assert why is None, (what, why)


# the dozen: every dim, library size, query count and top_m of the issue's lists appears, 65 and 130 queries cross a query pass
IDENTITY = [(1, 1, 1, 1), (1, 65, 17, 10), (7, 63, 64, 10), (7, 4097, 65, 256), (130, 64, 130, 1), (130, 65, 1, 256),
            (256, 4097, 17, 10), (256, 63, 65, 1), (256, 1, 64, 256), (1536, 64, 1, 10), (1536, 65, 64, 1), (1536, 4097, 130, 256)]


@pytest.mark.parametrize("dim,n,nq,M", IDENTITY)
def test_bit_identity_with_index_search(bn, dim, n, nq, M):
    rng = np.random.default_rng([dim, n, nq, M])
    X, Q = general(rng, n, dim), general(rng, nq, dim)
    if dim == 1:
        X, Q = np.abs(X), np.abs(Q)       # dim 1: every score is +-1; keep the fixture's invalid rows the only special ones
    if n > 2:
        X[n // 3] = 0.0                   # a zero row
        X[n // 2, dim // 2] = np.nan      # a NaN row
    if nq > 2:
        Q[nq // 3] = 0.0                  # a zero query
        Q[nq - 1, 0] = np.inf             # an Inf query
    idx = bn.Index(0, dim, n)
    idx.add(X)
    si, ss, sc = idx.search(Q, M)
    got = idx.match(Q, M)
    check(got, match_ref.prefix(si, ss, sc), "no threshold")
    assert np.all(got[2] == 0)           # never tagged
    if nq > 2:
        assert got[3][nq // 3] == 0 and got[3][nq - 1] == 0
    if n > 2:
        assert not np.isin([n // 3, n // 2], got[0][np.arange(M)[None, :] < got[3][:, None]]).any()
    # with a threshold: the prefix of the same lists
    finite = ss[np.isfinite(ss)]
    if finite.size:
        t = float(np.median(finite))
        check(idx.match(Q, M, min_score=t), match_ref.prefix(si, ss, sc, min_score=t), "threshold at the median score")


def test_threshold_on_exact_levels(bn):
    dim, nnz, M = 128, 64, 20
    rng = np.random.default_rng(11)
    lv = np.concatenate([np.full(30, 40), np.full(7, 24), np.full(5, 8), np.full(50, -16), rng.integers(-16, 41, 300)])
    lv = lv[rng.permutation(len(lv))]
    X = ir.rows_at_levels(rng, lv, dim, nnz)
    Q = np.concatenate([ir.canonical_query(dim, nnz)[None], ir.dyadic_rows(rng, 4, dim, nnz)])
    tags = rng.integers(0, 65536, len(X)).astype(np.uint32)
    idx = bn.Index(0, dim, len(X))
    idx.add(X)
    idx.set_tags(0, tags)
    S, qbad, xbad = ir.scores64(Q, X)
    top = ir.top_m_from_scores(S, qbad, xbad, M)
    lowest = float(lv.min()) / nnz
    for name, t in (("at a level with more ties than top_m", 40 / 64), ("between two levels", 33 / 64), ("above all", 41 / 64),
                    ("at the lowest level", lowest), ("between, low", 7 / 64), ("negative zero", -0.0)):
        got = idx.match(Q, M, min_score=t)
        check(got, match_ref.prefix(*top, min_score=t, tags=tags), name)
    got = idx.match(Q[:1], M, min_score=40 / 64)
    assert got[3][0] == M and np.array_equal(got[0][0], np.flatnonzero(lv == 40)[:M])
    assert idx.match(Q[:1], M, min_score=41 / 64)[3][0] == 0
    got = idx.match(Q[:1], 256, min_score=33 / 64)
    assert got[3][0] == int((lv >= 33).sum()) and np.all(got[1][0, :got[3][0]] >= np.float32(33 / 64))
    got = idx.match(Q[:1], 256, min_score=lowest)
    assert got[3][0] == 256


def test_selection_under_load(bn):
    """114 725 rows = 1 793 tiles: the split rule (smallest R with R^2 >= 64 * tiles, at most 256) gives 256 ranges, so 8 tiles per
    workgroup in 225 workgroups: every workgroup but the last walks 8 tiles and carries its lists across them.  The rows are dyadic
    rows sorted by ascending score against query 0, so nearly every row beats the running M-th entry and the pending lists (128
    entries) overflow again and again."""
    n, dim, nnz = 1793 * TILE - 27, 128, 64
    assert match_ranges(n) == (8, 225)
    rng = np.random.default_rng(5)
    X = ir.dyadic_rows(rng, n, dim, nnz)
    X = X[np.argsort(X[:, :nnz].sum(axis=1), kind="stable")]
    Q = np.concatenate([ir.canonical_query(dim, nnz)[None], ir.dyadic_rows(rng, 69, dim, nnz)])
    idx = bn.Index(0, dim, n)
    idx.add(X)
    S, qbad, xbad = ir.scores64(Q, X)
    for M in (10, 256):
        top = ir.top_m_from_scores(S, qbad, xbad, M)
        check(idx.match(Q, M), match_ref.prefix(*top), ("M", M))
        cut = float(top[1][0, M // 2])    # inside query 0's list; ties at the cut stay
        got = idx.match(Q, M, min_score=cut)
        check(got, match_ref.prefix(*top, min_score=cut), ("M", M, "threshold", cut))
        assert 0 < got[3][0] <= M


def test_tags_follow_the_ids(bn):
    rng = np.random.default_rng(6)
    X, Q = general(rng, 700, 96), general(rng, 9, 96)
    idx = bn.Index(0, 96, 1000)
    idx.add(X)
    ids, _, tags, counts = idx.match(Q, 50)
    assert np.all(counts == 50) and np.all(tags == 0)      # an index never tagged: zeros
    idx.fill_tags(0, 700, 3)
    idx.set_tags(100, rng.integers(0, 65536, 500).astype(np.uint32))
    ids, scores, tags, counts = idx.match(Q, 50)
    check((ids, scores, tags, counts), match_ref.prefix(*idx.search(Q, 50), tags=idx.tags()), "tags")
    assert len(np.unique(tags)) > 10


def test_position_independence(bn):
    rng = np.random.default_rng(7)
    dim = 200
    X, Q = general(rng, 1500, dim), general(rng, 130, dim)
    small, large = bn.Index(0, dim, 1500), bn.Index(0, dim, 4000)
    small.add(X)
    large.add(X)
    alone = small.match(Q[69:70], 40)
    among = small.match(Q, 40)
    for a, b in zip(alone, among):
        assert a[0].tobytes() == b[69].tobytes()
    # The same library as the prefix of a larger index.  Through a context's snapshot the bytes are the same outright
    # (test_gpu_match_step.py); bn_index_match searches the index's current size, so here every row the two lists share must
    # carry the same score bits although the split into row ranges differs (1500 rows: 24 ranges; 2500 rows: 40)
    assert match_ranges(1500) != match_ranges(2500)
    large.add(general(rng, 1000, dim))
    big = large.match(Q, 40)
    shared = 0
    for q in range(len(Q)):
        sa = {int(i): s.tobytes() for i, s in zip(among[0][q], among[1][q])}
        for i, s in zip(big[0][q, :big[3][q]], big[1][q]):
            if int(i) in sa:
                assert sa[int(i)] == s.tobytes()
                shared += 1
    assert shared > 40 * len(Q) // 4


def test_more_rows_than_one_round_and_an_empty_index(bn):
    rng = np.random.default_rng(8)
    X, Q = general(rng, 300, 40), general(rng, 600, 40)
    idx = bn.Index(0, 40, 512)
    got = idx.match(Q[:5], 3)
    assert np.all(got[3] == 0)
    idx.add(X)
    check(idx.match(Q, 7, m_stride=9), match_ref.prefix(*idx.search(Q, 7, m_stride=9)), "600 queries")


def test_refusals(bn):
    idx = bn.Index(0, 8, 16)
    idx.add(np.ones((4, 8), dtype=np.float32))
    q = np.ones((2, 8), dtype=np.float32)
    for call, word in ((lambda: idx.match(q, 0), "top_m must be in 1..256"), (lambda: idx.match(q, 257), "top_m must be in 1..256"),
                       (lambda: idx.match(q, 5, m_stride=4), "m_stride < top_m"), (lambda: idx.match(q, 5, min_score=float("nan")), "finite"),
                       (lambda: idx.match(q, 5, min_score=float("inf")), "finite")):
        with pytest.raises(bn.EngineError) as e:
            call()
        assert e.value.status == 1 and word in bn.last_error()
    assert bn.lib.bn_index_match(idx._h, None, 2, 5, 0, 0.0, 5, None, None, None, None) == 1 and "null" in bn.last_error()
    assert idx.match(q, 5)[3].tolist() == [4, 4]
