"""Every search over an index across a round boundary of the shared host loop (csrc/index.hip, for_each_round): 1030 queries are two
rounds of the 1024 the index's query buffers hold, so the second round's staging, its pass offsets, its thresholds and the copy into
the caller's arrays at query 1024 onwards all run.  The shape is test_host_plumbing_rounds_and_stride's: 1000 dyadic rows of dim 128,
1030 queries with query 1025 zeroed, an output stride of three more than the entries asked for (the trailing slots keep the binding's
sentinels), each family in both forms: host rows, and stored ids with exclude_radius 2.

Dyadic rows make every f32 score exact, so the expected values are cut from ONE float64 product per form by the references the
families' own tests use, and compared with ==, score bytes included.  ivf at full probe and sq8 where every row is a candidate are
what bn_index_search returns, which is itself checked against index_ref here."""
import numpy as np
import pytest

import above_ref
import group_above_ref
import index_ref as ir
import peaks_ref
import seq_ref
import sq8_ref
import subset_ref
from test_gpu_index_exact import assert_exact, queries, radius_mask

pytestmark = pytest.mark.gpu

N, NQ, DIM, NNZ, M, RADIUS = 1000, 1030, 128, 64, 10, 2
L, NSEQ = 3, 400                     # 341 sequences of 3 windows fit a round of 1024 rows
GROUPS = 3                           # tags are id % 4: tag 3 belongs to no group


class Shape:
    """the index, the queries of both forms and the float64 products every expected value is cut from"""

    def __init__(self, bn):
        rng = np.random.default_rng(53)
        self.X = ir.dyadic_rows(rng, N, DIM, NNZ)
        self.Q = queries(rng, DIM, NNZ, NQ)
        self.Q[1025] = 0                                      # count 0 in the second round
        self.qids = rng.integers(0, N, NQ)
        self.tags = (np.arange(N) % 4).astype(np.uint32)
        self.thr = ((np.arange(NQ) % 5) / 8 - 1 / 16).astype(np.float32)   # one threshold per query, so a round must upload its own
        self.idx = bn.Index(0, DIM, N)
        assert self.idx.add(self.X) == 0
        self.idx.set_tags(0, self.tags)
        self.host = ir.scores64(self.Q, self.X)                # (S, qbad, xbad)
        self.ids = ir.scores64(self.X[self.qids], self.X)
        assert self.host[1].sum() == 1 and not self.ids[1].any() and not self.host[2].any()

    def forms(self):
        """(name, (S, qbad, xbad), qid or None, radius)"""
        return (("host", self.host, None, -1), ("ids", self.ids, self.qids, RADIUS))


def strided(want, stride):
    """(ids, scores, counts) of M entries per query as the binding returns them at m_stride = stride"""
    ids, sc, cnt = want
    wi, ws = np.zeros((len(cnt), stride), dtype=np.uint64), np.full((len(cnt), stride), np.nan, dtype=np.float32)
    wi[:, :ids.shape[1]], ws[:, :ids.shape[1]] = ids, sc
    return wi, ws, cnt


def exact_search(shape, form):
    """bn_index_search / _ids at the stride, checked against index_ref: what ivf and sq8 are then compared with"""
    name, (S, qbad, xbad), qid, radius = form
    ex = None if qid is None else radius_mask(qid, radius, N)
    got = shape.idx.search(shape.Q, M, m_stride=M + 3) if qid is None else shape.idx.search_ids(qid, M, exclude_radius=radius, m_stride=M + 3)
    assert_exact(got, strided(ir.top_m_from_scores(S, qbad, xbad, M, ex), M + 3), ("index", name))
    return got


def check_subset(bn, shape):
    every, tagged = bn.Subset.select(shape.idx), bn.Subset.select(shape.idx, tags=[1, 3])
    assert len(every) == N and tagged.ids.tolist() == [i for i in range(N) if i % 4 in (1, 3)]
    for name, (S, qbad, xbad), qid, radius in shape.forms():
        for what, sub in (("every row", every), ("tags 1 and 3", tagged)):
            want = strided(subset_ref.restricted_top_m(S, qbad, xbad, sub.ids, M, qid, radius), M + 3)
            got = sub.search(shape.Q, M, m_stride=M + 3) if qid is None else sub.search_ids(qid, M, exclude_radius=radius, m_stride=M + 3)
            assert_exact(got, want, ("subset", what, name))
            if sub is every:
                ex = None if qid is None else radius_mask(qid, radius, N)
                assert_exact(got, strided(ir.top_m_from_scores(S, qbad, xbad, M, ex), M + 3), ("subset of every row is the index", name))


def check_peaks(bn, shape):
    for name, (S, qbad, xbad), qid, radius in shape.forms():
        want = strided(peaks_ref.peaks_top_m(S, peaks_ref.eligibility(N, qbad, xbad, qid, radius), 2, M), M + 3)
        got = (shape.idx.search_peaks(shape.Q, M, 2, m_stride=M + 3) if qid is None
               else shape.idx.search_peaks_ids(qid, M, 2, exclude_radius=radius, m_stride=M + 3))
        assert_exact(got, want, ("peaks", name))


def check_seq(bn, shape):
    """400 sequences of 3 windows: 341 in the first round, 59 in the second; host sequence 341 = windows 1023..1025 holds the zeroed query"""
    W = np.concatenate([shape.Q, shape.Q[:NSEQ * L - NQ]])    # 1200 window rows
    S, qbad, xbad = ir.scores64(W, shape.X)
    want = strided(seq_ref.seq_top_m(S, qbad, xbad, L, 0, M), M + 3)
    assert want[2][341] == 0 and (np.delete(want[2], 341) == M).all()
    assert_exact(shape.idx.search_seq(W, L, M, m_stride=M + 3), want, ("seq", "host"))
    first = np.random.default_rng(54).integers(0, N - L + 1, NSEQ)
    rows = (first[:, None] + np.arange(L)[None, :]).reshape(-1)
    S, qbad, xbad = ir.scores64(shape.X[rows], shape.X)
    want = strided(seq_ref.seq_top_m(S, qbad, xbad, L, 0, M, first, RADIUS), M + 3)
    assert_exact(shape.idx.search_seq_ids(first, L, RADIUS, M, m_stride=M + 3), want, ("seq", "ids"))


def check_above(bn, shape):
    for name, (S, qbad, xbad), qid, radius in shape.forms():
        hits = above_ref.hits_from_scores(S, qbad, xbad, shape.thr, 0, 0, qid, radius)
        n_hits = np.array([len(h[0]) for h in hits])
        second = n_hits[1024:]
        assert (second > 50).any() and ((second > 0) & (second < 50)).any() and (second == 0).any(), "the second round: truncated, short and empty lists"
        for max_hits in (0, 50):
            want = above_ref.layout(hits, max_hits, max_hits + 3, shape.tags)
            got = (shape.idx.search_above(shape.Q, shape.thr, max_hits, h_stride=max_hits + 3) if qid is None
                   else shape.idx.search_above_ids(qid, shape.thr, max_hits, exclude_radius=radius, h_stride=max_hits + 3))
            assert_exact((got[0], got[1], got[3]), (want[0], want[1], want[3]), ("above", name, max_hits))
            assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2]), ("above", name, max_hits, "tags")
        if qid is None:
            assert np.array_equal(shape.idx.count_above(shape.Q, shape.thr), n_hits.astype(np.uint32))


def check_group_above(bn, shape):
    for name, (S, qbad, xbad), qid, radius in shape.forms():
        want = group_above_ref.from_scores(S, qbad, xbad, shape.thr, GROUPS, shape.tags, 0, 0, qid, radius, GROUPS + 3)
        assert want[5][1024:].any() and want[0][1024:].any()
        got = (shape.idx.group_above(shape.Q, shape.thr, GROUPS, g_stride=GROUPS + 3) if qid is None
               else shape.idx.group_above_ids(qid, shape.thr, GROUPS, exclude_radius=radius, g_stride=GROUPS + 3))
        group_above_ref.assert_same(got, want, ("group_above", name))


def check_ivf(bn, shape):
    k = 5
    ivf = bn.Ivf(shape.idx, shape.X[np.random.default_rng(55).integers(0, N, k)])
    for form in shape.forms():
        name, _, qid, radius = form
        want = exact_search(shape, form)
        got = ivf.search(shape.Q, k, M, m_stride=M + 3) if qid is None else ivf.search_ids(qid, k, M, exclude_radius=radius, m_stride=M + 3)
        assert_exact(got[:3], want, ("ivf", name))
        assert got[3].shape == (NQ, k) and (np.sort(got[3][0]) == np.arange(k)).all() and (np.sort(got[3][1029]) == np.arange(k)).all()
        assert got[4][1029] == N and got[4][1024] == N and (got[4][1025] == 0) == (qid is None), "probes and scanned rows of the second round"


def check_sq8(bn, shape):
    """refine 256.  Over the 1000 rows the candidates are sq8_ref's and the result their exact re-rank; over the first 256 rows every
    row is a candidate and the result is bn_index_search's"""
    view = bn.Sq8(shape.idx)
    stored = ir.stored(shape.X, NNZ)
    assert shape.idx.read().tobytes() == stored.tobytes()
    Qn = ir.stored(shape.Q, NNZ)
    Qn[1025] = 0
    for name, (S, qbad, xbad), qid, radius in shape.forms():
        ex = None if qid is None else radius_mask(qid, radius, N)
        wi, ws, wc, wcand, wcc = sq8_ref.Expected(stored, Qn if qid is None else stored[qid], S, excluded=ex).at(256, M)
        got = view.search(shape.Q, 256, M, m_stride=M + 3) if qid is None else view.search_ids(qid, 256, M, exclude_radius=radius, m_stride=M + 3)
        assert_exact(got[:3], strided((wi, ws, wc), M + 3), ("sq8", name))
        assert np.array_equal(got[4], wcc) and np.array_equal(got[3], wcand), ("sq8", name, "candidates")
    small = bn.Index(0, DIM, 256)
    small.add(shape.X[:256])
    view = bn.Sq8(small)
    qids = shape.qids % 256
    for got, want in ((view.search(shape.Q, 256, M, m_stride=M + 3), small.search(shape.Q, M, m_stride=M + 3)),
                      (view.search_ids(qids, 256, M, exclude_radius=RADIUS, m_stride=M + 3), small.search_ids(qids, M, exclude_radius=RADIUS, m_stride=M + 3))):
        assert_exact(got[:3], want, "sq8 with every row a candidate")
    S, qbad, xbad = ir.scores64(shape.Q, shape.X[:256])
    assert_exact(small.search(shape.Q, M, m_stride=M + 3), strided(ir.top_m_from_scores(S, qbad, xbad, M), M + 3), "the small index")


def test_every_family_across_a_round_boundary(bn):
    shape = Shape(bn)
    for check in (check_subset, check_peaks, check_seq, check_above, check_group_above, check_ivf, check_sq8):
        check(bn, shape)
