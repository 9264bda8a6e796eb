"""Row tags and bn_subset_* on the GPU.  Members come from tests/subset_ref.members; expected search results from
subset_ref.restricted_top_m over the score matrix bn_index_search itself gives (test_gpu_ivf.search_matrix) or, for dyadic rows, over
index_ref.scores64.  Counts, ids and score bytes are compared with ==."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import index_ref as ir
import subset_ref
import test_gpu_index_exact as exact
from gpu_helpers import write_model
from subset_ref import Filter
from test_gpu_ivf import as_stored, search_matrix

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
INVALID_ARG = 1
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
EX = subset_ref.EXCLUDE_TAGS


def _bn():
    return importlib.import_module("rust-birdnet-onnx_amd")


def select(bn, idx, f):
    return bn.Subset.select(idx, f.first_id, f.n_ids, f.tags, bool(f.flags & EX))


def cut(want, nq, M):
    """the first nq queries and the first M ranks of a result computed at a larger M"""
    ids, sc, cnt = want
    return ids[:nq, :M], sc[:nq, :M], np.minimum(cnt[:nq], M).astype(np.uint32)


# ---- 1. tags --------------------------------------------------------------------------------------------------------------------
def test_tags_round_trip_refusals_and_no_effect_on_search(bn):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((200, 130)).astype(np.float32)
    Q = rng.standard_normal((5, 130)).astype(np.float32)
    idx = bn.Index(0, 130, 300)
    idx.add(X)
    before = [a.tobytes() for a in idx.search(Q, 50)]
    assert idx.tags().dtype == np.uint32 and not idx.tags().any(), "the tag is 0 until set"
    want = np.zeros(200, dtype=np.uint32)
    want[60:71] = np.arange(11) + 1000                       # across the tile edge at row 64
    idx.set_tags(60, want[60:71])
    assert np.array_equal(idx.tags(), want) and np.array_equal(idx.tags(63, 3), want[63:66])
    idx.fill_tags(190, 10, 65535)
    want[190:] = 65535
    idx.fill_tags(0, 1, 7)
    want[0] = 7
    idx.set_tags(200, [])                                    # nothing, at the end: legal
    idx.fill_tags(5, 0, 3)
    assert np.array_equal(idx.tags(), want) and len(idx.tags(200)) == 0
    # a refused call changes no tag: the whole array is checked before any write
    t = np.array([1, 2, 3, 65536], dtype=np.uint32)
    lib = bn.lib
    assert lib.bn_index_set_tags(idx._h, 10, 4, t.ctypes.data_as(u32p)) == INVALID_ARG and "65536" in bn.last_error()
    assert lib.bn_index_set_tags(idx._h, 198, 3, t.ctypes.data_as(u32p)) == INVALID_ARG and bn.last_error()
    assert lib.bn_index_set_tags(idx._h, 201, 0, t.ctypes.data_as(u32p)) == INVALID_ARG
    assert lib.bn_index_set_tags(idx._h, 10, 3, None) == INVALID_ARG
    assert lib.bn_index_fill_tags(idx._h, 10, 4, 65536) == INVALID_ARG and lib.bn_index_fill_tags(idx._h, 199, 2, 1) == INVALID_ARG
    out = np.full(4, 9, dtype=np.uint32)
    assert lib.bn_index_read_tags(idx._h, 198, 3, out.ctypes.data_as(u32p)) == INVALID_ARG and (out == 9).all()
    assert lib.bn_index_read_tags(idx._h, 0, 3, None) == INVALID_ARG
    assert np.array_equal(idx.tags(), want)
    # tags survive later appends; the new rows have tag 0
    assert idx.add(X[:70]) == 200
    want = np.concatenate([want, np.zeros(70, dtype=np.uint32)])
    assert np.array_equal(idx.tags(), want)
    # tags take no part in the search
    idx2 = bn.Index(0, 130, 300)
    idx2.add(X)
    idx2.fill_tags(0, 200, 5)
    assert [a.tobytes() for a in idx2.search(Q, 50)] == before
    assert [a.tobytes() for a in idx.search(Q, 50)] == [a.tobytes() for a in bn_search_of(bn, np.concatenate([X, X[:70]]), Q, 50)]


def bn_search_of(bn, X, Q, M):
    """bn_index_search over a fresh, untagged index of X"""
    idx = bn.Index(0, X.shape[1], len(X))
    idx.add(X)
    return idx.search(Q, M)


# ---- the shared general case ------------------------------------------------------------------------------------------------------
class General:
    """5 000 Gaussian rows, three of them invalid, skewed tags, 70 queries and the score bn_index_search gives every pair"""

    def __init__(self, dim):
        bn = _bn()
        rng = np.random.default_rng(7000 + dim)
        self.n = n = 5000
        self.X = rng.standard_normal((n, dim)).astype(np.float32)
        self.bad = [100, 2500, 4097]
        self.X[100] = 0.0
        self.X[2500, dim // 3] = np.nan
        self.X[4097, 0] = np.inf
        self.tags = rng.choice(7, n, p=[0.4, 0.2, 0.15, 0.1, 0.08, 0.05, 0.02]).astype(np.uint32)
        self.tags[100], self.tags[2500], self.tags[4097] = 3, 0, 5
        self.Q = (self.X[rng.integers(0, n, 70)] + 0.5 * rng.standard_normal((70, dim))).astype(np.float32)
        self.Q[5:9] = self.X[[0, 63, 64, n - 1]]
        self.idx = bn.Index(0, dim, n)
        self.idx.add(self.X)
        self.idx.set_tags(0, self.tags)
        self.xbad = ~(self.idx.read() != 0).any(axis=1)
        _, self.qbad = as_stored(bn, self.Q)
        self.S = search_matrix(bn, self.X, self.Q)
        # the member lists of the searches: several thousand, exactly 64, 65, 1, 0; the invalid row 100 is in the first three
        big = subset_ref.members(self.tags, n, Filter(tags=[0], flags=EX))
        some = np.sort(np.concatenate([[100], rng.choice(np.setdiff1d(np.arange(n), [100]), 64, replace=False)]))
        self.lists = {"thousands": big, "64": some[some != some[-1]] if some[-1] != 100 else some[1:], "65": some,
                      "1": np.array([n - 1]), "0": np.zeros(0, dtype=np.int64)}
        self.lists = {k: np.asarray(v, dtype=np.uint64) for k, v in self.lists.items()}


@functools.lru_cache(maxsize=None)
def general(dim):
    return General(dim)


# ---- 2. selection -------------------------------------------------------------------------------------------------------------------
FILTERS = (Filter(tags=[3]), Filter(tags=[0, 5, 5]), Filter(tags=[0], flags=EX), Filter(63, 2), Filter(64, 64), Filter(100, 1000),
           Filter(1000, 0, tags=[1, 6]), Filter(4990, 10, tags=[0, 1, 2, 3], flags=EX), Filter(tags=[9]), Filter(5000, 0), Filter())


def test_selection_equals_the_reference(bn):
    g = general(130)
    assert np.array_equal(g.idx.tags(), g.tags) and g.xbad.sum() == 3
    for f in FILTERS:
        want = subset_ref.members(g.tags, g.n, f)
        s = select(bn, g.idx, f)
        got = s.ids
        what = (f.first_id, f.n_ids, f.tags, f.flags)
        assert got.dtype == np.uint64 and len(s) == len(want) and np.array_equal(got, want), what
        assert select(bn, g.idx, f).ids.tobytes() == got.tobytes(), ("two selections differ", what)
    assert len(select(bn, g.idx, Filter(tags=[9]))) == 0 and len(select(bn, g.idx, Filter(tags=[0], flags=EX))) > 2000
    assert np.isin(g.bad, select(bn, g.idx, Filter()).ids).all(), "validity is not tested at selection"
    # an index that never tagged: an absent plane reads as zeros
    plain = bn.Index(0, 130, 200)
    plain.add(g.X[:150])
    assert np.array_equal(select(bn, plain, Filter(tags=[0])).ids, np.arange(150)) and len(select(bn, plain, Filter(tags=[1]))) == 0
    assert np.array_equal(select(bn, plain, Filter(10, 100, tags=[1], flags=EX)).ids, np.arange(10, 110))
    # bn_subset_read by pieces
    s = select(bn, g.idx, Filter(tags=[3]))
    want = subset_ref.members(g.tags, g.n, Filter(tags=[3]))
    part = np.zeros(10, dtype=np.uint64)
    assert bn.lib.bn_subset_read(s._h, len(want) - 10, 10, part.ctypes.data_as(u64p)) == 0 and np.array_equal(part, want[-10:])
    assert bn.lib.bn_subset_read(s._h, len(want) - 9, 10, part.ctypes.data_as(u64p)) == INVALID_ARG


# ---- 3. general data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [130, 1536])
def test_general_data(bn, dim):
    g = general(dim)
    assert not g.qbad.any() and np.array_equal(np.flatnonzero(g.xbad), g.bad)
    assert [len(g.lists[k]) for k in ("64", "65", "1", "0")] == [64, 65, 1, 0] and len(g.lists["thousands"]) > 2000
    for name, mem in g.lists.items():
        assert name in ("1", "0") or 100 in mem, "an invalid row is a member"
        s = select(bn, g.idx, Filter(tags=[0], flags=EX)) if name == "thousands" else bn.Subset.from_ids(g.idx, mem)
        assert np.array_equal(s.ids, mem)
        want = subset_ref.restricted_top_m(g.S, g.qbad, g.xbad, mem, 256)
        for nq in (1, 17, 70):
            for M in (1, 64, 100, 256):
                exact.assert_exact(s.search(g.Q[:nq], M), cut(want, nq, M), (dim, name, "Q", nq, "M", M))
        assert not np.isin(g.bad, want[0][want[2] > 0]).any()


@pytest.mark.parametrize("dim", [130, 1536])
def test_general_data_search_ids(bn, dim):
    g = general(dim)
    rng = np.random.default_rng(6)
    big = g.lists["thousands"].astype(np.int64)
    out = np.setdiff1d(np.arange(g.n), big)
    # queries inside and outside the subset, at its edges, next to each other, and the invalid rows
    qi = np.concatenate([big[[0, 1, 2, -1]], out[[0, 1, -1]], [63, 64, 65], g.bad, rng.choice(big, 30), rng.choice(out, 30)])[:70].astype(np.int64)
    assert len(qi) == 70 and np.isin(qi, big).sum() > 20 and (~np.isin(qi, big)).sum() > 20
    S = search_matrix(bn, g.X, g.X[qi])
    qbad = g.xbad[qi]
    assert qbad.sum() >= 3
    for name in ("thousands", "65", "64", "1", "0"):
        mem = g.lists[name]
        s = bn.Subset.from_ids(g.idx, mem)
        for radius in (-1, 0, 3):
            want = subset_ref.restricted_top_m(S, qbad, g.xbad, mem, 256, qi, radius)
            for nq in (1, 17, 70):
                for M in (1, 64, 100, 256):
                    got = s.search_ids(qi[:nq], M, exclude_radius=radius)
                    exact.assert_exact(got, cut(want, nq, M), (dim, name, "radius", radius, "Q", nq, "M", M))
            if radius >= 0:
                got = s.search_ids(qi, 256, exclude_radius=radius)
                for q in range(70):
                    assert not (np.abs(got[0][q, :got[2][q]].astype(np.int64) - qi[q]) <= radius).any(), (name, radius, q)
            assert not want[2][qbad].any(), "the id of an invalid row gives count 0"


# ---- 4. many list tiles per workgroup ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["constant", "sawtooth", "random"])
def test_dyadic_rows_many_list_tiles_per_workgroup(bn, order):
    case = exact.ordered_case(bn, order, 128, 64)
    n = exact.N
    mem = np.flatnonzero(np.arange(n) % 4 != 0)
    assert len(mem) == 122907 and (len(mem) + 63) // 64 == 1921
    exact.require_many_tiles(len(mem))                       # at least 4 list tiles per workgroup, or fail loudly
    case.idx.set_tags(0, (np.arange(n) % 4).astype(np.uint32))
    s = bn.Subset.select(case.idx, tags=[0], exclude=True)
    assert np.array_equal(s.ids, mem)
    want = subset_ref.restricted_top_m(case.S, case.qbad, case.xbad, mem, 256)   # the float64 sort, ties by id
    for nq in (1, 40, 70):
        for M in (1, 65, 256):
            exact.assert_exact(s.search(case.Q[:nq], M), cut(want, nq, M), (order, "Q", nq, "M", M))
    if order == "constant":
        assert np.array_equal(want[0][0], mem[:256])


# ---- 5. the whole index as a subset -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [130, 1536])
def test_whole_index_equals_the_exact_search(bn, dim):
    g = general(dim)
    a, b = bn.Subset.from_ids(g.idx, np.arange(g.n)), select(bn, g.idx, Filter())
    assert np.array_equal(a.ids, np.arange(g.n)) and a.ids.tobytes() == b.ids.tobytes()
    qi = [0, 63, 64, 100, 2499, g.n - 1]
    for s in (a, b):
        for nq, M in ((1, 1), (17, 100), (70, 256), (64, 64)):
            exact.assert_exact(s.search(g.Q[:nq], M), g.idx.search(g.Q[:nq], M), (dim, "Q", nq, "M", M))
        for radius in (-1, 0, 3):
            exact.assert_exact(s.search_ids(qi, 100, exclude_radius=radius), g.idx.search_ids(qi, 100, exclude_radius=radius), (dim, radius))
    got = a.search(g.Q[:3], 10, m_stride=13)
    exact.assert_exact(got, g.idx.search(g.Q[:3], 10, m_stride=13), "stride")
    assert np.isnan(got[1][:, 10:]).all() and not got[0][:, 10:].any(), "entries past top_m keep the binding's sentinels"


# ---- 6. independence --------------------------------------------------------------------------------------------------------------
def test_independence_of_subset_size_call_shape_and_later_changes(bn):
    g = general(1536)
    row = int(g.lists["65"][40])
    assert row not in g.bad
    Q = np.concatenate([g.X[row][None], g.Q[:69]])             # query 0 is the row itself: it finds the row in any subset
    bits = None
    for members in ([row], g.lists["65"], np.arange(g.n)):
        s = bn.Subset.from_ids(g.idx, members)
        ids, sc, cnt = s.search(Q, 256)
        found = [np.flatnonzero(ids[q, :cnt[q]] == row) for q in range(70)]
        assert len(found[0]) == 1 and (len(s) == g.n or all(len(f) == 1 for f in found)), len(s)   # only the full subset may rank it past 256
        mine = np.array([sc[q, f[0]] if len(f) else np.nan for q, f in enumerate(found)], dtype=np.float32)
        if bits is None:
            bits = mine
        keep = ~np.isnan(mine)
        assert mine[keep].tobytes() == bits[keep].tobytes(), ("score bits depend on the subset", len(s))
    # one call of 70 queries and 70 calls of one
    s = bn.Subset.from_ids(g.idx, g.lists["thousands"])
    whole = s.search(g.Q, 100)
    for q in range(70):
        one = s.search(g.Q[q:q + 1], 100)
        assert all(a.tobytes() == b[q:q + 1].tobytes() for a, b in zip(one, whole)), q
    # a subset made before add / set_tags gives the same results after them
    rng = np.random.default_rng(3)
    X = rng.standard_normal((300, 130)).astype(np.float32)
    idx = bn.Index(0, 130, 500)
    idx.add(X)
    idx.set_tags(0, np.arange(300) % 3)
    s = bn.Subset.select(idx, 10, 250, tags=[1])
    ids0 = s.ids
    before = s.search(X[:70], 100), s.search_ids([0, 11, 13, 299], 50, exclude_radius=1)
    idx.add(X[:150] * np.float32(3.0) + X[150:])
    idx.set_tags(0, np.full(450, 2))
    after = s.search(X[:70], 100), s.search_ids([0, 11, 13, 299], 50, exclude_radius=1)
    assert s.ids.tobytes() == ids0.tobytes() and len(s) == len(subset_ref.members(np.arange(300) % 3, 300, Filter(10, 250, tags=[1])))
    for a, b in zip(before, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert len(bn.Subset.select(idx, 10, 250, tags=[1])) == 0 and len(bn.Subset.select(idx, tags=[2])) == 450
    # query ids are bounded by the index's current size, not the subset's
    assert s.search_ids([449], 5)[2][0] == 5


# ---- 7. invalid queries and rows ------------------------------------------------------------------------------------------------------
def test_invalid_query_and_subset_of_invalid_rows(bn):
    g = general(130)
    Q = g.Q[:5].copy()
    Q[1] = 0.0
    Q[3, 7] = np.nan
    s = bn.Subset.from_ids(g.idx, g.lists["thousands"])
    ids, sc, cnt = s.search(Q, 50)
    assert cnt.tolist() == [50, 0, 50, 0, 50] and not ids[1].any() and np.isnan(sc[3]).all()
    good = s.search(g.Q[[0, 2, 4]], 50)
    assert ids[[0, 2, 4]].tobytes() == good[0].tobytes() and sc[[0, 2, 4]].tobytes() == good[1].tobytes()
    dead = bn.Subset.from_ids(g.idx, g.bad)
    assert len(dead) == 3
    assert not dead.search(g.Q, 256)[2].any() and not dead.search_ids([0, 100, 4097], 256)[2].any()
    empty = bn.Subset.from_ids(g.idx, [])
    assert len(empty) == 0 and len(empty.ids) == 0
    assert not empty.search(g.Q, 256)[2].any() and not empty.search_ids([0, 1], 3, exclude_radius=0)[2].any()


# ---- refusals that need an index ----------------------------------------------------------------------------------------------------
def test_refusals_with_an_index(bn):
    g = general(130)
    lib, size = bn.lib, C.sizeof(bn.BnIndexFilter)
    h = C.c_void_p(0x1234)
    for first, n in ((g.n + 1, 0), (0, g.n + 1), (g.n - 5, 6), (g.n, 1), (1 << 40, 0), (0, 1 << 63)):
        f = bn.BnIndexFilter(first, n, None, 0, 0)
        assert lib.bn_subset_select(g.idx._h, C.byref(f), size, C.byref(h)) == INVALID_ARG and "range" in bn.last_error(), (first, n)
    f = bn.BnIndexFilter(0, 0, None, 0, 0)
    assert lib.bn_subset_select(g.idx._h, C.byref(f), size - 1, C.byref(h)) == INVALID_ARG
    assert lib.bn_subset_select(None, C.byref(f), size, C.byref(h)) == INVALID_ARG and "null" in bn.last_error()
    for bad in ([0, g.n], [g.n], [5, 5], [7, 6], [0, 1, 1 << 33]):
        a = np.array(bad, dtype=np.uint64)
        assert lib.bn_subset_from_ids(g.idx._h, a.ctypes.data_as(u64p), len(a), C.byref(h)) == INVALID_ARG and bn.last_error(), bad
    a = np.array([1], dtype=np.uint64)
    assert lib.bn_subset_from_ids(None, a.ctypes.data_as(u64p), 1, C.byref(h)) == INVALID_ARG
    assert h.value == 0x1234, "nothing created"
    s = bn.Subset.from_ids(g.idx, [1, 2, 3])
    ids, sc, cnt = np.full(8, 0xABCDEF, dtype=np.uint64), np.full(8, -7.5, dtype=np.float32), np.full(2, 77, dtype=np.uint32)
    outs = (ids.ctypes.data_as(u64p), sc.ctypes.data_as(f32p), cnt.ctypes.data_as(u32p))
    q = np.ones((2, 130), dtype=np.float32)
    qi = np.array([0, g.n], dtype=np.uint64)
    assert lib.bn_subset_search_ids(s._h, qi.ctypes.data_as(u64p), 2, -1, 4, 4, *outs) == INVALID_ARG and str(g.n) in bn.last_error()
    assert lib.bn_subset_search(None, q.ctypes.data_as(f32p), 2, 4, 4, *outs) == INVALID_ARG and "null" in bn.last_error()
    for top_m, stride in ((0, 4), (257, 300), (4, 3)):
        assert lib.bn_subset_search(s._h, q.ctypes.data_as(f32p), 2, top_m, stride, *outs) == INVALID_ARG
        assert lib.bn_subset_search_ids(s._h, qi.ctypes.data_as(u64p), 1, 0, top_m, stride, *outs) == INVALID_ARG
    assert (ids == 0xABCDEF).all() and (sc == -7.5).all() and (cnt == 77).all(), "a refused search writes nothing"
    assert lib.bn_subset_search(s._h, None, 0, 4, 4, None, None, None) == 0, "no queries: nothing to refuse"


# ---- 8. a network-filled index ----------------------------------------------------------------------------------------------------
def test_network_filled_index(bn):
    m = bn.Model(write_model(synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)))
    cfg = m.config
    n_samp, sr, B = int(cfg.sample_count), int(cfg.sample_rate), 4
    rng = np.random.default_rng(8)
    pcm = synth.synthetic_segments(1, n_samp * 2 * B, sr)[0]
    pcm = np.clip(pcm + 0.05 * rng.standard_normal(len(pcm)), -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    ctx = bn.Context(m, B)
    n = 2 * B
    idx = bn.Index(0, int(cfg.embedding_dim), n)
    ctx.infer_windows(rec, n_samp, 0, B)
    assert idx.add_context(ctx, B) == 0
    idx.fill_tags(0, B, 1)
    first_only = bn.Subset.select(idx, tags=[1])
    ctx.infer_windows(rec, n_samp, B, B)
    assert idx.add_context(ctx, B) == B
    every = np.arange(n, dtype=np.uint64)
    early = first_only.search_ids(every, n)          # straight after the append: the call orders itself behind it
    idx.fill_tags(B, B, 2)
    s = bn.Subset.select(idx, tags=[2])
    got = s.search_ids(every, n, exclude_radius=0)
    assert np.array_equal(idx.tags(), [1] * B + [2] * B) and np.array_equal(s.ids, np.arange(B, n)) and np.array_equal(first_only.ids, np.arange(B))
    S = np.zeros((n, n), dtype=np.float32)
    ids, sc, cnt = idx.search_ids(every, n)
    assert (cnt == n).all()
    for q in range(n):
        S[q, ids[q].astype(np.int64)] = sc[q]
    none = np.zeros(n, dtype=bool)
    exact.assert_exact(got, subset_ref.restricted_top_m(S, none, none, s.ids, n, every, 0), "second batch")
    exact.assert_exact(early, subset_ref.restricted_top_m(S, none, none, first_only.ids, n), "first batch")
    assert all((got[0][q, :got[2][q]] >= B).all() for q in range(n)) and got[2].tolist() == [B] * B + [B - 1] * B
