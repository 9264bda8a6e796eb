"""bn_index_append_rows / bn_index_append_subset on the GPU.  The expected state of the destination comes from tests/index_copy_ref.py over
the rows bn_index_read gives for the source; rows and tags are compared as bytes.  Dims 3, 130 and 1536 are 1, 2 and 12 units of 512
bytes per row; every source holds an all-zero row, a row with a NaN element and a pair of identical rows."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import index_copy_ref as cr
import index_file_ref as fr
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
INVALID_ARG = 1
SENTINEL = 0xABCDEF0123
DIMS = (3, 130, 1536)
ZERO, NAN, TWIN_A, TWIN_B = 5, 9, 11, 66                     # the twin pair straddles the 64-row tile boundary
TOMB = 7                                                     # the tag that means "dropped"


def _bn():
    return importlib.import_module("rust-birdnet-onnx_amd")


def host_rows(dim, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    if n > TWIN_B:
        X[ZERO] = 0.0
        X[NAN, dim // 2] = np.nan
        X[TWIN_B] = X[TWIN_A]
    return X


def host_tags(n, seed):
    t = np.random.default_rng(seed).choice([0, 1, 2, TOMB, 65535], n, p=[0.3, 0.2, 0.2, 0.2, 0.1]).astype(np.uint32)
    t[:3] = [65535, TOMB, 0]
    if n > TWIN_B:
        t[[ZERO, NAN, TWIN_A, TWIN_B]] = [1, 2, 65535, 0]    # the special rows survive the tombstone filter
    return t


def build(bn, dim, n, seed, tagged, capacity=None):
    """an index of n appended rows and its State"""
    idx = bn.Index(0, dim, capacity or max(n, 1))
    tags = None
    if n:
        idx.add(host_rows(dim, n, seed))
        if tagged:
            tags = host_tags(n, seed)
            idx.set_tags(0, tags)
    st = cr.state(idx.read(), tags, idx.capacity)
    if n > TWIN_B:
        assert np.flatnonzero(~st.valid).tolist() == [ZERO, NAN] and st.rows[TWIN_A].tobytes() == st.rows[TWIN_B].tobytes()
    return idx, st


def agrees(idx, st, what=""):
    assert len(idx) == st.size, what
    assert idx.read().tobytes() == st.rows.tobytes(), ("rows", what)
    assert idx.tags().tobytes() == st.read_tags().tobytes(), ("tags", what)
    if st.size:                                              # the valid bytes, earlier rows' included: a threshold of -inf returns exactly the valid rows
        q = np.ones((1, st.dim), dtype=np.float32)
        assert idx.count_above(q, -np.inf)[0] == st.valid.sum(), ("valid bytes", what)
        if st.size <= 65536:
            ids, _, _, cnt = idx.search_above(q, -np.inf, st.size)
            assert np.array_equal(ids[0, :cnt[0]], np.flatnonzero(st.valid)), ("valid bytes", what)


class Source:
    def __init__(self, dim, n=700):
        self.idx, self.st = build(_bn(), dim, n, 100 + dim, True)
        self.n = n


@functools.lru_cache(maxsize=None)
def source(dim):
    return Source(dim)


def selections(bn, s):
    """name -> (keyword arguments of the reference, the call on a destination)"""
    n, tags = s.n, s.st.tags
    out = {"whole": dict(first_id=0, n_ids=0), "inner": dict(first_id=61, n_ids=70), "tail": dict(first_id=n - 37, n_ids=0),
           "one row": dict(first_id=64, n_ids=1)}
    lists = {"all": np.arange(n), "every other": np.arange(0, n, 2), "single": np.array([TWIN_B]), "last": np.array([n - 1]),
             "by tag": np.flatnonzero(np.isin(tags, [1, 65535])), "without the tombstones": np.flatnonzero(tags != TOMB)}
    subsets = {"all": bn.Subset.select(s.idx), "every other": bn.Subset.from_ids(s.idx, lists["every other"]),
               "single": bn.Subset.from_ids(s.idx, lists["single"]), "last": bn.Subset.from_ids(s.idx, lists["last"]),
               "by tag": bn.Subset.select(s.idx, tags=[1, 65535]), "without the tombstones": bn.Subset.select(s.idx, tags=[TOMB], exclude=True)}
    for k in lists:
        assert np.array_equal(subsets[k].ids, lists[k]) and (k in ("single", "last") or len(lists[k]) > 100)
        out["subset " + k] = dict(ids=lists[k], subset=subsets[k])
    return out


def apply(dst, s, kw):
    if "subset" in kw:
        return dst.append_subset(kw["subset"])
    return dst.append_rows(s.idx, kw["first_id"], kw["n_ids"])


def ref_kw(kw):
    return {k: v for k, v in kw.items() if k != "subset"}


# ---- 1. bytes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_bytes_of_every_selection(bn, dim):
    s = source(dim)
    before = s.idx.read().tobytes(), s.idx.tags().tobytes()
    for name, kw in selections(bn, s).items():
        for held, tagged in ((0, False), (70, True), (3, False)):          # an empty dst, one with tagged rows, one without a plane
            dst, st = build(bn, dim, held, 7 + held, tagged, capacity=held + s.n)
            want, first = cr.append(st, s.st, **ref_kw(kw))
            assert apply(dst, s, kw) == first == held, (name, held)
            agrees(dst, want, (dim, name, held))
            assert want.size == held + len(cr.source_ids(s.st, **ref_kw(kw)))
    assert (s.idx.read().tobytes(), s.idx.tags().tobytes()) == before and len(s.idx) == s.n, "the source is unchanged"


def test_more_units_than_one_pass_of_the_grid(bn):
    """70 001 rows of one unit each: more than 8 workgroups x 32 units on each of 256 CUs, so the grid-stride loop comes round"""
    n = 70001
    src, st = build(bn, 3, n, 3, True)
    for kw in (dict(first_id=0, n_ids=0), dict(ids=np.arange(1, n, 2))):
        dst, dst_st = build(bn, 3, 0, 0, False, capacity=n)
        want, _ = cr.append(dst_st, st, **kw)
        assert (dst.append_subset(bn.Subset.from_ids(src, kw["ids"])) if "ids" in kw else dst.append_rows(src)) == 0
        agrees(dst, want, sorted(kw))


# ---- 2. the subset contract, made literal ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_a_copied_subset_answers_as_the_subset_does(bn, dim):
    s = source(dim)
    sub = bn.Subset.select(s.idx, 3, 650, tags=[TOMB], exclude=True)
    old = sub.ids
    assert ZERO in old and NAN in old and TWIN_A in old and TWIN_B in old and 300 < len(old) < 650
    dst = bn.Index(0, dim, len(old))
    assert dst.append_subset(sub) == 0 and len(dst) == len(old)
    rng = np.random.default_rng(dim)
    Q = np.concatenate([host_rows(dim, s.n, 100 + dim)[[TWIN_A, 0, 699]], rng.standard_normal((14, dim)).astype(np.float32)])
    for M in (1, 100, 256):
        got, want = dst.search(Q, M), sub.search(Q, M)
        assert got[2].tobytes() == want[2].tobytes() and got[1].tobytes() == want[1].tobytes(), (dim, M)
        for q in range(len(Q)):
            assert np.array_equal(old[got[0][q, :got[2][q]].astype(np.int64)], want[0][q, :want[2][q]]), (dim, M, q)
    new_q = np.array([0, 1, len(old) // 2, len(old) - 1, int(np.flatnonzero(old == ZERO)[0]), int(np.flatnonzero(old == TWIN_B)[0])])
    got, want = dst.search_ids(new_q, 100, exclude_radius=-1), sub.search_ids(old[new_q], 100, exclude_radius=-1)
    assert got[2].tobytes() == want[2].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2][4] == 0
    for q in range(len(new_q)):
        assert np.array_equal(old[got[0][q, :got[2][q]].astype(np.int64)], want[0][q, :want[2][q]]), (dim, q)
    # every valid row, in order, with the copied tags
    ids, _, tags, cnt = dst.search_above(Q[:2], -np.inf, len(old))
    valid = np.flatnonzero(s.st.valid[old.astype(np.int64)])
    assert len(valid) == len(old) - 2
    for q in range(2):
        assert cnt[q] == len(valid) and np.array_equal(ids[q, :cnt[q]], valid)
        assert np.array_equal(tags[q, :cnt[q]], s.st.tags[old.astype(np.int64)][valid])


# ---- 3. tag planes ----------------------------------------------------------------------------------------------------------------------
def test_tag_plane_cases(bn):
    dim = 130
    tagged, plain_idx = source(dim), build(bn, dim, 200, 5, False)
    # src with a plane, dst without
    dst, st = build(bn, dim, 10, 1, False, capacity=400)
    want, _ = cr.append(st, tagged.st, 60, 10)
    assert dst.append_rows(tagged.idx, 60, 10) == 10 and want.tags is not None and not want.tags[:10].any()
    agrees(dst, want)
    # src without, dst with: the new tags read 0, whatever the plane held past the size before
    dst, st = build(bn, dim, 10, 2, True, capacity=400)
    want, _ = cr.append(st, plain_idx[1], 0, 0)
    assert dst.append_rows(plain_idx[0]) == 10 and not dst.tags(10).any() and np.array_equal(dst.tags(0, 10), st.tags)
    agrees(dst, want)
    # neither: zeros, and a later bn_index_set_tags works
    dst, st = build(bn, dim, 0, 0, False, capacity=400)
    want, _ = cr.append(st, plain_idx[1], 100, 50)
    assert dst.append_rows(plain_idx[0], 100, 50) == 0 and want.tags is None and not dst.tags().any()
    agrees(dst, want)
    dst.set_tags(45, [9, 8, 7, 6, 5])
    assert dst.tags(44).tolist() == [0, 9, 8, 7, 6, 5] and dst.read().tobytes() == want.rows.tobytes()


# ---- 4. refusals on the device ----------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(bn):
    s = source(130)
    dst, st = build(bn, 130, 70, 4, True, capacity=170)
    other = bn.Index(0, 131, 10)
    mine = bn.Subset.select(dst, 0, 10)
    hundred = bn.Subset.from_ids(s.idx, np.arange(0, 202, 2))    # 101 members into room for 100
    first = C.c_uint64(SENTINEL)
    rows = lambda src, f, n: bn.lib.bn_index_append_rows(dst._h, src._h, f, n, C.byref(first))
    for call, word in ((lambda: rows(other, 0, 0), "dim"), (lambda: rows(dst, 0, 0), "same index"),
                       (lambda: bn.lib.bn_index_append_subset(dst._h, mine._h, C.byref(first)), "borrows"),
                       (lambda: rows(s.idx, s.n + 1, 0), "range"), (lambda: rows(s.idx, 0, s.n + 1), "range"), (lambda: rows(s.idx, s.n, 1), "range"),
                       (lambda: rows(s.idx, 1 << 40, 1 << 63), "range"),
                       (lambda: rows(s.idx, 0, 101), "capacity"), (lambda: rows(s.idx, 0, 0), "capacity"),
                       (lambda: bn.lib.bn_index_append_subset(dst._h, hundred._h, C.byref(first)), "capacity")):
        assert call() == INVALID_ARG and word in bn.last_error(), (word, bn.last_error())
        assert first.value == SENTINEL and len(s.idx) == s.n and len(other) == 0
        agrees(dst, st, word)
    # the empty cases are legal and launch nothing; exactly full is legal
    assert dst.append_rows(s.idx, s.n, 0) == 70 and dst.append_subset(bn.Subset.from_ids(s.idx, [])) == 70 and len(dst) == 70
    assert bn.lib.bn_index_append_rows(dst._h, s.idx._h, 3, 100, None) == 0 and len(dst) == 170
    agrees(dst, cr.append(st, s.st, 3, 100)[0])
    with pytest.raises(bn.EngineError):
        dst.append_rows(s.idx, 0, 1)


# ---- 5. ordering behind a pending bn_index_add_ctx ------------------------------------------------------------------------------------------
def test_the_copy_waits_for_a_pending_append_of_either_index(bn):
    m = bn.Model(write_model(synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)))
    cfg = m.config
    n_samp, sr, B = int(cfg.sample_count), int(cfg.sample_rate), 4
    rec = bn.Recording(np.clip(synth.synthetic_segments(1, n_samp * B, sr)[0], -1, 1).astype(np.float32))
    ctx = bn.Context(m, B)
    dim = int(cfg.embedding_dim)
    src, dst = bn.Index(0, dim, B), bn.Index(0, dim, 3 * B)
    ctx.infer_windows(rec, n_samp, 0, B)
    assert src.add_context(ctx, B) == 0
    assert dst.append_rows(src) == 0                          # straight after the append: the call orders itself behind it
    net = src.read()
    assert (net != 0).any(axis=1).all() and dst.read().tobytes() == net.tobytes()
    # the pending append on the destination's side
    assert dst.add_context(ctx, B) == B
    assert dst.append_rows(src, 1, 0) == 2 * B and len(dst) == 3 * B - 1
    assert dst.read().tobytes() == np.concatenate([net, net, net[1:]]).tobytes()


# ---- 6. views and the file ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [130, 1536])
def test_views_extend_and_the_file_holds_the_copied_bits(bn, dim, tmp_path):
    s = source(dim)
    dst, st = build(bn, dim, 100, 8, True, capacity=800)
    cent = dst.read()[[0, 20, 40, 60, 80]]
    sq, ivf = bn.Sq8(dst), bn.Ivf(dst, cent)
    sub = bn.Subset.select(s.idx, tags=[TOMB], exclude=True)
    want, first = cr.append(st, s.st, ids=sub.ids)
    assert dst.append_subset(sub) == first == 100
    agrees(dst, want)
    assert sq.rows == ivf.rows == 100
    sq.extend()
    ivf.extend()
    assert sq.rows == ivf.rows == want.size
    fresh_sq, fresh_ivf = bn.Sq8(dst), bn.Ivf(dst, cent)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(sq.read(), fresh_sq.read()))
    assert ivf.list_sizes().tobytes() == fresh_ivf.list_sizes().tobytes()
    for c in range(len(ivf)):
        assert ivf.read_list(c).tobytes() == fresh_ivf.read_list(c).tobytes(), c
    path = tmp_path / "copied.bnx"
    dst.save(path)
    assert open(path, "rb").read() == fr.file_bytes(want.rows)
    back = bn.Index.load(path)
    assert len(back) == want.size and back.read().tobytes() == want.rows.tobytes()


# ---- 7. merge ---------------------------------------------------------------------------------------------------------------------------
def test_merge_of_two_sources(bn):
    dim = 130
    a = source(dim)
    b_idx, b = build(bn, dim, 333, 21, False)
    dst, st = build(bn, dim, 0, 0, False, capacity=2000)
    sub = bn.Subset.from_ids(b_idx, np.arange(2, 333, 3))
    firsts = [dst.append_rows(a.idx, 600, 0), dst.append_subset(sub), dst.append_rows(a.idx, 0, 65)]
    st, f0 = cr.append(st, a.st, 600, 0)
    st, f1 = cr.append(st, b, ids=np.arange(2, 333, 3))
    st, f2 = cr.append(st, a.st, 0, 65)
    assert firsts == [f0, f1, f2] == [0, 100, 100 + 111] and st.size == 276
    agrees(dst, st)
    assert not st.tags[100:211].any() and np.array_equal(st.tags[211:], a.st.tags[:65])


# ---- 8. the same bytes twice ---------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(bn):
    s = source(1536)
    sub = bn.Subset.from_ids(s.idx, np.arange(0, s.n, 2))
    runs = []
    for _ in range(2):
        dst = bn.Index(0, 1536, 2 * s.n)
        dst.append_rows(s.idx)
        dst.append_subset(sub)
        runs.append((dst.read().tobytes(), dst.tags().tobytes()))
    assert runs[0] == runs[1] and len(runs[0][0]) == (s.n + len(sub)) * 1536 * 4
