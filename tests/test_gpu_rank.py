"""bn_head_rank_index on the GPU.  Every expected value comes from code the feature did not add or from numpy: the logits are
bn_head_apply_host's of the twin head (same W and b, flags 0) on the rows bn_index_read returns, the selection is tests/rank_ref.py,
and the comparisons are ==: counts, ids and the bytes of the logits.

On top of that: the head block's float64 bound, identity with the logits of the step that appended a window, ties (by id, z
against -z, -0.0 against +0.0), ranges / exclusions / counts, many tiles per workgroup under three row orders, position
independence, nothing else moved, every refusal, and the search -> label -> fit -> rank loop."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import rank_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
MODES = ("top", "uncertain")
ID_SENTINEL, LOGIT_SENTINEL, COUNT_SENTINEL = 0xABABABABABABABAB, np.float32(123.25), 0xCDCDCDCD


def stored_rows(idx):
    """(rows as the index stores them, their validity: a stored row is all zeros exactly when the index holds it invalid)"""
    S = idx.read()
    return S, (S != 0).any(axis=1)


def twin_logits(bn, W, b, S):
    """the oracle's logits: bn_head_apply_host of a head with the same W and b and flags 0, on the stored rows"""
    return bn.Head(0, W, b, l2norm=False).apply(S)


def raw_rank(bn, head_h, index_h, mode, first_id, n_ids, exclude, top_m, m_stride, n_classes, null=()):
    """the C entry point on sentinel-filled outputs: (status, ids, logits, counts)"""
    ids = np.full((n_classes, max(m_stride, 1)), ID_SENTINEL, dtype=np.uint64)
    logits = np.full((n_classes, max(m_stride, 1)), LOGIT_SENTINEL, dtype=np.float32)
    counts = np.full(n_classes, COUNT_SENTINEL, dtype=np.uint32)
    ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64)
    st = bn.lib.bn_head_rank_index(head_h, index_h, mode, first_id, n_ids, None if ex is None or "exclude" in null else ex.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   0 if ex is None else len(ex), top_m, m_stride,
                                   None if "ids" in null else ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   None if "logits" in null else logits.ctypes.data_as(C.POINTER(C.c_float)),
                                   None if "counts" in null else counts.ctypes.data_as(C.POINTER(C.c_uint32)))
    return st, ids, logits, counts


def assert_same(got, want, what=""):
    gi, gz, gc = got
    wi, wz, wc = want
    assert np.array_equal(gc, wc), (what, gc, wc)
    for c in range(len(wc)):
        k = int(wc[c])
        assert np.array_equal(gi[c, :k], wi[c, :k]), (what, c)
        assert gz[c, :k].tobytes() == wz[c, :k].tobytes(), (what, c)


# ---- exactness ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(dim, classes):
    """1000 random rows (a zero row, a NaN row, an Inf row among them) in an index, an L2NORM head, and the oracle's logits"""
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    rng = np.random.default_rng(1000 * dim + classes)
    X = (rng.standard_normal((1000, dim)) * rng.uniform(0.1, 10, (1000, 1))).astype(np.float32)
    X[7] = 0.0
    X[300, dim // 2] = np.nan
    X[941, 0] = np.inf
    W = rng.standard_normal((classes, dim)).astype(np.float32)
    b = rng.standard_normal(classes).astype(np.float32)
    if dim > 1:
        X[20:30, 0] = 0.0  # with the infinite weight below: NaN logits of class 1 on valid rows
        if classes > 1:
            W[1, 0] = np.inf
    idx = bn.Index(0, dim, 1000)
    idx.add(X)
    head = bn.Head(0, W, b, l2norm=True)
    S, valid = stored_rows(idx)
    assert not valid[7] and not valid[300] and not valid[941] and valid.sum() == 997
    Z = twin_logits(bn, W, b, S)
    return idx, head, W, b, S, valid, Z


@pytest.mark.parametrize("classes", [1, 3, 65])
@pytest.mark.parametrize("dim", [1, 130, 1536])
def test_bits_and_selection(bn, dim, classes):
    idx, head, W, b, S, valid, Z = _case(dim, classes)
    if dim > 1 and classes > 1:
        assert np.isnan(Z[20:30, 1]).all() and np.isinf(Z[31, 1])
    for mode in MODES:
        for M in (1, 10, 256):
            got = head.rank_index(idx, M, mode)
            want = rank_ref.rank(Z, valid, mode, M)
            assert_same(got, want, (mode, M))
            for c in range(classes):  # no invalid row, no NaN logit
                k = int(got[2][c])
                assert valid[got[0][c, :k].astype(np.int64)].all() and not np.isnan(got[1][c, :k]).any()


@pytest.mark.parametrize("dim", [1, 130, 1536])
def test_float64_bound(bn, dim):
    idx, head, W, b, S, valid, Z = _case(dim, 3)
    Wf = np.where(np.isfinite(W), W, 0).astype(np.float64)  # the infinite weight's class is left out below
    z64 = S.astype(np.float64) @ Wf.T + b.astype(np.float64)
    mag = np.abs(S.astype(np.float64)) @ np.abs(Wf).T + np.abs(b.astype(np.float64))
    bound = 2.0 * (dim + 8) * 2.0 ** -24 * mag
    worst = 0.0
    for mode in MODES:
        ids, z, counts = head.rank_index(idx, 256, mode)
        for c in range(3):
            if not np.isfinite(W[c]).all():
                continue
            r = ids[c, :counts[c]].astype(np.int64)
            err = np.abs(z[c, :counts[c]].astype(np.float64) - z64[r, c])
            worst = max(worst, float((err / bound[r, c]).max()))
            assert np.all(err <= bound[r, c])
    print(f"dim {dim}: worst |z - z64| / bound = {worst:.4f}")


@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v30(num_species=300, width=0.5, depth=0.5, emb=256)))


def test_step_identity(bn, model):
    rng = np.random.default_rng(3)
    dim, B = int(model.config.embedding_dim), 5
    W = rng.standard_normal((7, dim)).astype(np.float32)
    b = rng.standard_normal(7).astype(np.float32)
    head = bn.Head(0, W, b, l2norm=True)
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    x = synth.synthetic_segments(1, S * B, sr)[0]
    pcm = np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    ctx = bn.Context(model, B)
    ctx.attach_head(head, top_k=3)
    ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
    step_logits = ctx.step_head_results(B)[0].copy()
    idx = bn.Index(0, dim, 16)
    assert idx.add_context(ctx, B) == 0
    for mode in MODES:
        ids, z, counts = head.rank_index(idx, 8, mode)  # the call waits for the pending append itself
        assert np.all(counts == B)
        for c in range(7):
            assert sorted(ids[c, :B].tolist()) == list(range(B))
            assert z[c, :B].tobytes() == step_logits[ids[c, :B].astype(np.int64), c].tobytes(), (mode, c)


# ---- ordering -------------------------------------------------------------------------------------------------------
def test_ties(bn):
    rng = np.random.default_rng(4)
    dim = 20
    v = rng.standard_normal((2, dim)).astype(np.float32)
    X = np.tile(np.stack([v[0], -v[0], v[1], -v[1]]), (175, 1))  # 700 rows of 4 distinct vectors, in x / -x pairs
    W = np.zeros((4, dim), dtype=np.float32)
    W[0] = rng.standard_normal(dim)
    W[1] = rng.standard_normal(dim)
    b = np.array([0.375, 0.0, -0.0, 0.0], dtype=np.float32)
    assert np.signbit(b[2]) and not np.signbit(b[3])
    idx = bn.Index(0, dim, 700)
    idx.add(X)
    head = bn.Head(0, W, b, l2norm=True)
    S, valid = stored_rows(idx)
    Z = twin_logits(bn, W, b, S)
    assert len(np.unique(Z[:, 0])) == 4 and np.array_equal(Z[0::4, 1], -Z[1::4, 1]) and Z[0, 1] != 0
    for mode in MODES:
        for M in (1, 100, 256):
            ids, z, counts = got = head.rank_index(idx, M, mode)
            assert_same(got, rank_ref.rank(Z, valid, mode, M), (mode, M))
            for c in range(4):  # inside a run of equal keys the ids ascend
                key = np.abs(z[c]) if mode == "uncertain" else z[c]
                same = key[1:] == key[:-1]
                assert np.all(ids[c, 1:][same] > ids[c, :-1][same])
            assert np.array_equal(ids[2], ids[3]) and np.array_equal(ids[2], np.arange(M))  # b = -0.0 and b = +0.0: one order
    ids, z, _ = head.rank_index(idx, 256, "uncertain")
    a = np.abs(Z[:, 1])
    small = np.flatnonzero(a == a.min())[:256]  # z and -z alternate along the ids and tie
    assert np.array_equal(ids[1], small) and (z[1] > 0).any() and (z[1] < 0).any()


def test_range_exclusions_counts(bn):
    idx, head, W, b, S, valid, Z = _case(130, 3)
    n, C_ = Z.shape
    h, x = head._h, idx._h
    top1 = rank_ref.rank(Z, valid, "top", 1)[0][:, 0]
    unc1 = rank_ref.rank(Z, valid, "uncertain", 1)[0][:, 0]
    for mi, mode in enumerate(MODES):
        best = top1 if mode == "top" else unc1
        cases = [
            dict(first_id=70, n_ids=30),      # inside one tile
            dict(first_id=50, n_ids=200),     # across tiles, each a workgroup of its own at this size
            dict(first_id=63, n_ids=2),
            dict(first_id=n, n_ids=0),        # exactly 0 rows
            dict(first_id=900, n_ids=0),      # to the end
            dict(first_id=0, n_ids=n),
            dict(exclude=np.concatenate([best, best, [5, 5, 999, 0]]).astype(np.uint64)),  # duplicates, every class's top-1
            dict(first_id=100, n_ids=500, exclude=np.arange(90, 300, dtype=np.uint64)),
        ]
        for kw in cases:
            for M in (1, 256):
                st, ids, z, counts = raw_rank(bn, h, x, mi, kw.get("first_id", 0), kw.get("n_ids", 0), kw.get("exclude"), M, M + 3, C_)
                assert st == 0, bn.last_error()
                want = rank_ref.rank(Z, valid, mode, M, m_stride=M + 3, **kw)
                assert_same((ids, z, counts), want, (mode, kw, M))
                for c in range(C_):  # slots past count keep the caller's bytes
                    assert np.all(ids[c, counts[c]:] == ID_SENTINEL) and np.all(z[c, counts[c]:] == LOGIT_SENTINEL)
                if "exclude" in kw:
                    assert not np.isin(ids[:, :M][ids[:, :M] != ID_SENTINEL], kw["exclude"]).any()
        st, ids, z, counts = raw_rank(bn, h, x, mi, 70, 10, None, 256, 256, C_)  # eligible rows < M
        assert st == 0 and np.all(counts == 10) and np.all(ids[:, 10:] == ID_SENTINEL)
        st, ids, z, counts = raw_rank(bn, h, x, mi, n, 0, None, 4, 4, C_)
        assert st == 0 and np.all(counts == 0) and np.all(ids == ID_SENTINEL) and np.all(z == LOGIT_SENTINEL)
    empty = bn.Index(0, 130, 10)
    for mi in (0, 1):
        st, ids, z, counts = raw_rank(bn, h, empty._h, mi, 0, 0, None, 4, 4, C_)
        assert st == 0 and np.all(counts == 0) and np.all(ids == ID_SENTINEL)


def _compute_units():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows_for_eight_tiles_per_workgroup(cus):
    """the scan's grid rule (tiles of 64 rows; tiles per workgroup = ceil(tiles / compute units); workgroups = ceil(tiles /
    that)): the smallest tile count at which every workgroup, the last included, walks >= 8 tiles; the last tile is partial"""
    t = 8 * cus
    while True:
        tpw = -(-t // cus)
        n_wg = -(-t // tpw)
        if tpw >= 8 and t - (n_wg - 1) * tpw >= 8:
            return t * 64 - 27, tpw, n_wg
        t += 1


@pytest.mark.parametrize("order", ["ascending", "descending", "best_last"])
def test_many_tiles_per_workgroup(bn, order):
    dim, P = 8, 300
    n, tpw, n_wg = _rows_for_eight_tiles_per_workgroup(_compute_units())
    rng = np.random.default_rng(6)
    pool = rng.standard_normal((P, dim)).astype(np.float32)
    w = rng.standard_normal(dim).astype(np.float32)
    # the pool's own logits, to lay the rows out by key: class 0 (TOP) and class 1 = the same weights shifted so that its |z| is
    # smallest where class 0 is largest (UNCERTAIN meets the same adversarial order)
    tmp = bn.Index(0, dim, P)
    tmp.add(pool)
    zp = twin_logits(bn, w[None, :], np.zeros(1, dtype=np.float32), tmp.read())[:, 0]
    by_z = np.argsort(zp, kind="stable")
    W = np.stack([w, w])
    b = np.array([0.0, -zp.max()], dtype=np.float32)
    if order == "best_last":  # the two best pool vectors only inside the last workgroup's range; everything else random
        assign = by_z[rng.integers(0, P - 2, n)]
        tail = 8 * 64 - 27 - 5
        assign[n - tail:] = by_z[P - 2 + rng.integers(0, 2, tail)]
        assert tail >= 256
    else:
        assign = by_z[np.sort(rng.integers(0, P, n))]  # a few hundred distinct values: ties cross every workgroup boundary
        if order == "descending":
            assign = assign[::-1]
    idx = bn.Index(0, dim, n)
    idx.add(pool[assign])
    head = bn.Head(0, W, b, l2norm=True)
    S, valid = stored_rows(idx)
    assert valid.all()
    Z = twin_logits(bn, W, b, S)
    assert 200 < len(np.unique(Z[:, 0])) <= P
    print(f"{n} rows, {n_wg} workgroups x {tpw} tiles")
    for mode in MODES:
        for M in (256, 1):
            assert_same(head.rank_index(idx, M, mode), rank_ref.rank(Z, valid, mode, M), (order, mode, M))
    if order == "best_last":
        ids, _, _ = head.rank_index(idx, 256, "top")
        assert ids[0].min() >= (n_wg - 1) * tpw * 64


def test_position_independence(bn):
    rng = np.random.default_rng(7)
    dim = 130
    X = rng.standard_normal((64, dim)).astype(np.float32)
    W = rng.standard_normal((3, dim)).astype(np.float32)
    b = rng.standard_normal(3).astype(np.float32)
    head = bn.Head(0, W, b, l2norm=True)
    a = bn.Index(0, dim, 64)
    a.add(X)
    big = bn.Index(0, dim, 10064)
    big.add(rng.standard_normal((10000, dim)).astype(np.float32))
    assert big.add(X) == 10000
    for mode in MODES:
        ia, za, ca = head.rank_index(a, 64, mode)
        ib, zb, cb = head.rank_index(big, 64, mode, first_id=10000)
        assert np.all(ca == 64) and np.all(cb == 64)
        assert np.array_equal(ia + 10000, ib) and za.tobytes() == zb.tobytes()
        # and inside a ranking of the whole index the same rows carry the same bytes
        iw, zw, _ = head.rank_index(big, 256, mode)
        for c in range(3):
            late = iw[c] >= 10000
            want = {int(i) + 10000: z for i, z in zip(ia[c], za[c])}
            assert all(want[int(i)].tobytes() == z.tobytes() for i, z in zip(iw[c][late], zw[c][late]))


# ---- safety ---------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(bn):
    idx, head, W, b, S, valid, Z = _case(130, 3)
    q = S[[3, 500, 998]]
    before = idx.search(q, 20), head.read(), idx.read().tobytes(), len(idx)
    first = [head.rank_index(idx, 50, mode, exclude=[1, 2, 3]) for mode in MODES]
    second = [head.rank_index(idx, 50, mode, exclude=[1, 2, 3]) for mode in MODES]
    for f, s in zip(first, second):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(f, s))
    after = idx.search(q, 20), head.read(), idx.read().tobytes(), len(idx)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[0], after[0]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before[1], after[1]))
    assert before[2:] == after[2:]


def test_refusals(bn):
    idx, head, W, b, S, valid, Z = _case(130, 3)
    n = len(idx)
    h, x = head._h, idx._h
    other_dim = bn.Head(0, np.ones((3, 131), dtype=np.float32), None, l2norm=True)
    raw_head = bn.Head(0, W, b, l2norm=False)
    ok = dict(head_h=h, index_h=x, mode=0, first_id=0, n_ids=0, exclude=None, top_m=4, m_stride=4)
    bad = [
        dict(head_h=None), dict(index_h=None),                                   # NULL where data is required
        dict(null=("ids",)), dict(null=("logits",)), dict(null=("counts",)),
        dict(exclude=[1, 2], null=("exclude",)),
        dict(mode=2), dict(mode=0xFFFFFFFF),                                     # an unknown mode
        dict(top_m=0, m_stride=4), dict(top_m=257, m_stride=300),                # top_m outside 1..256
        dict(top_m=4, m_stride=3),                                               # m_stride < top_m
        dict(first_id=n + 1),                                                    # first_id > size
        dict(first_id=n - 5, n_ids=6), dict(first_id=0, n_ids=n + 1),            # a range that runs past the end
        dict(first_id=1, n_ids=2 ** 64 - 1),
        dict(exclude=[0, n]), dict(exclude=[2 ** 40]),                           # an excluded id >= size
        dict(head_h=other_dim._h),                                               # dim mismatch
        dict(head_h=raw_head._h),                                                # a head without BN_HEAD_L2NORM
    ]
    if bn.device_count() > 1:  # a head can only be made on a device that exists: one GPU cannot reach this refusal
        elsewhere = bn.Head(1, W, b, l2norm=True)
        bad.append(dict(head_h=elsewhere._h))
    for i, kw in enumerate(bad):
        a = dict(ok, **kw)
        null = a.pop("null", ())
        st, ids, z, counts = raw_rank(bn, a["head_h"], a["index_h"], a["mode"], a["first_id"], a["n_ids"], a["exclude"], a["top_m"], a["m_stride"], 3, null)
        assert st == 1 and bn.last_error(), (i, kw)
        assert np.all(ids == ID_SENTINEL) and np.all(z == LOGIT_SENTINEL) and np.all(counts == COUNT_SENTINEL), (i, kw)
    # after the refusals a valid call still works
    assert_same(head.rank_index(idx, 4, "top"), rank_ref.rank(Z, valid, "top", 4))


# ---- end to end -----------------------------------------------------------------------------------------------------
def test_search_label_fit_rank_loop(bn):
    rng = np.random.default_rng(10)
    dim = 256
    c = np.linalg.qr(rng.standard_normal((dim, 2)))[0].T  # two orthonormal centres
    spread = np.linspace(0.05, 0.6, 300)

    def cluster(centre):
        return centre[None, :] + spread[:, None] * rng.standard_normal((300, dim)) / np.sqrt(dim)

    exemplar = (c[0] + c[1])[None, :]
    X = np.concatenate([cluster(c[0]), cluster(c[1]), rng.standard_normal((100, dim)), exemplar]).astype(np.float32)
    positive = np.zeros(len(X), dtype=bool)
    positive[:300] = True
    perm = rng.permutation(len(X))
    X, positive = X[perm], positive[perm]
    ex_id = int(np.flatnonzero(perm == 700)[0])
    idx = bn.Index(0, dim, len(X))
    idx.add(X)
    hits, _, cnt = idx.search_ids([ex_id], 200, exclude_radius=0)
    labelled = hits[0, :cnt[0]]
    y = positive[labelled.astype(np.int64)].astype(np.uint8)[:, None]
    assert 40 < y.sum() < 160  # the hits hold both clusters
    head = bn.Head.fit_index(idx, labelled, y)
    unlabelled_pos = int(positive.sum() - y.sum())
    ids, z, counts = head.rank_index(idx, 256, "top", exclude=labelled)
    assert counts[0] == 256 and unlabelled_pos < 256
    assert positive[ids[0, :unlabelled_pos].astype(np.int64)].all()      # every unlabelled positive ahead of every negative
    assert not positive[ids[0, unlabelled_pos:].astype(np.int64)].any()
    top_ids, top_z, _ = head.rank_index(idx, 20, "top", exclude=labelled)
    unc_ids, unc_z, unc_n = head.rank_index(idx, 20, "uncertain", exclude=labelled)
    assert unc_n[0] == 20 and not np.isin(unc_ids[0], labelled).any()
    assert np.abs(unc_z[0]).max() < np.abs(top_z[0]).min()
