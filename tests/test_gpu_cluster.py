"""bn_index_assign / bn_index_cluster on the GPU.  Every expected score comes from code older than the feature: the scores are
bn_head_apply_host's of a head with W = centroids, no bias and flags 0 on the rows bn_index_read returns; the argmax and the
centroid update are tests/cluster_ref.py; assignments and score bytes are compared with ==.

On top of that: position independence (centroid order, id ranges, append blocks), many tiles per workgroup, one update against a
float64 evaluation under the header's bound, chaining and determinism, convergence properties, planted clusters under the built-in
max-min start, the empty cluster, every refusal, nothing else moved, and the cluster -> search loop on a network-filled index."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import cluster_ref
import test_gpu_index_exact as exact
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
NONE = cluster_ref.NONE


def stored_rows(idx):
    S = idx.read()
    return S, (S != 0).any(axis=1)


def twin_scores(bn, cent, S):
    """the oracle's scores: bn_head_apply_host of a head with W = centroids, no bias, flags 0"""
    return bn.Head(0, np.ascontiguousarray(cent, dtype=np.float32), None, l2norm=False).apply(S)


def assert_exact_assignment(bn, idx, cent, assign, score, first=0, what=""):
    """(assign, score) of rows [first, first + len(assign)) is cluster_ref.assign of the twin head's scores, bytes and all"""
    S, valid = stored_rows(idx)
    wa, ws = cluster_ref.assign(twin_scores(bn, cent, S), valid)
    wa, ws = wa[first:first + len(assign)], ws[first:first + len(assign)]
    assert np.array_equal(assign, wa), (what, np.flatnonzero(assign != wa)[:8], assign[assign != wa][:8], wa[assign != wa][:8])
    assert score.tobytes() == ws.tobytes(), (what, np.flatnonzero(score.view(np.uint32) != ws.view(np.uint32))[:8])
    return wa, ws


# ---- 1. bits and assignment -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rows(dim):
    """test_gpu_rank._case's 1000 rows: a zero row, a NaN row, an Inf row; with dim > 1 rows whose component 0 is zero and two
    rows that overflow against the huge centroid"""
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    rng = np.random.default_rng(1000 * dim)
    X = (rng.standard_normal((1000, dim)) * rng.uniform(0.1, 10, (1000, 1))).astype(np.float32)
    X[7] = 0.0
    X[300, dim // 2] = np.nan
    X[941, 0] = np.inf
    if dim > 1:
        X[20:30, 0] = 0.0
        X[40] = 0.0
        X[40, :6] = 1.0
        X[41] = 0.0
        X[41, :6] = -1.0
    idx = bn.Index(0, dim, 1000)
    idx.add(X)
    S, valid = stored_rows(idx)
    assert not valid[7] and not valid[300] and not valid[941] and valid.sum() == 997
    return idx, X, S, valid


def _centroids(dim, k):
    rng = np.random.default_rng(77 * dim + k)
    c = rng.standard_normal((k, dim)).astype(np.float32)
    c /= np.sqrt((c.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    if dim > 1 and k > 1:
        c[1] = 0.0
        c[1, :6] = 3e38                  # finite, huge: +inf and -inf scores on rows 40 and 41
    if dim > 1 and k >= 6:
        c[4] = 0.0
        c[4, 0] = 1.5                    # c and -c, both orthogonal to rows 20..29: +-0 scores
        c[5] = -c[4]
    if k >= 3:
        c[2] = c[0]                      # a duplicate: every tie goes to index 0
    if k >= 65:
        c[64] = c[1]                     # a duplicate across the pass boundary
        c[k - 1] = c[3]
    return c


@pytest.mark.parametrize("k", [1, 3, 64, 65, 130])
@pytest.mark.parametrize("dim", [1, 130, 1536])
def test_bits_and_assignment(bn, dim, k):
    idx, X, S, valid = _rows(dim)
    cent = _centroids(dim, k)
    assign, score = idx.assign(cent)
    Z = twin_scores(bn, cent, S)
    wa, ws = assert_exact_assignment(bn, idx, cent, assign, score, what=(dim, k))
    assert np.all(assign[~valid] == NONE) and np.isnan(score[~valid]).all() and not np.isnan(score[valid]).any()
    if k >= 3:
        assert not (assign == 2).any()
    if k >= 65:
        assert not (assign == 64).any() and not (assign == k - 1).any()
    if dim > 1 and k > 1:
        assert np.isposinf(Z[40, 1]) and np.isneginf(Z[41, 1]) and assign[40] == 1 and np.isposinf(score[40]) and assign[41] != 1
    if dim > 1 and k >= 6:
        assert np.all(Z[20:30, 4] == 0) and np.all(Z[20:30, 5] == 0) and not (assign[20:30] == 5).any()


def test_signed_zero_tie(bn):
    """a row orthogonal to c and -c, every other score negative: the pair ties at +-0 and the lower index wins, in either order"""
    X = np.zeros((70, 4), dtype=np.float32)
    X[:, 1] = 1.0
    X[:, 2] = np.arange(70) * 0.01
    idx = bn.Index(0, 4, 70)
    idx.add(X)
    c = np.array([[1.5, 0, 0, 0], [-1.5, 0, 0, 0], [0, -1, 0, 0]], dtype=np.float32)
    for cent in (c, c[[1, 0, 2]], c[[2, 1, 0]]):
        assign, score = idx.assign(cent)
        assert_exact_assignment(bn, idx, cent, assign, score)
        assert np.all(score == 0) and np.all(assign == (1 if cent[0, 1] else 0))


# ---- 2. position independence ---------------------------------------------------------------------------------------
def test_position_independence(bn):
    dim, k = 130, 130
    idx, X, S, valid = _rows(dim)
    cent = _centroids(dim, k)
    assign, score = idx.assign(cent)
    # reversed centroid order: the same scores, and ties go to the new lowest index
    ra, rs = idx.assign(cent[::-1])
    assert_exact_assignment(bn, idx, cent[::-1], ra, rs, what="reversed")
    assert rs.tobytes() == score.tobytes()
    moved = (k - 1 - ra.astype(np.int64))[valid] != assign[valid]
    assert moved.any() and np.all(np.isin(assign[valid][moved], [0, 1, 3]))  # only rows whose winner has a duplicate change
    # a sub-range that is not tile-aligned
    sa, ss = idx.assign(cent, first_id=37, n_ids=500)
    assert np.array_equal(sa, assign[37:537]) and ss.tobytes() == score[37:537].tobytes()
    ta, ts = idx.assign(cent, first_id=900)
    assert np.array_equal(ta, assign[900:]) and ts.tobytes() == score[900:].tobytes()
    # the same rows appended in three blocks, into a larger index
    other = bn.Index(0, dim, 5000)
    for a, b in ((0, 1), (1, 650), (650, 1000)):
        other.add(X[a:b])
    oa, osc = other.assign(cent)
    assert np.array_equal(oa, assign) and osc.tobytes() == score.tobytes()
    # an empty range writes nothing
    ea, es = idx.assign(cent, first_id=1000)
    assert len(ea) == 0 and len(es) == 0


# ---- 3. many tiles per workgroup ------------------------------------------------------------------------------------
def test_many_tiles_per_workgroup(bn):
    cus = exact.require_many_tiles(exact.N)
    tpw, n_wg = exact.tiles_per_workgroup(exact.N, cus)
    assert tpw >= 4
    rng = np.random.default_rng(12)
    dim, k = 8, 65
    pool = rng.standard_normal((300, dim)).astype(np.float32)
    X = pool[rng.integers(0, 300, exact.N)]
    X[[0, 63, 64, tpw * 64 - 1, tpw * 64, exact.N - 1]] = 0.0
    idx = bn.Index(0, dim, exact.N)
    idx.add(X)
    cent = rng.standard_normal((k, dim)).astype(np.float32)
    cent[64] = cent[5]
    assign, score = idx.assign(cent)
    assert_exact_assignment(bn, idx, cent, assign, score)
    print(f"{exact.N} rows, {n_wg} workgroups x {tpw} tiles")


# ---- 4 - 6. the update, chaining, convergence -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _blobs():
    """overlapping blobs: 1203 rows (three of them invalid) around 6 centres in 40 dimensions, sigma large enough that Lloyd moves"""
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    rng = np.random.default_rng(21)
    dim, k, n = 40, 6, 1203
    centres = rng.standard_normal((k, dim))
    centres /= np.sqrt((centres ** 2).sum(axis=1, keepdims=True))
    label = rng.integers(0, k, n)
    X = (centres[label] + 0.25 * rng.standard_normal((n, dim))).astype(np.float32)
    X[[5, 600, 1202]] = 0.0
    idx = bn.Index(0, dim, n)
    idx.add(X)
    S, valid = stored_rows(idx)
    init = np.flatnonzero(valid)[[0, 100, 200, 300, 400, 500]].astype(np.uint64)
    return idx, S, valid, init, k


def assert_update_within_bound(S, assign, prev, got, what):
    k = len(prev)
    want, kept = cluster_ref.update(S, assign, prev)
    c64, bound = cluster_ref.update_bound(S, assign, k)
    live = ~kept
    err = np.abs(got[live].astype(np.float64) - c64[live])
    worst = float((err / bound[live]).max()) if live.any() else 0.0
    print(f"{what}: worst |c - c64| / bound = {worst:.4f}")
    assert np.all(err <= bound[live]), what
    assert got[kept].tobytes() == prev[kept].tobytes(), what
    return kept


def test_one_update(bn):
    idx, S, valid, init, k = _blobs()
    cent, assign, score, counts, rep = idx.cluster(k, max_iters=1, init_ids=init)
    assert rep["iters"] == 1 and np.array_equal(rep["start_ids"], init)
    c0 = S[init.astype(np.int64)]
    a0, s0 = idx.assign(c0)
    assert_exact_assignment(bn, idx, c0, a0, s0, what="init assignment")
    kept = assert_update_within_bound(S, a0, c0, cent, "one update")
    assert not kept.any() and rep["empty_clusters"] == 0
    assert_exact_assignment(bn, idx, cent, assign, score, what="returned assignment")
    assert (assign != a0).any() and rep["moved_last"] == int((assign != a0).sum()), "the first assignment was already the last"
    assert np.array_equal(counts, np.bincount(assign[assign != NONE], minlength=k))


def test_chaining_and_determinism(bn):
    idx, S, valid, init, k = _blobs()
    one = idx.cluster(k, max_iters=3, init_ids=init, history=8)
    two = idx.cluster(k, max_iters=3, init_ids=init, history=8)
    for x, y in zip(one[:4], two[:4]):
        assert x.tobytes() == y.tobytes()
    assert one[4]["objective"] == two[4]["objective"] and one[4]["objective_history"].tobytes() == two[4]["objective_history"].tobytes()
    assert one[4]["iters"] == 3 and len(one[4]["objective_history"]) == 4
    step = idx.cluster(k, max_iters=1, init_ids=init)
    for _ in range(2):
        step = idx.cluster(k, max_iters=1, init_centroids=step[0])
    for x, y in zip(one[:4], step[:4]):
        assert x.tobytes() == y.tobytes()
    assert step[4]["start_ids"] is None
    # a sub-range clusters the sub-range's rows alone
    sub = idx.cluster(k, first_id=100, n_ids=700, max_iters=2, init_ids=init[1:].tolist() + [150])
    assert len(sub[1]) == 700 and sub[3].sum() == valid[100:800].sum()
    a, s = idx.assign(sub[0], first_id=100, n_ids=700)
    assert np.array_equal(a, sub[1]) and s.tobytes() == sub[2].tobytes()


def test_convergence_properties(bn):
    idx, S, valid, init, k = _blobs()
    cent, assign, score, counts, rep = idx.cluster(k, max_iters=50, init_ids=init, history=64)
    assert rep["converged"] and rep["moved_last"] == 0 and 1 < rep["iters"] < 50
    assert_exact_assignment(bn, idx, cent, assign, score)
    assert_update_within_bound(S, assign, cent, cent, "converged")
    assert np.array_equal(counts, np.bincount(assign[assign != NONE], minlength=k)) and counts.sum() == valid.sum()
    want = np.cumsum(score[assign != NONE].astype(np.float64))[-1]  # cumsum adds in id order
    assert rep["objective"] == want
    h = rep["objective_history"]
    assert len(h) == rep["iters"] + 1 and h[-1] == rep["objective"]
    steps = np.diff(h)
    print(f"{rep['iters']} updates, smallest objective step {steps.min():.3e}")
    assert np.all(steps >= -len(S) * S.shape[1] * 2.0 ** -23)


# ---- 7. planted clusters, the built-in start ------------------------------------------------------------------------
def replay_max_min(bn, S, valid, k):
    """the max-min rule on the twin head's scores"""
    chosen = [int(np.flatnonzero(valid)[0])]
    best = None
    while len(chosen) < k:
        s = twin_scores(bn, S[chosen[-1]][None], S)[:, 0]
        best = s if best is None else np.where(s > best, s, best)
        masked = np.where(valid, best, np.inf).astype(np.float64)
        masked[chosen] = np.inf
        chosen.append(int(np.argmin(masked)))  # the first minimum: ties by lowest id
    return np.array(chosen, dtype=np.uint64)


@pytest.mark.parametrize("dim,k,per,sigma", [(32, 5, 60, 0.05), (130, 7, 40, 0.03), (1536, 64, 16, 0.01), (1536, 70, 15, 0.01)])
def test_planted_clusters_with_the_built_in_start(bn, dim, k, per, sigma):
    rng = np.random.default_rng([dim, k])
    centres = rng.standard_normal((k, dim))
    centres /= np.sqrt((centres ** 2).sum(axis=1, keepdims=True))
    label = rng.permutation(np.repeat(np.arange(k), per))
    X = (centres[label] + sigma * rng.standard_normal((k * per, dim))).astype(np.float32)
    X64 = X.astype(np.float64)
    X64 /= np.sqrt((X64 ** 2).sum(axis=1, keepdims=True))
    cos = X64 @ X64.T
    same = label[:, None] == label[None, :]
    within, cross = cos[same].min(), cos[~same].max()
    print(f"within >= {within:.3f}, cross <= {cross:.3f}")
    # the precondition, in float64: with it max-min picks one row per planted cluster and the first assignment is the partition
    assert within > cross, "the planted clusters are not separated"
    idx = bn.Index(0, dim, len(X))
    idx.add(X)
    S, valid = stored_rows(idx)
    cent, assign, score, counts, rep = idx.cluster(k)
    assert rep["converged"] and rep["empty_clusters"] == 0
    # the partition is the planted one up to relabelling
    pairs = set(zip(assign.tolist(), label.tolist()))
    assert len(pairs) == k and len({p[0] for p in pairs}) == k and len({p[1] for p in pairs}) == k
    assert np.all(counts == per)
    start = rep["start_ids"]
    assert np.array_equal(start, replay_max_min(bn, S, valid, k))
    assert len(set(label[start.astype(np.int64)].tolist())) == k  # one row per planted cluster
    assert_exact_assignment(bn, idx, cent, assign, score)


# ---- 8. the empty cluster -------------------------------------------------------------------------------------------
def test_empty_cluster_keeps_its_centroid(bn):
    idx, S, valid, init, k = _blobs()
    c0 = S[init[:3].astype(np.int64)].copy()
    c0[2] = c0[0]
    a0, _ = idx.assign(c0)
    assert not (a0 == 2).any()  # the tie goes to index 0: the second copy has no members
    cent, assign, score, counts, rep = idx.cluster(3, max_iters=1, init_centroids=c0)
    assert cent[2].tobytes() == c0[2].tobytes() and cent[0].tobytes() != c0[0].tobytes()
    assert rep["empty_clusters"] >= 1 and rep["iters"] == 1
    assert_exact_assignment(bn, idx, cent, assign, score)
    assert np.array_equal(counts, np.bincount(assign[assign != NONE], minlength=3))


# ---- 9. refusals ----------------------------------------------------------------------------------------------------
SENT_U32, SENT_F32 = 0xCDCDCDCD, np.float32(123.25)


def raw_assign(bn, x, cent, k, first_id, n_ids, n_out, null=()):
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    a = np.full(n_out, SENT_U32, dtype=np.uint32)
    s = np.full(n_out, SENT_F32, dtype=np.float32)
    st = bn.lib.bn_index_assign(x, None if "cent" in null else cent.ctypes.data_as(f32p), k, first_id, n_ids,
                                None if "assign" in null else a.ctypes.data_as(u32p), s.ctypes.data_as(f32p))
    return st, (a, s)


def raw_cluster(bn, x, k, dim, first_id, n_ids, n_out, init_ids=None, init_centroids=None, null=()):
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    cent = np.full(max(k, 1) * dim, SENT_F32, dtype=np.float32)
    a = np.full(n_out, SENT_U32, dtype=np.uint32)
    s = np.full(n_out, SENT_F32, dtype=np.float32)
    counts = np.full(max(k, 1), SENT_U32, dtype=np.uint32)
    start = np.full(max(k, 1), 0xABABABABABABABAB, dtype=np.uint64)
    ids = None if init_ids is None else np.ascontiguousarray(init_ids, dtype=np.uint64)
    ic = None if init_centroids is None else np.ascontiguousarray(init_centroids, dtype=np.float32)
    o = bn.BnClusterOpts(2, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint64)), None if ic is None else ic.ctypes.data_as(f32p),
                         start.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0)
    rep = bn.BnClusterReport(11, 12, 13, 14, 15.5, 16)
    before = bytes(rep)
    st = bn.lib.bn_index_cluster(x, k, first_id, n_ids, C.byref(o), C.sizeof(o), None if "cent" in null else cent.ctypes.data_as(f32p),
                                 None if "assign" in null else a.ctypes.data_as(u32p), s.ctypes.data_as(f32p),
                                 None if "counts" in null else counts.ctypes.data_as(u32p), C.byref(rep), C.sizeof(rep))
    return st, (cent, a, s, counts, start), bytes(rep) == before


def untouched(arrays):
    return all(np.all(x == (SENT_F32 if x.dtype == np.float32 else 0xABABABABABABABAB if x.dtype == np.uint64 else SENT_U32)) for x in arrays)


def test_refusals(bn):
    idx, S, valid, init, k = _blobs()
    n, dim, x = len(idx), S.shape[1], idx._h
    q = S[[3, 500, 998]]
    before = idx.search(q, 20)
    good = S[init.astype(np.int64)].copy()
    nan_c, inf_c = good.copy(), good.copy()
    nan_c[2, 7] = np.nan
    inf_c[5, 0] = -np.inf
    big = np.zeros((1025, dim), dtype=np.float32)
    bad_assign = [
        dict(x=None), dict(null=("cent",)), dict(null=("assign",)),
        dict(k=0), dict(k=1025, cent=big),
        dict(first_id=n + 1), dict(first_id=n - 5, n_ids=6), dict(first_id=0, n_ids=n + 1), dict(first_id=1, n_ids=2 ** 64 - 1),
        dict(cent=nan_c), dict(cent=inf_c),
    ]
    for i, kw in enumerate(bad_assign):
        a = dict(dict(x=x, cent=good, k=k, first_id=0, n_ids=0, null=()), **kw)
        st, outs = raw_assign(bn, a["x"], a["cent"], a["k"], a["first_id"], a["n_ids"], n, a["null"])
        assert st == 1 and bn.last_error(), ("assign", i, kw)
        assert untouched(outs) and len(idx) == n, ("assign", i, kw)
    few = np.flatnonzero(valid)[:3].astype(np.uint64)
    bad_cluster = [
        dict(x=None), dict(null=("cent",)), dict(null=("assign",)), dict(null=("counts",)),
        dict(k=0), dict(k=1025),
        dict(first_id=n + 1), dict(first_id=n - 5, n_ids=6), dict(first_id=0, n_ids=n + 1),
        dict(init_centroids=nan_c), dict(init_centroids=inf_c),
        dict(init_ids=list(init[:5]) + [n]), dict(init_ids=list(init[:5]) + [2 ** 40]),      # out of the index
        dict(first_id=100, n_ids=1000, init_ids=list(init[1:]) + [99]),                      # out of the range
        dict(first_id=0, n_ids=int(init[5]), init_ids=init),                                 # the last one just past the range
        dict(init_ids=list(init[:5]) + [5]),                                                 # an invalid row
        dict(init_ids=list(init[:5]) + [int(init[2])]),                                      # a duplicate
        dict(init_ids=init, init_centroids=good),                                            # both
        dict(first_id=0, n_ids=5), dict(first_id=n, n_ids=0), dict(first_id=5, n_ids=1, k=1),  # fewer valid rows than k
        dict(k=1000),
    ]
    assert valid[:5].all() and not valid[5]
    for i, kw in enumerate(bad_cluster):
        a = dict(dict(x=x, k=k, first_id=0, n_ids=0, init_ids=None, init_centroids=None, null=()), **kw)
        if a["k"] == 1000:  # 1200 valid rows, but only 998 in this range
            a.update(first_id=0, n_ids=1000)
        st, outs, rep_same = raw_cluster(bn, a["x"], a["k"], dim, a["first_id"], a["n_ids"], n, a["init_ids"], a["init_centroids"], a["null"])
        assert st == 1 and bn.last_error(), ("cluster", i, kw)
        assert untouched(outs) and rep_same and len(idx) == n, ("cluster", i, kw)
    after = idx.search(q, 20)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(before, after))
    st, outs, _ = raw_cluster(bn, x, 3, dim, 0, 0, n, init_ids=few)  # and a valid call still works
    assert st == 0 and not untouched(outs[:1])


# ---- 10. nothing else moved; the loop on a network-filled index -----------------------------------------------------
def test_nothing_else_moves(bn):
    idx, S, valid, init, k = _blobs()
    head = bn.Head(0, np.random.default_rng(3).standard_normal((3, S.shape[1])).astype(np.float32), None, l2norm=True)
    q = S[[3, 500, 998]]
    before = idx.search(q, 20), head.rank_index(idx, 30, "top"), idx.read().tobytes(), len(idx)
    idx.cluster(k, max_iters=3)
    idx.assign(S[:70])
    after = idx.search(q, 20), head.rank_index(idx, 30, "top"), idx.read().tobytes(), len(idx)
    for b, a in zip(before[:2], after[:2]):
        assert all(u.tobytes() == v.tobytes() for u, v in zip(b, a))
    assert before[2:] == after[2:]


def test_cluster_then_search_on_a_network_filled_index(bn):
    m = bn.Model(write_model(synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)))
    cfg = m.config
    n_samp, sr, B = int(cfg.sample_count), int(cfg.sample_rate), 4
    rng = np.random.default_rng(8)
    pcm = synth.synthetic_segments(1, n_samp * 3 * B, sr)[0]
    pcm = np.clip(pcm + 0.05 * rng.standard_normal(len(pcm)), -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    ctx = bn.Context(m, B)
    idx = bn.Index(0, int(cfg.embedding_dim), 3 * B)
    for f in range(0, 3 * B, B):
        ctx.infer_windows(rec, n_samp, f, B)
        assert idx.add_context(ctx, B) == f
    cent, assign, score, counts, rep = idx.cluster(3, max_iters=5)  # the call waits for the pending append itself
    assert len(idx) == 3 * B and counts.sum() == 3 * B and not (assign == NONE).any()
    assert_exact_assignment(bn, idx, cent, assign, score)
    # the row nearest each centroid is the seed of a search: it finds itself at cosine 1
    for c in np.flatnonzero(counts):
        members = np.flatnonzero(assign == c)
        exemplar = int(members[np.argmax(score[members])])
        ids, sc, cnt = idx.search_ids([exemplar], 3 * B, exclude_radius=-1)
        hit = np.flatnonzero(ids[0, :cnt[0]] == exemplar)
        assert len(hit) == 1 and sc[0, hit[0]] >= 1 - 1e-6
