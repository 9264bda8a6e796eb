"""The embedding index (bn_index_*) against a float64 numpy brute force computed here: exact top-M cosine search, its total
order (score descending, ties by id ascending), bit-identity across call structure, masking of invalid / excluded rows, the
refusals of the ABI, and appends straight from a context's embedding output."""
import importlib

import numpy as np
import pytest

from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")

SCORE_TOL = 1e-5  # |returned score - float64 cosine|
SWAP_TOL = 2e-5   # rows this close to the M-th float64 score may trade places


def cosine64(queries, rows):
    """float64 cosine [Q, N]; rows / queries with zero norm or a non-finite element -> NaN (never eligible)"""
    def unit(a):
        a = np.asarray(a, dtype=np.float64)
        with np.errstate(all="ignore"):
            n = np.sqrt((a * a).sum(axis=1, keepdims=True))
            u = a / n
        bad = ~np.isfinite(a).all(axis=1) | (n[:, 0] == 0) | ~np.isfinite(n[:, 0])
        u[bad] = np.nan
        return u
    with np.errstate(all="ignore"):
        return unit(queries) @ unit(rows).T


def check_top_m(ids, scores, counts, ref, M, excluded=None):
    Q, N = ref.shape
    for q in range(Q):
        r = ref[q].copy()
        if excluded is not None:
            r[excluded[q]] = np.nan
        elig = np.isfinite(r)
        c = int(min(M, elig.sum()))
        assert counts[q] == c, (q, counts[q], c)
        got_i, got_s = ids[q, :c].astype(np.int64), scores[q, :c]
        assert len(set(got_i.tolist())) == c
        assert elig[got_i].all(), "an ineligible row was returned"
        assert np.all(np.abs(got_s.astype(np.float64) - r[got_i]) <= SCORE_TOL), np.abs(got_s - r[got_i]).max()
        assert np.all(np.diff(got_s) <= 0), "scores not non-increasing"
        ties = np.diff(got_s) == 0
        assert np.all(np.diff(got_i)[ties] > 0), "equal scores not in ascending id order"
        if c == 0:
            continue
        key = np.where(elig, r, -np.inf)
        order = np.lexsort((np.arange(N), -key))
        want = order[:c]
        mth = key[order[c - 1]]
        for i in set(got_i.tolist()) ^ set(want.tolist()):
            assert abs(r[i] - mth) <= SWAP_TOL, (q, i, r[i], mth)


def rows_and_queries(rng, n, dim, nq):
    X = rng.standard_normal((n, dim), dtype=np.float32)
    # half the queries near stored rows (a meaningful neighbourhood), half random directions
    near = X[rng.integers(0, n, nq // 2 + nq % 2)] + 0.3 * rng.standard_normal((nq // 2 + nq % 2, dim), dtype=np.float32)
    Qs = np.concatenate([near, rng.standard_normal((nq // 2, dim), dtype=np.float32)]).astype(np.float32)
    return X, Qs


@pytest.mark.parametrize("dim", [37, 192, 1024, 1536])
def test_exact_top_m_against_float64(bn, dim):
    rng = np.random.default_rng(dim)
    N = 10007
    X, Qall = rows_and_queries(rng, N, dim, 70)
    idx = bn.Index(0, dim, N)
    assert idx.add(X) == 0 and len(idx) == N
    ref = cosine64(Qall, X)
    for Q in (1, 5, 32, 33, 70):
        for M in (1, 10, 100, 256):
            ids, scores, counts = idx.search(Qall[:Q], M)
            check_top_m(ids, scores, counts, ref[:Q], M)


def test_ties_and_total_order(bn):
    rng = np.random.default_rng(7)
    dim, N = 64, 200
    X = rng.standard_normal((N, dim), dtype=np.float32)
    for d in (5, 77, 150):
        X[d] = X[10]                 # identical bits
    q = X[10].copy()
    X[199] = -q                      # scores -1: last when M = N
    idx = bn.Index(0, dim, N)
    idx.add(X)
    ids, scores, counts = idx.search(q[None], 4)
    assert counts[0] == 4 and list(ids[0]) == [5, 10, 77, 150]
    assert scores[0].tobytes() == np.repeat(scores[0, :1], 4).tobytes()
    ids, scores, counts = idx.search(q[None], N)
    assert counts[0] == N and ids[0, -1] == 199 and abs(scores[0, -1] + 1) <= 1e-6
    check_top_m(ids, scores, counts, cosine64(q[None], X), N)
    # -0.0 and +0.0 are one score: rows orthogonal to the query tie and come back by id
    Z = np.zeros((6, 4), dtype=np.float32)
    Z[:, 1] = [1, -1, 2, -2, 3, -3]
    idx2 = bn.Index(0, 4, 8)
    idx2.add(Z)
    ids, scores, counts = idx2.search(np.array([[1, 0, 0, 0]], dtype=np.float32), 6)
    assert counts[0] == 6 and list(ids[0]) == [0, 1, 2, 3, 4, 5] and np.all(scores[0] == 0)


def test_bit_identity_across_call_structure(bn):
    rng = np.random.default_rng(11)
    dim, N, Q, M = 192, 10007, 33, 100
    X, Qs = rows_and_queries(rng, N, dim, Q)
    one = bn.Index(0, dim, N)
    one.add(X)
    parts = bn.Index(0, dim, N)
    cuts = np.sort(rng.choice(np.arange(1, N), 16, replace=False))
    for a, b in zip(np.r_[0, cuts], np.r_[cuts, N]):
        assert parts.add(X[a:b]) == a
    assert len(parts) == N and one.read().tobytes() == parts.read().tobytes()
    r1 = one.search(Qs, M)
    r2 = parts.search(Qs, M)
    r3 = one.search(Qs, M)
    for a, b, c in zip(r1, r2, r3):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    for q in range(Q):
        single = one.search(Qs[q:q + 1], M)
        for a, b in zip(r1, single):
            assert a[q:q + 1].tobytes() == b.tobytes(), q
    check_top_m(*r1, cosine64(Qs, X), M)


def test_masking_and_edges(bn):
    rng = np.random.default_rng(5)
    dim, N = 96, 300
    X = rng.standard_normal((N, dim), dtype=np.float32)
    bad = [0, 17, 18, 150, 299]
    X[0] = 0
    X[17, 3] = np.nan
    X[18, 40] = np.inf
    X[150, 0] = -np.inf
    X[299] = 0
    idx = bn.Index(0, dim, N + 10)
    empty = bn.Index(0, dim, 4)
    _, _, c = empty.search(X[1:3], 5)
    assert list(c) == [0, 0]
    idx.add(X)
    Qs = np.concatenate([X[[1, 17, 0]], rng.standard_normal((3, dim), dtype=np.float32)])
    Qs[4] = 0                                  # zero query
    Qs[5, 7] = np.nan                          # non-finite query
    ids, scores, counts = idx.search(Qs, 256)
    assert counts[1] == counts[2] == counts[4] == counts[5] == 0
    assert counts[0] == counts[3] == 256
    ids, scores, counts = idx.search(Qs[[0, 3]], 256)
    assert not set(bad) & set(ids[:, :256].ravel().tolist())
    # top_m > eligible rows: every eligible row, nothing else
    small = bn.Index(0, dim, 20)
    small.add(X[:20])                          # rows 0, 17, 18 invalid
    ids, scores, counts = small.search(X[1:2], 256)
    assert counts[0] == 17 and set(ids[0, :17].tolist()) == set(range(20)) - {0, 17, 18}
    check_top_m(ids, scores, counts, cosine64(X[1:2], X[:20]), 256)
    stored = small.read()
    assert np.all(stored[[0, 17, 18]] == 0) and np.isfinite(stored).all()
    # refusals
    for top_m, stride in ((0, 1), (257, 257), (10, 9)):
        with pytest.raises(bn.EngineError) as e:
            idx.search(Qs[:1], top_m, m_stride=stride)
        assert e.value.status == 1
    with pytest.raises(bn.EngineError) as e:
        idx.search_ids([N], 5)                 # not an id of the index
    assert e.value.status == 1
    with pytest.raises(bn.EngineError) as e:
        idx.add(X[:11])                        # 300 + 11 > 310: refused whole
    assert e.value.status == 1 and len(idx) == N
    assert idx.add(X[:10]) == N and len(idx) == N + 10


def _network_case(bn, data, batch=4):
    path = write_model(data)
    m = bn.Model(path)
    cfg = m.config
    S, sr = int(cfg.sample_count), int(cfg.sample_rate)
    step = S - sr                              # 1 s overlap
    n_win = 3 * batch + 2                      # 4 batches, the last one ragged
    pcm = np.clip(synth.synthetic_segments(1, S + step * (n_win - 1) - 123, sr)[0], -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    G = rec.n_windows(step)
    assert G >= 3 * batch
    ctx = bn.Context(m, batch)
    idx = bn.Index(0, int(cfg.embedding_dim), G + 8)
    embs = []
    for f in range(0, G, batch):
        n = min(batch, G - f)
        _, emb = ctx.infer_windows(rec, step, f, n)
        embs.append(emb)
        assert idx.add_context(ctx, n) == f
    emb = np.concatenate(embs)
    assert len(idx) == G
    return m, ctx, idx, emb, G


@pytest.mark.parametrize("family", ["v30", "perch"])
def test_appends_from_the_network(bn, family):
    data = (synth.birdnet_v30(num_species=300, width=0.5, depth=0.34, emb=1024) if family == "v30"
            else synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192))
    m, ctx, idx, emb, G = _network_case(bn, data)
    e64 = emb.astype(np.float64)
    want = e64 / np.sqrt((e64 * e64).sum(axis=1, keepdims=True))
    got = idx.read()
    assert got.shape == emb.shape and np.abs(got - want).max() <= 1e-6
    ids = np.arange(G)
    M = G  # every window: the synthetic recording's windows may all lie within 1e-6 of each other
    out_i, out_s, cnt = idx.search_ids(ids, M, exclude_radius=-1)
    assert np.all(cnt == G)
    cos = cosine64(emb, emb)
    for q in range(G):
        pos = np.nonzero(out_i[q, :cnt[q]] == q)[0]
        assert len(pos) == 1, (q, out_i[q])
        own = out_s[q, pos[0]]
        assert own >= 1 - 1e-6
        # rows ranked ahead of the window itself: equal score within 1e-6, or rows that are themselves duplicates of the window
        # to within 1e-6 in float64 (the synthetic network maps neighbouring windows almost onto one direction; among such
        # rows f32 rounding of a 1024-term dot product decides the order)
        ahead_ids = out_i[q, :pos[0]].astype(np.int64)
        assert np.all((np.abs(out_s[q, :pos[0]] - own) <= 1e-6) | (cos[q, ahead_ids] >= 1 - 1e-6)), (q, out_s[q], cos[q, ahead_ids])
    check_top_m(out_i, out_s, cnt, cos, M)
    out_i, out_s, cnt = idx.search_ids(ids, M, exclude_radius=1)
    excl = [np.arange(max(0, q - 1), min(G, q + 2)) for q in range(G)]
    for q in range(G):
        assert np.all(np.abs(out_i[q, :cnt[q]].astype(np.int64) - q) > 1), (q, out_i[q])
    check_top_m(out_i, out_s, cnt, cos, M, excluded=excl)
    # host queries find the same neighbourhoods
    h_i, h_s, h_c = idx.search(emb[:5], M)
    check_top_m(h_i, h_s, h_c, cosine64(emb[:5], emb), M)


def test_add_context_refusals(bn):
    v24 = bn.Model(write_model(synth.birdnet_v24(num_species=64, width=0.25, depth=0.25, head=64)))
    perch_data = synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)
    m, ctx, idx, emb, G = _network_case(bn, perch_data)
    before = idx.read()
    last = G - (G - 1) // 4 * 4                # rows of the last run
    cfg = v24.config
    rec = bn.Recording(np.zeros(int(cfg.sample_count) * 2, dtype=np.float32))
    vctx = bn.Context(v24, 2)
    vctx.infer_windows(rec, int(cfg.sample_count), 0, 2)
    wrong_dim = bn.Index(0, 1024, 16)
    for call in (lambda: idx.add_context(vctx, 1),          # model without embeddings
                 lambda: wrong_dim.add_context(ctx, 1),     # 192-d embeddings, 1024-d index
                 lambda: idx.add_context(ctx, last + 1)):   # more rows than the last run had
        with pytest.raises(bn.EngineError) as e:
            call()
        assert e.value.status == 1
    assert len(idx) == G and len(wrong_dim) == 0 and idx.read().tobytes() == before.tobytes()
    assert idx.add_context(ctx, last) == G and len(idx) == G + last


def test_scale_300k_rows_1536(bn):
    rng = np.random.default_rng(2026)
    dim, N, Q, M, chunk = 1536, 300_000, 64, 100, 25_000
    idx = bn.Index(0, dim, N)
    ref = np.empty((Q, N))
    Qs = None
    for a in range(0, N, chunk):
        X = rng.standard_normal((chunk, dim), dtype=np.float32)
        if Qs is None:
            Qs = (X[:Q] + 0.5 * rng.standard_normal((Q, dim), dtype=np.float32)).astype(np.float32)
            Qs[Q // 2:] = rng.standard_normal((Q - Q // 2, dim), dtype=np.float32)
        assert idx.add(X) == a
        ref[:, a:a + chunk] = cosine64(Qs, X)
    ids, scores, counts = idx.search(Qs, M)
    check_top_m(ids, scores, counts, ref, M)
