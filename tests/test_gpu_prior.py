"""Per-site species priors on the GPU (bn_prior_*): every result compared bit for bit (tobytes) with tests/prior_ref.py, through
bn_prior_apply_host unless noted.

Widths: every row length at which the select kernel takes another path (below one 16-byte group, around one wave, rows that are no
multiple of 4 and so start at other alignments, the flagship 6522, 14795 near the LDS form's limit, 16389 beyond it), both kernel forms
(BN_PRIOR_GENERAL), K in {1, 2, 10, min(n, 1024)}, both orders x rerank x minimum.  Ties, edges, independence of batch and position,
the three step entry points, lifetime, refusals, and the host mirror."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle
import prior_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
SITES = (2, 0, 2, 1, 0)  # row -> site: neither sorted nor a permutation
THR = 0.3
_CASES = {}


def _width_case(n):
    """5 rows of n logits with ties, 3 sites; the sigmoids computed once per width."""
    if n not in _CASES:
        rng = np.random.default_rng(n)
        x = (rng.standard_normal((5, n)) * 3).astype(np.float32)
        x[1] = np.round(x[1] * 2) / 2           # a row of heavy ties
        x[3, : n // 2] = x[3, n // 2: 2 * (n // 2)]  # every value twice
        table = rng.uniform(0, 1, (3, n)).astype(np.float32)
        table[rng.uniform(size=(3, n)) < 0.2] = prior_ref.UNKNOWN
        _CASES[n] = (x, table, prior_ref.sigmoid_row(x).reshape(5, n))
    return _CASES[n]


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("idx", "conf", "count")):
        assert g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g, w)


@pytest.mark.parametrize("general", [False, True])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 6522, 14795, 16389])
def test_widths_orders_and_both_kernel_forms(bn, monkeypatch, n, general):
    if general:
        monkeypatch.setenv("BN_PRIOR_GENERAL", "1")
    x, table, conf = _width_case(n)
    for after in (False, True):
        for rerank in (False, True):
            if after and general:
                continue  # the switch concerns the select kernel only
            prior = bn.Prior(0, table, THR, after_topk=after, rerank=rerank)
            assert (prior.n_sites, prior.n_species, prior.flags) == (3, n, (1 if after else 0) | (2 if rerank else 0))
            assert prior.threshold == np.float32(THR)
            for k in sorted({1, min(2, n), min(10, n), min(n, 1024)}):
                for min_conf in (None, 0.2):
                    got = prior.apply(x, SITES, k, min_conf)
                    want = prior_ref.apply(x, table, SITES, THR, k, min_conf, after, rerank, conf)
                    _same(got, want, (n, after, rerank, k, min_conf))
    assert prior.read().tobytes() == table.tobytes() and prior.read(1, 1).tobytes() == table[1:2].tobytes()


def test_ties(bn):
    n = 300
    table = np.full((2, n), 0.5, dtype=np.float32)
    table[1] = prior_ref.UNKNOWN
    x = np.zeros((4, n), dtype=np.float32)
    x[0] = 0.75                                   # all equal logits, all equal priors: by index alone
    x[1] = np.linspace(-3, 3, n, dtype=np.float32)
    x[1, 100:170] = 1.0                            # 70 equal keys (more than one wave) straddling the K-th place
    k1 = int((x[1] > 1.0).sum()) + 35
    x[2] = np.linspace(-2, 2, n, dtype=np.float32)
    x[2, 7], x[2, 200] = 20.0, 20.5                # distinct logits, the same f32 sigmoid
    assert oracle.sigmoid(20.0) == oracle.sigmoid(20.5) == 1.0
    x[3] = x[1][::-1]
    for rerank in (False, True):
        prior = bn.Prior(0, table, THR, rerank=rerank)
        for k in (1, 5, 64, 65, k1, n):
            for sites in ((0, 0, 0, 0), (1, 0, 1, 0)):
                _same(prior.apply(x, sites, k), prior_ref.apply(x, table, sites, THR, k, None, False, rerank), (rerank, k, sites))
    i, c, m = bn.Prior(0, table, THR).apply(x, (0, 0, 0, 0), 10)
    assert list(i[0]) == list(range(10)) and list(i[2][:2]) == [7, 200] and m.tolist() == [10] * 4


def test_edges(bn):
    n = 60  # at most 64 survivors: beyond that the step's own top-K, which AFTER_TOPK filters, leaves the order of NaN confidences open
    rng = np.random.default_rng(5)
    table = rng.uniform(0.31, 1, (5, n)).astype(np.float32)
    table[0] = 0.1                                 # site 0 admits nothing
    table[1] = 0.1
    table[1, [3, 40, 59]] = [0.9, 0.5, 0.31]       # site 1 admits fewer than K
    table[2] = prior_ref.UNKNOWN                   # all unknown
    table[3, 10] = np.float32(THR)                 # p == threshold exactly: admitted
    table[3, 11] = np.nextafter(np.float32(THR), np.float32(0))
    table[3, 12] = 0.0                             # below the threshold
    table[4, :8] = [0.0, -0.0, 0.0, 0.5, 0.0, 0.5, 0.5, 0.0]
    x = (rng.standard_normal((5, n)) * 2).astype(np.float32)
    x[3, 10:13] = 9.0
    x[4, :12] = [np.inf, -np.inf, 0.0, -0.0, np.nan, -np.nan, 1.0, 1.0, np.inf, -np.inf, np.nan, -np.nan]
    sites = (0, 1, 2, 3, 4)
    for thr in (THR, 0.0):
        for after in (False, True):
            for rerank in (False, True):
                prior = bn.Prior(0, table, thr, after_topk=after, rerank=rerank)
                conf4 = prior_ref.conf_prime(prior_ref.sigmoid_row(x[4]), table[4], rerank)
                for k in (1, 4, 10, n):
                    # p == 0 with rerank gives conf' == 0 and stays in order (thr 0); min_conf equal to one conf' exactly
                    for min_conf in (None, 0.0, float(conf4[6]), float(oracle.sigmoid(float(x[2, 5])))):
                        got = prior.apply(x, sites, k, min_conf)
                        _same(got, prior_ref.apply(x, table, sites, thr, k, min_conf, after, rerank), (thr, after, rerank, k, min_conf))
                        if thr == THR:
                            assert got[2][0] == 0 and got[2][1] <= 3
                            if min_conf is not None:
                                assert not np.isnan(got[1]).any()
    i, c, m = bn.Prior(0, table, THR).apply(x, sites, n)
    assert m[1] == 3 and m[2] == n and 10 in i[3][:m[3]] and 11 not in i[3][:m[3]] and 12 not in i[3][:m[3]]
    assert np.isnan(c[4][0]) and np.isnan(c[4][m[4] - 1])   # total_cmp: +NaN first, -NaN last


@pytest.mark.parametrize("general", [False, True])
def test_a_row_does_not_depend_on_batch_or_position(bn, monkeypatch, general):
    if general:
        monkeypatch.setenv("BN_PRIOR_GENERAL", "1")
    x, table, conf = _width_case(6522)
    for after in (False, True):
        prior = bn.Prior(0, table, THR, after_topk=after, rerank=True)
        alone = prior.apply(x[2:3], [1], 10, 0.05)
        batch = np.stack([x[2], x[0], x[1], x[3], x[2]])
        got = prior.apply(batch, [1, 0, 2, 1, 1], 10, 0.05)
        for g, a in zip(got, alone):
            assert g[0].tobytes() == a[0].tobytes() and g[4].tobytes() == a[0].tobytes()
        again = prior.apply(batch, [1, 0, 2, 1, 1], 10, 0.05)
        _same(got, again)
    big = np.tile(x, (300, 1))[:1100]              # more rows than one round of apply_host
    sites = np.arange(1100) % 3
    got = bn.Prior(0, table, THR).apply(big, sites, 3)
    _same([g[:5] for g in got], bn.Prior(0, table, THR).apply(big[:5], sites[:5], 3))
    _same([g[1095:] for g in got], bn.Prior(0, table, THR).apply(big[1095:], sites[1095:], 3))


# ---- step -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[16, 70])
def model(request, bn):
    return bn.Model(write_model(synth.birdnet_v24(num_species=request.param, width=0.25, depth=0.25, head=32)))


def _pcm(model, n_windows, seed=0):
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    x = synth.synthetic_segments(1, S * n_windows, sr)[0]
    rng = np.random.default_rng(seed)
    return np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32), S


def _table(n, n_sites, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0, 1, (n_sites, n)).astype(np.float32)
    t[rng.uniform(size=t.shape) < 0.2] = prior_ref.UNKNOWN
    return t


@pytest.mark.parametrize("after", [False, True])
def test_step_paths(bn, model, after):
    n, B = int(model.config.num_species), 6
    table = _table(n, 3, n)
    prior = bn.Prior(0, table, THR, after_topk=after, rerank=True)
    pcm, S = _pcm(model, 2 * B)
    rec = bn.Recording(pcm)
    plain, ctx = bn.Context(model, B), bn.Context(model, B)
    pk, pmin = 4, 0.05                             # the attachment's own K / minimum (SELECT); AFTER_TOPK takes the step's
    ctx.attach_prior(prior, top_k=pk, min_confidence=pmin)
    k_eff, min_eff = (5, 0.01) if after else (pk, pmin)

    def check(m, sites):
        got = ctx.step_results(m)
        pres = ctx.step_prior_results(m)
        assert pres[0].shape == (m, min(k_eff, n))
        _same(pres, prior.apply(got[0], sites, k_eff, min_eff))
        _same(pres, prior_ref.apply(got[0], table, sites, THR, k_eff, min_eff, after, True))
        return got, pres

    for site, (first, m) in ((0, (0, B)), (2, (B, B - 2))):
        ctx.set_prior_site(site)
        plain.step_windows(rec, S, first, m, 5, 0.01, sync=True)
        want = plain.step_results(m)
        ctx.step_windows(rec, S, first, m, 5, 0.01, sync=True)
        got, pres = check(m, [site] * m)
        for a, w in zip(got, want):
            assert a.tobytes() == w.tobytes()      # the step's own outputs: bit-identical to a context without a prior
        ctx.step_device(ctx.input_device()[0], m, 5, 0.01, sync=False)
        ctx.synchronize()
        for a, w in zip(ctx.step_results(m), want):
            assert a.tobytes() == w.tobytes()
        _same(ctx.step_prior_results(m), pres)
    # bn_step_live without a map: every row at the context's site
    live = bn.Live(0, 2, S, S, 4 * S, 1)
    live.push(0, pcm[:2 * S])
    live.push(1, pcm[2 * S:4 * S])
    src, win = ctx.step_live(live, B, 5, 0.01, sync=True)
    assert len(src) == 4
    check(4, [2] * 4)
    assert ctx.stats()["capture_fallbacks"] == 0 and plain.stats()["capture_fallbacks"] == 0 and ctx.stats()["replays"] > 0
    # detach restores the plain step
    ctx.attach_prior(None)
    ctx.step_windows(rec, S, 0, B, 5, 0.01, sync=True)
    plain.step_windows(rec, S, 0, B, 5, 0.01, sync=True)
    for a, w in zip(ctx.step_results(B), plain.step_results(B)):
        assert a.tobytes() == w.tobytes()
    with pytest.raises(bn.EngineError) as e:
        ctx.step_prior_results(B)
    assert e.value.status == 1


def test_live_rows_take_their_sources_sites_two_contexts_one_pool(bn, model):
    n = int(model.config.num_species)
    table = _table(n, 3, 7)
    prior = bn.Prior(0, table, THR)
    source_sites = [2, 0, 1, 2, 0, 1][::-1]       # 6 sources on 3 sites, non-monotone: (1, 0, 2, 1, 0, 2)
    n_src, n_win, B = 6, 3, 4
    S = int(model.config.sample_count)
    live = bn.Live(0, n_src, S, S, 2 * S * n_win, 1)
    for s in range(n_src):
        live.push(s, _pcm(model, n_win, seed=s)[0])
    ctxs = [bn.Context(model, B), bn.Context(model, B)]
    for c in ctxs:
        c.attach_prior(prior, source_sites=source_sites, top_k=3)
    seen = 0
    while True:
        taken = [c.step_live(live, B, 5, None, sync=False) for c in ctxs]  # both in flight on the one pool
        if not any(len(t[0]) for t in taken):
            break
        for c, (src, win) in zip(ctxs, taken):
            if not len(src):
                continue
            c.synchronize()
            m = len(src)
            sites = [source_sites[int(s)] for s in src]
            _same(c.step_prior_results(m), prior_ref.apply(c.step_results(m)[0], table, sites, THR, 3))
            seen += m
    assert seen == n_src * n_win and all(c.stats()["capture_fallbacks"] == 0 for c in ctxs)


def test_head_results_are_unchanged_by_a_prior(bn):
    model = bn.Model(write_model(synth.birdnet_v30(num_species=70, width=0.25, depth=0.25, emb=64)))
    dim, n, B = int(model.config.embedding_dim), int(model.config.num_species), 3
    rng = np.random.default_rng(3)
    head = bn.Head(0, rng.standard_normal((9, dim)).astype(np.float32), None)
    pcm, S = _pcm(model, B)
    rec = bn.Recording(pcm)
    a, b = bn.Context(model, B), bn.Context(model, B)
    a.attach_head(head, top_k=4)
    b.attach_head(head, top_k=4)
    table = _table(n, 2, 1)
    b.attach_prior(bn.Prior(0, table, THR, rerank=True), top_k=6)
    b.set_prior_site(1)
    a.step_windows(rec, S, 0, B, 5, None, sync=True)
    b.step_windows(rec, S, 0, B, 5, None, sync=True)
    for u, v in zip(a.step_head_results(B), b.step_head_results(B)):
        assert u.tobytes() == v.tobytes()
    for u, v in zip(a.step_results(B), b.step_results(B)):
        assert u.tobytes() == v.tobytes()
    _same(b.step_prior_results(B), prior_ref.apply(b.step_results(B)[0], table, [1] * B, THR, 6, None, False, True))


def test_lifetime_either_order_and_shared_prior(bn, model):
    n, B = int(model.config.num_species), 2
    table = _table(n, 2, 9)
    pcm, S = _pcm(model, B)
    rec = bn.Recording(pcm)
    prior = bn.Prior(0, table, THR)
    c1, c2 = bn.Context(model, B), bn.Context(model, B)
    c1.attach_prior(prior, top_k=3)
    c2.attach_prior(prior, top_k=n)
    c1._prior = c2._prior = None
    prior.close()                                  # freed first: the contexts keep it alive
    for c, k in ((c1, 3), (c2, n)):
        c.step_windows(rec, S, 0, B, 5, None, sync=True)
        _same(c.step_prior_results(B), prior_ref.apply(c.step_results(B)[0], table, [0] * B, THR, k))
    c1.close()
    c2.close()
    prior = bn.Prior(0, table, THR)
    c3 = bn.Context(model, B)
    c3.attach_prior(prior, top_k=3)
    c3.close()                                     # the context first, then the prior
    prior.close()


def test_refusals_leave_the_previous_attachment(bn, model):
    n, B = int(model.config.num_species), 2
    table = _table(n, 3, 4)
    pcm, S = _pcm(model, 3 * B)
    rec = bn.Recording(pcm)
    good = bn.Prior(0, table, THR)
    ctx = bn.Context(model, B)
    ctx.attach_prior(good, source_sites=[0, 1], top_k=3)
    ctx.set_prior_site(1)
    nan_t, inf_t = table.copy(), table.copy()
    nan_t[1, 2], inf_t[2, 0] = np.nan, -np.inf
    live3 = bn.Live(0, 3, S, S, 4 * S, 1)          # more sources than the attached map
    for s in range(3):
        live3.push(s, pcm[s * S:(s + 1) * S])
    other = bn.Prior(0, _table(n + 1, 1, 0), THR)
    calls = [
        lambda: bn.Prior(0, np.zeros((0, n), dtype=np.float32), THR),
        lambda: bn.Prior(0, nan_t, THR),
        lambda: bn.Prior(0, inf_t, THR),
        lambda: bn.Prior(0, table, float("inf")),
        lambda: bn.Prior(0, table, THR, flags=8),
        lambda: ctx.attach_prior(other, top_k=3),                       # n_species != num_species
        lambda: ctx.attach_prior(good, top_k=0),
        lambda: ctx.attach_prior(good, top_k=1025),
        lambda: ctx.attach_prior(good, source_sites=[0, 3], top_k=3),   # a site outside 0..n_sites
        lambda: ctx.attach_prior(good, source_sites=[0, -1], top_k=3),
        lambda: ctx.set_prior_site(3),
        lambda: ctx.set_prior_site(-1),
        lambda: bn.Context(model, B).set_prior_site(0),                 # no prior attached
        lambda: ctx.step_live(live3, B, 5, None, sync=True),
        lambda: good.apply(np.zeros((2, n), dtype=np.float32), [0, 3], 3),
        lambda: good.apply(np.zeros((2, n), dtype=np.float32), [0, 1], 0),
        lambda: good.apply(np.zeros((2, n), dtype=np.float32), [0, 1], 3, k_stride=2),
        lambda: bn.Prior(0, table, THR, after_topk=True).apply(np.zeros((2, n), dtype=np.float32), [0, 1], 0),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(bn.EngineError) as e:
            call()
        assert e.value.status == 1 and bn.last_error(), i
    assert live3.ready(0) == 1                     # the refused live step took nothing from the pool
    null = bn.lib.bn_prior_apply_host(good._h, None, 2, None, 3, 0, C.c_float(0), 3, None, None, None)
    assert null == 1 and bn.last_error()
    # the attachment made before the refusals still stands, site 1 and K = 3
    ctx.step_windows(rec, S, 0, B, 5, None, sync=True)
    _same(ctx.step_prior_results(B), prior_ref.apply(ctx.step_results(B)[0], table, [1] * B, THR, 3))
    if bn.device_count() > 1:  # a prior can only be made on a device that exists: one GPU cannot reach this refusal
        with pytest.raises(bn.EngineError) as e:
            ctx.attach_prior(bn.Prior(1, table, THR), top_k=3)
        assert e.value.status == 1


# ---- host mirror ----------------------------------------------------------------------------------------------------
def test_host_mirror_prior_row_and_after_topk_equals_filter_predictions(bn):
    n_meta = 40
    meta_labels = [f"m{i}" for i in range(n_meta)]
    rf = bn.RangeFilter.builder().model_path(write_model(synth.meta_model(num_species=n_meta, hidden=16))).labels(meta_labels).threshold(0.05).with_rocm(0).build()
    lat, lon, month, day = 60.2, 24.9, 6, 15
    raw = rf.scores(lat, lon, month, day)
    assert raw.shape == (n_meta,)
    pred = rf.predict(lat, lon, month, day)
    assert sorted(p.index for p in pred) == [i for i in range(n_meta) if raw[i] >= np.float32(0.05)]
    assert all(np.float32(p.score).tobytes() == raw[p.index].tobytes() for p in pred)
    for bad in ((95.0, 0.0, 6, 15), (0.0, 200.0, 6, 15)):
        with pytest.raises(bn.Error) as e:
            rf.scores(*bad)
        assert e.value.kind == bn.ErrorKind.InvalidCoordinates and oracle.validate_coordinates(bad[0], bad[1]) != 0
    for bad in ((0.0, 0.0, 13, 1), (0.0, 0.0, 6, 32)):
        with pytest.raises(bn.Error) as e:
            rf.scores(*bad)
        assert e.value.kind == bn.ErrorKind.InvalidDate and oracle.validate_date(bad[2], bad[3]) != 0
    # classifier labels: a shuffled part of the meta model's, and some it lacks
    rng = np.random.default_rng(2)
    order = rng.permutation(n_meta)[:30]
    cls_labels = [meta_labels[i] for i in order] + [f"x{i}" for i in range(6)]
    rng.shuffle(cls_labels)
    row = rf.prior_row(cls_labels, lat, lon, month, day)
    want = np.array([raw[int(l[1:])] if l[0] == "m" else -1.0 for l in cls_labels], dtype=np.float32)
    assert row.tobytes() == want.tobytes()
    n = len(cls_labels)
    logits = (rng.standard_normal((4, n)) * 2).astype(np.float32)
    thr = float(np.float32(np.median(raw)))
    for rerank in (False, True):
        prior = bn.Prior(0, row[None, :], thr, after_topk=True, rerank=rerank)
        idx, conf, cnt = prior.apply(logits, [0] * 4, 8, 0.1)
        ti, tc, tn = bn.topk_host(logits, 8, 0.1)
        loc = [bn.LocationScore(meta_labels[i], float(raw[i]), i) for i in range(n_meta)]   # the full score list, not predict's
        for r in range(4):
            preds = [bn.Prediction(cls_labels[int(ti[r, j])], float(tc[r, j]), int(ti[r, j])) for j in range(int(tn[r]))]
            kept = bn.filter_predictions(preds, loc, thr, rerank)
            assert [p.index for p in kept] == [int(v) for v in idx[r, :cnt[r]]]
            assert np.array([p.confidence for p in kept], dtype=np.float32).tobytes() == conf[r, :cnt[r]].tobytes()
