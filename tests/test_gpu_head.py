"""Classifier heads on the GPU (bn_head_*) against the float64 restatements of tests/head_ref.py.

Apply: every logit within the derived bound 2 (dim + 8) 2^-24 (sum |W xh| + |b|); bits identical across batch size, row position, a
head holding a subset of the classes, and bn_head_apply_host versus an attached step.  Step: the model's own outputs unchanged bit for
bit, head top-K bit-identical to bn_topk_host of the head logits, through bn_step_device / bn_step_windows / bn_step_live, no capture
fallback, shared heads and either order of frees, detach, refusals.  Fit: converged, and the float64 certificate and L - L*_Newton at
the returned parameters both <= 2 tol on the three fixtures (the factor 2 covers (sqrt(tol) + sqrt(floor))^2, the floor being the f32
gradient's own error, 1e-13 to 1e-15 here); determinism; max_iters; bn_head_fit_index; and the end-to-end workflow."""
import ctypes as C
import importlib

import numpy as np
import pytest

import head_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
TOL = 1e-6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- apply ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l2norm", [False, True])
@pytest.mark.parametrize("classes", [1, 3, 64, 1000])
@pytest.mark.parametrize("dim", [1, 7, 130, 1024, 1536])
def test_apply_bound_and_bit_identity(bn, dim, classes, l2norm):
    rng = np.random.default_rng(dim * 7 + classes)
    W = rng.standard_normal((classes, dim)).astype(np.float32)
    b = rng.standard_normal(classes).astype(np.float32)
    X = (rng.standard_normal((128, dim)) * rng.uniform(0.1, 10, (128, 1))).astype(np.float32)
    X[5] = 0.0                      # zero norm
    if dim > 1:
        X[9, dim // 2] = np.inf     # non-finite element
    X[12] = 1e30 if l2norm else 1.0  # finite elements whose sum of squares overflows f32 (without the flag: an ordinary row)
    head = bn.Head(0, W, b, l2norm=l2norm)
    assert (head.dim, head.n_classes, head.l2norm) == (dim, classes, l2norm)
    rw, rb = head.read()
    assert rw.tobytes() == W.tobytes() and rb.tobytes() == b.tobytes()
    full = head.apply(X)
    finite = np.isfinite(X).all(axis=1) if not l2norm else np.ones(128, dtype=bool)
    z, bound = head_ref.logits64(W, b, X[finite], l2norm)
    err = np.abs(full[finite].astype(np.float64) - z)
    mag = bound / (2.0 * (dim + 8))  # 2^-24 * (sum |w x| + |b|)
    ratio = err / mag
    print(f"dim {dim} classes {classes} l2norm {l2norm}: logit error rms {np.sqrt((ratio ** 2).mean()):.3f} max {ratio.max():.3f} x 2^-24 sum|w||x|")
    assert np.all(err <= bound), (err / bound).max()
    if l2norm:
        assert bits(full[5]).tobytes() == bits(b).tobytes() and (dim == 1 or bits(full[9]).tobytes() == bits(b).tobytes())
        assert bits(full[12]).tobytes() == bits(b).tobytes()
    for n in (1, 2, 15, 16, 17, 33, 100, 127):
        assert bits(head.apply(X[:n])).tobytes() == bits(full[:n]).tobytes(), n
    perm = rng.permutation(128)
    assert bits(head.apply(X[perm])).tobytes() == bits(full[perm]).tobytes()
    sub = np.sort(rng.choice(classes, max(1, classes // 3), replace=False))
    part = bn.Head(0, W[sub], b[sub], l2norm=l2norm)
    assert bits(part.apply(X)).tobytes() == bits(full[:, sub]).tobytes()
    nobias = bn.Head(0, W[:1], None, l2norm=l2norm)
    assert np.all(nobias.read()[1] == 0)


def test_apply_more_rows_than_one_round(bn):
    rng = np.random.default_rng(1)
    W = rng.standard_normal((5, 96)).astype(np.float32)
    X = rng.standard_normal((2500, 96)).astype(np.float32)
    head = bn.Head(0, W, None)
    z, bound = head_ref.logits64(W, None, X, False)
    got = head.apply(X)
    assert np.all(np.abs(got - z) <= bound)
    assert bits(head.apply(X[2000:2100])).tobytes() == bits(got[2000:2100]).tobytes()


# ---- step -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v30(num_species=300, width=0.5, depth=0.5, emb=256)))


def _pcm(model, n_windows, seed=0):
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    x = synth.synthetic_segments(1, S * n_windows, sr)[0]
    rng = np.random.default_rng(seed)
    return np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32), S


def _check_head_rows(bn, head, emb, got, top_k, min_conf):
    lg, ix, cf, ct = got
    assert bits(lg).tobytes() == bits(head.apply(emb)).tobytes()
    wi, wc, wn = bn.topk_host(lg, top_k, min_conf)
    assert np.array_equal(ct, wn)
    for r in range(len(ct)):
        assert np.array_equal(ix[r, :ct[r]], wi[r, :wn[r]]) and bits(cf[r, :ct[r]]).tobytes() == bits(wc[r, :wn[r]]).tobytes()


def test_step_paths_outputs_unchanged_and_head_results(bn, model):
    rng = np.random.default_rng(2)
    dim, B = int(model.config.embedding_dim), 6
    assert dim == 256
    W = rng.standard_normal((37, dim)).astype(np.float32)
    b = rng.standard_normal(37).astype(np.float32)
    head = bn.Head(0, W, b, l2norm=True)
    pcm, S = _pcm(model, 2 * B)
    rec = bn.Recording(pcm)
    plain, ctx = bn.Context(model, B), bn.Context(model, B)
    ctx.attach_head(head, top_k=5, min_confidence=0.1)
    eo = model.config.embedding_output
    for first, m in ((0, B), (B, B - 2)):
        # bn_step_windows
        plain.step_windows(rec, S, first, m, 10, 0.01, sync=True)
        want = plain.step_results(m)
        ctx.step_windows(rec, S, first, m, 10, 0.01, sync=True)
        got = ctx.step_results(m)
        for a, w in zip(got, want):
            assert a.tobytes() == w.tobytes()
        emb = ctx.read_output(eo, m)
        hres = ctx.step_head_results(m)
        assert hres[0].shape == (m, 37) and hres[1].shape == (m, 5)
        _check_head_rows(bn, head, emb, hres, 5, 0.1)
        z, bound = head_ref.logits64(W, b, emb, True)
        assert np.all(np.abs(hres[0] - z) <= bound)
        # bn_step_device on the context's own input buffer (the windows just cut into it), asynchronous
        ctx.step_device(ctx.input_device()[0], m, 10, 0.01, sync=False)
        ctx.synchronize()
        for a, w in zip(ctx.step_results(m), want):
            assert a.tobytes() == w.tobytes()
        for a, w in zip(ctx.step_head_results(m), hres):
            assert a.tobytes() == w.tobytes()
    # bn_step_live
    live = bn.Live(0, 2, S, S, 4 * S, 1)
    live.push(0, pcm[:2 * S])
    live.push(1, pcm[2 * S:4 * S])
    src, win = ctx.step_live(live, B, 10, 0.01, sync=True)
    assert len(src) == 4
    got, hres = ctx.step_results(4), ctx.step_head_results(4)
    order = [int(s) * 2 + int(w) for s, w in zip(src, win)]
    plain.step_windows(rec, S, 0, 4, 10, 0.01, sync=True)
    want = plain.step_results(4)
    for a, w in zip(got, want):
        assert a.tobytes() == w[order].tobytes()
    _check_head_rows(bn, head, ctx.read_output(eo, 4), hres, 5, 0.1)
    assert ctx.stats()["capture_fallbacks"] == 0 and plain.stats()["capture_fallbacks"] == 0
    assert ctx.stats()["replays"] > 0
    # detach restores the plain step
    ctx.attach_head(None)
    ctx.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    plain.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    for a, w in zip(ctx.step_results(B), plain.step_results(B)):
        assert a.tobytes() == w.tobytes()
    with pytest.raises(bn.EngineError) as e:
        ctx.step_head_results(B)
    assert e.value.status == 1


def test_two_contexts_share_a_head_freed_first(bn, model):
    rng = np.random.default_rng(4)
    dim, B = int(model.config.embedding_dim), 4
    W = rng.standard_normal((1000, dim)).astype(np.float32)
    head = bn.Head(0, W, None)
    keep = bn.Head(0, W, None)
    pcm, S = _pcm(model, 2 * B, seed=1)
    rec = bn.Recording(pcm)
    c1, c2 = bn.Context(model, B), bn.Context(model, B)
    c1.attach_head(head, top_k=1000)
    c2.attach_head(head, top_k=3, min_confidence=0.5)
    c1._head = c2._head = None
    head.close()                     # the contexts keep it alive
    c1.step_windows(rec, S, 0, B, 10, None, sync=False)
    c2.step_windows(rec, S, B, B, 10, None, sync=False)
    c1.synchronize()
    c2.synchronize()
    eo = model.config.embedding_output
    _check_head_rows(bn, keep, c1.read_output(eo, B), c1.step_head_results(B), 1000, None)
    _check_head_rows(bn, keep, c2.read_output(eo, B), c2.step_head_results(B), 3, 0.5)
    c1.close()
    c2.close()


def test_refusals(bn, model):
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    dim = int(model.config.embedding_dim)
    ctx = bn.Context(model, 2)
    good = bn.Head(0, np.ones((4, dim), dtype=np.float32), None)
    v24 = bn.Model(write_model(synth.birdnet_v24(num_species=64, width=0.25, depth=0.25, head=64)))
    calls = [
        lambda: bn.Context(v24, 2).attach_head(bn.Head(0, np.ones((4, 64), dtype=np.float32), None)),   # no embeddings
        lambda: ctx.attach_head(bn.Head(0, np.ones((4, dim + 1), dtype=np.float32), None)),              # dim != embedding_dim
        lambda: ctx.attach_head(good, top_k=0),
        lambda: bn.Head(0, np.ones((1, 8193), dtype=np.float32), None),
        lambda: bn.Head(0, np.ones((4097, 2), dtype=np.float32), None),
        lambda: bn.Head(0, np.ones((0, 2), dtype=np.float32), None),
    ]
    X, Y, _, _ = head_ref.fixture("n2000_d256_c3")
    bad_y = Y.copy()
    bad_y[17, 1] = 2
    calls += [
        lambda: bn.Head.fit(0, X, bad_y),
        lambda: bn.Head.fit(0, X, Y, l2=-1.0),
        lambda: bn.Head.fit(0, X, Y, l2=float("inf")),
        lambda: bn.Head.fit(0, X, Y, tol=float("nan")),
        lambda: bn.Head.fit(0, X, Y, pos_weight=[1.0, 0.0, 1.0]),
        lambda: bn.Head.fit(0, X, Y, pos_weight=[1.0, float("inf"), 1.0]),
        lambda: bn.Head.fit(0, X[:0], Y[:0]),
    ]
    idx = bn.Index(0, 256, 64)
    rows = X[:10].copy()
    rows[3] = 0.0
    idx.add(rows)
    calls += [
        lambda: bn.Head.fit_index(idx, [0, 1, 10], Y[:3]),   # id >= size
        lambda: bn.Head.fit_index(idx, [0, 3, 4], Y[:3]),    # a row stored as zeros
        lambda: bn.Head.fit_index(idx, [], Y[:0]),
    ]
    for i, call in enumerate(calls):
        with pytest.raises(bn.EngineError) as e:
            call()
        assert e.value.status == 1 and bn.last_error(), i
    if bn.device_count() > 1:  # a head can only be made on a device that exists: one GPU cannot reach this refusal
        with pytest.raises(bn.EngineError) as e:
            ctx.attach_head(bn.Head(1, np.ones((4, dim), dtype=np.float32), None))
        assert e.value.status == 1
    # nothing changed: the context still steps plainly, and a valid attach still works
    rec = bn.Recording(_pcm(model, 2)[0])
    ctx.step_windows(rec, int(model.config.sample_count), 0, 2, 10, None, sync=True)
    with pytest.raises(bn.EngineError):
        ctx.step_head_results(2)
    ctx.attach_head(good, top_k=4)
    ctx.step_windows(rec, int(model.config.sample_count), 0, 2, 10, None, sync=True)
    assert ctx.step_head_results(2)[0].shape == (2, 4)


# ---- fit ------------------------------------------------------------------------------------------------------------
def _check_fit(name, head, X, Y, l2, pw, newton_loss):
    W, b = head.read()
    rep = head.report
    loss, _, _, cert = head_ref.objective(W, b, X, Y, l2, pw)
    print(f"{name}: iters {rep['iters']} converged {rep['converged']} f32 certificate {rep['certificate']:.3e} loss {rep['loss']:.9f}; "
          f"float64 certificate {cert:.3e}, L - L* {loss - newton_loss:.3e}")
    assert rep["converged"]
    assert cert <= 2 * TOL
    assert loss - newton_loss <= 2 * TOL
    assert abs(rep["loss"] - loss) <= 1e-5


@pytest.mark.parametrize("name", sorted(head_ref.FIXTURES))
def test_fit_reaches_the_certificate(bn, name):
    X, Y, l2, pw = head_ref.fixture(name)
    Wn, bn_ = head_ref.newton(X, Y, l2, pw)
    newton_loss = head_ref.objective(Wn, bn_, X, Y, l2, pw)[0]
    head = bn.Head.fit(0, X, Y, l2=l2, tol=TOL, l2norm=True, pos_weight=pw)
    assert head.l2norm and (head.n_classes, head.dim) == (Y.shape[1], X.shape[1])
    # the rows are unit vectors already; the head's inputs are their f32 re-normalisation
    _check_fit(name, head, head_ref.normalise64(X), Y, l2, pw, newton_loss)
    again = bn.Head.fit(0, X, Y, l2=l2, tol=TOL, l2norm=True, pos_weight=pw)
    assert again.report == head.report
    for a, c in zip(head.read(), again.read()):
        assert a.tobytes() == c.tobytes()


def test_fit_defaults_degenerate_classes_and_max_iters(bn):
    X, Y, l2, _ = head_ref.fixture("n2000_d256_c3")
    Y = Y.copy()
    Y[:, 0] = 0                      # no positives
    Y[:, 2] = 1                      # no negatives
    head = bn.Head.fit(0, X, Y)      # defaults: l2 1e-3, tol 1e-6, max_iters 2000, rows used as they are
    assert not head.l2norm
    Wn, bn_ = head_ref.newton(X, Y, 1e-3)
    _check_fit("degenerate", head, X, Y, 1e-3, None, head_ref.objective(Wn, bn_, X, Y, 1e-3)[0])
    z = head.apply(X)
    assert np.all(z[:, 0] < 0) and np.all(z[:, 2] > 0)
    short = bn.Head.fit(0, X, Y, max_iters=3)
    assert short.report["iters"] == 3 and not short.report["converged"] and short.report["certificate"] > TOL
    assert short.read()[0].shape == (3, 256)


def test_fit_index_meets_the_certificate_against_the_stored_rows(bn):
    X, Y, l2, pw = head_ref.fixture("n2000_d256_c3_l2_1e-4_pw4")
    rng = np.random.default_rng(8)
    raw = (X * rng.uniform(0.5, 20, (len(X), 1))).astype(np.float32)  # the index normalises on append
    idx = bn.Index(0, 256, 4000)
    idx.add(rng.standard_normal((100, 256)).astype(np.float32))
    first = idx.add(raw)
    ids = rng.permutation(np.arange(first, first + len(X)))[:1500]
    stored = idx.read()[ids]
    Ys = Y[ids - first]
    head = bn.Head.fit_index(idx, ids, Ys, l2=l2, tol=TOL, pos_weight=pw)
    assert head.l2norm
    Wn, bn_ = head_ref.newton(stored, Ys, l2, pw)
    _check_fit("fit_index", head, stored, Ys, l2, pw, head_ref.objective(Wn, bn_, stored, Ys, l2, pw)[0])
    # per-class top-M over the index is a search with W_c as the query: logit = cosine |W_c| + b_c
    out_i, out_z, cnt = idx.search_head(head, 20)
    z = head.apply(idx.read())
    for c in range(head.n_classes):
        assert cnt[c] == 20
        assert np.all(np.abs(out_z[c] - z[out_i[c].astype(np.int64), c]) <= 1e-4)
        assert out_z[c, -1] >= np.sort(z[:, c])[-20] - 1e-4


def test_end_to_end_search_label_fit_attach_live(bn, model):
    cfg = model.config
    S, sr, B, n_src, n_win = int(cfg.sample_count), int(cfg.sample_rate), 8, 6, 4
    rng = np.random.default_rng(12)
    t = np.arange(S * n_win) / sr
    pcms = []
    for s in range(n_src):
        if s % 2:
            x = sum(0.3 * np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in rng.uniform(500, 6000, 3))
        else:
            x = 0.3 * rng.standard_normal(len(t))
        pcms.append(np.clip(x, -1, 1).astype(np.float32))
    ctx = bn.Context(model, B)
    idx = bn.Index(0, int(cfg.embedding_dim), n_src * n_win)
    for s in range(n_src):
        ctx.infer_windows(bn.Recording(pcms[s]), S, 0, n_win)
        assert idx.add_context(ctx, n_win) == s * n_win
    E = idx.read().astype(np.float64)
    fam = np.repeat(np.arange(n_src) % 2, n_win)
    u = E[fam == 1].mean(axis=0) - E[fam == 0].mean(axis=0)
    p = E @ u
    order = np.argsort(p)
    gaps = np.diff(p[order])
    lo, hi = len(p) // 4, len(p) - len(p) // 4
    cut = lo + int(np.argmax(gaps[lo - 1:hi - 1]))          # the widest gap that leaves a quarter of the rows on each side
    theta = 0.5 * (p[order[cut - 1]] + p[order[cut]])
    labels = (p > theta).astype(np.uint8)                    # linearly separable by construction, margin = half that gap
    assert 0 < labels.sum() < len(labels)
    Y = np.stack([labels, 1 - labels], axis=1)
    head = bn.Head.fit_index(idx, np.arange(len(labels)), Y, l2=1e-5)
    print("end to end:", head.report, "margin", 0.5 * gaps[cut - 1])
    ctx.attach_head(head, top_k=1)
    live = bn.Live(0, n_src, S, S, 2 * S * n_win, 1)
    for s in range(n_src):
        live.push(s, pcms[s])
    seen = 0
    while live.ready() > 0:
        src, win = ctx.step_live(live, B, 10, None, sync=True)
        z, ix, cf, ct = ctx.step_head_results(len(src))
        ids = src.astype(np.int64) * n_win + win.astype(np.int64)
        assert np.array_equal(z[:, 0] > 0, labels[ids] == 1), (z[:, 0], labels[ids])
        assert np.array_equal(z[:, 1] > 0, labels[ids] == 0)
        assert np.array_equal(ix[:, 0], 1 - labels[ids])
        seen += len(src)
    assert seen == n_src * n_win
