"""Detection events on the GPU (bn_track_*): every comparison is tobytes() of the sorted event array against tests/track_ref.py.

Widths below one wave, around one wave, no multiple of 4 or 64, more than one block, the flagship 6522; three (min_hits, max_gap) sets;
updates that mix the sources and hold two windows of one source; a row of confidences exactly at enter_conf and a row of NaN / +-inf
logits; independence of the batching; the prior's gate and rerank; overflow of max_events; the step entry points (bn_step_windows, and
bn_step_live from two contexts in flight on one pool); stale rows; refusals and lifetime."""
import ctypes as C
import importlib

import numpy as np
import pytest

import oracle
import prior_ref
import track_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
Z_ENTER = np.float32(0.25)
ENTER = float(np.float32(oracle.sigmoid(float(Z_ENTER))))   # logit 0.25 gives exactly this confidence
PARAMS = ((1, 0), (2, 1), (3, 2))
N_SRC, N_WIN = 3, 12
THR = 0.3
_CASES = {}


def _case(n):
    """36 rows (3 sources x 12 windows) of n logits, about a fifth of them hits, in runs (a per-species level plus per-window noise);
    absolute window numbers with holes; rows ordered by (window index, source).  The sigmoids are computed once per width."""
    if n not in _CASES:
        rng = np.random.default_rng(1000 + n)
        level = rng.standard_normal((N_SRC, 1, n)) * 2
        x = (level + rng.standard_normal((N_SRC, N_WIN, n)) - 1.9 + float(Z_ENTER)).astype(np.float32)   # P(x >= 0.25) = P(N(0, 5) >= 1.9) = 0.2
        x[0, 4] = Z_ENTER                             # a row of confidences exactly equal to enter_conf: every species hits
        x[1, 7] = np.resize(np.array([np.nan, np.inf, -np.inf, -np.nan, 0.3], dtype=np.float32), n)
        wins = np.stack([np.sort(rng.choice(16, N_WIN, replace=False)) + base for base in (0, 1000, 2 ** 31 - 16)])
        src = np.tile(np.arange(N_SRC), N_WIN)
        idx = np.repeat(np.arange(N_WIN), N_SRC)
        rows = np.ascontiguousarray(x[src, idx])
        _CASES[n] = (rows, src.astype(np.int32), wins[src, idx].astype(np.uint64), prior_ref.sigmoid_row(rows).reshape(rows.shape))
    return _CASES[n]


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, got, want)


def _feed(bn, case, cuts, min_hits, max_gap, prior=None, ref_prior=None, sites=None):
    """The case through a device tracker and the reference in updates cut at `cuts`; every update and the flush compared.  Returns the
    concatenated-and-sorted update events and the flush events of the device."""
    rows, src, win, conf = case
    n = rows.shape[1]
    # room for whatever one update can close (a record closes at most once per row): nothing is dropped
    dev = bn.Tracker(0, N_SRC, n, ENTER, min_hits, max_gap, max_events=36 * n, use_prior=prior is not None)
    ref = track_ref.Tracker(N_SRC, n, ENTER, min_hits, max_gap, prior=ref_prior)
    assert (dev.n_sources, dev.n_species, dev.open_events()) == (N_SRC, n, 0)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        st = None if sites is None else sites[a:b]
        got, dropped = dev.update(rows[a:b], src[a:b], win[a:b], prior=prior, sites=st)
        want = ref.update(rows[a:b], src[a:b], win[a:b], sites=st, conf=conf[a:b])
        assert dropped == 0
        _same(got, want, (n, min_hits, max_gap, a, b))
        parts.append(got)
    assert dev.open_events() == ref.open_events() and dev.open_events(1) == ref.open_events(1)
    got, dropped = dev.flush()
    _same(got, ref.flush(), (n, min_hits, max_gap, "flush"))
    assert dropped == 0 and dev.open_events() == 0
    return track_ref.concat(parts), got


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 257, 6522])
def test_widths_and_parameter_sets_in_updates_of_five_mixed_rows(bn, n):
    case = _case(n)
    hits = case[3] >= np.float32(ENTER)
    if n >= 63:
        assert 0.1 < hits.mean() < 0.35                   # about a fifth
    cuts = list(range(0, 36, 5)) + [36]                    # rows (w0: s0 s1 s2)(w1: s0 s1 | s2) ...: two windows of a source in an update
    total = 0
    for min_hits, max_gap in PARAMS:
        ev, fl = _feed(bn, case, cuts, min_hits, max_gap)
        total += len(ev) + len(fl)
    assert total > 0 or n == 1


def test_events_do_not_depend_on_the_batching(bn):
    case = _case(257)
    rng = np.random.default_rng(3)
    random_cuts = [0] + sorted(rng.choice(np.arange(1, 36), 6, replace=False).tolist()) + [36]
    results = [_feed(bn, case, cuts, 2, 1) for cuts in (list(range(37)), [0, 36], random_cuts)]
    assert len(results[0][0]) > 20 and len(results[0][1]) > 20
    for ev, fl in results[1:]:
        _same(ev, results[0][0])
        _same(fl, results[0][1])
    again = _feed(bn, case, random_cuts, 2, 1)             # two runs: the same bytes
    _same(again[0], results[0][0])
    # a flush of one source, a reset of another, and the sources' later windows
    rows, src, win, conf = case
    dev, ref = bn.Tracker(0, N_SRC, 257, ENTER, 1, 1), track_ref.Tracker(N_SRC, 257, ENTER, 1, 1)
    _same(dev.update(rows[:18], src[:18], win[:18])[0], ref.update(rows[:18], src[:18], win[:18], conf=conf[:18]))
    _same(dev.flush(2)[0], ref.flush(2))
    dev.reset(0)
    ref.reset(0)
    assert dev.open_events() == ref.open_events() and dev.open_events(0) == 0 == dev.open_events(2)
    w2 = win.copy()
    w2[src == 0] -= w2[18]                                 # the reset source starts over, at a window below its old last
    _same(dev.update(rows[18:], src[18:], w2[18:])[0], ref.update(rows[18:], src[18:], w2[18:], conf=conf[18:]))
    _same(dev.flush()[0], ref.flush())


@pytest.mark.parametrize("rerank", [False, True])
def test_prior_gates_hits_and_reranks(bn, rerank):
    n = 65
    case = _case(n)
    rng = np.random.default_rng(8)
    table = rng.uniform(0, 1, (3, n)).astype(np.float32)
    table[rng.uniform(size=table.shape) < 0.2] = prior_ref.UNKNOWN
    table[1] = 0.1                                         # site 1 admits nothing
    table[0, 5] = np.float32(THR)                          # p == threshold exactly: admitted
    table[2, :4] = [0.0, 1.0, prior_ref.UNKNOWN, 2.0]
    sites = np.array([2, 1, 0], dtype=np.int32)[case[1]]   # source -> site, not the identity
    prior = bn.Prior(0, table, THR, rerank=rerank)
    for min_hits, max_gap in PARAMS[:2]:
        ev, fl = _feed(bn, case, list(range(0, 36, 5)) + [36], min_hits, max_gap, prior=prior, ref_prior=(table, THR, rerank), sites=sites)
        both = track_ref.concat([ev, fl])
        assert len(both) > 0 and not (both["source"] == 1).any() and (both["source"] == 0).any()
    plain = _feed(bn, case, [0, 36], 1, 0)
    assert track_ref.concat(plain).tobytes() != track_ref.concat(_feed(bn, case, [0, 36], 1, 0, prior=prior, ref_prior=(table, THR, rerank), sites=sites)).tobytes()


def test_overflow_counts_what_it_drops(bn):
    n = 64
    x = np.stack([np.full(n, 3.0, dtype=np.float32), np.full(n, -3.0, dtype=np.float32)])
    dev, ref = bn.Tracker(0, 1, n, ENTER, 1, 0, max_events=4), track_ref.Tracker(1, n, ENTER, 1, 0)
    want = ref.update(x, [0, 0], [0, 1])
    got, dropped = dev.update(x, [0, 0], [0, 1])
    assert len(want) == n and len(got) == 4 and len(got) + dropped == len(want)
    known = {w.tobytes() for w in want}
    assert all(g.tobytes() in known for g in got) and len({g.tobytes() for g in got}) == 4
    assert list(got["species"]) == sorted(got["species"]) and dev.open_events() == 0
    # the caller's capacity cuts the sorted list, and counts what it cuts
    dev = bn.Tracker(0, 1, n, ENTER, 1, 0, max_events=n)
    got, dropped = dev.update(x, [0, 0], [0, 1], cap=10)
    _same(got, want[:10])
    assert dropped == n - 10
    dev.update(x[:1], [0], [5])
    got, dropped = dev.flush(0, cap=3)
    assert dropped == n - 3 and list(got["species"]) == [0, 1, 2] and list(got["first_window"]) == [5, 5, 5]


# ---- step -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v24(num_species=70, width=0.25, depth=0.25, head=32)))


def _pcm(model, n_windows, seed=0):
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    x = synth.synthetic_segments(1, S * n_windows, sr)[0]
    rng = np.random.default_rng(seed)
    return np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32), S


def _enter_for(logits):
    """An enter_conf that makes about a fifth of these logits hits (the synthetic model's logits sit wherever its random weights put them)."""
    return float(np.quantile(prior_ref.sigmoid_row(logits), 0.8))


@pytest.mark.parametrize("with_prior", [False, True])
def test_step_windows_in_batches_of_three(bn, model, with_prior):
    n, B, n_win = int(model.config.num_species), 3, 8
    pcm, S = _pcm(model, n_win)
    rec = bn.Recording(pcm)
    plain, ctx = bn.Context(model, B), bn.Context(model, B)
    batches = [(0, 3), (3, 3), (6, 2)]
    want = []
    for first, m in batches:
        plain.step_windows(rec, S, first, m, 5, 0.01, sync=True)
        want.append([a.copy() for a in plain.step_results(m)])
    enter = _enter_for(np.concatenate([w[0] for w in want]))
    table = None
    if with_prior:
        rng = np.random.default_rng(n)
        table = rng.uniform(0.2, 1, (2, n)).astype(np.float32)
        table[rng.uniform(size=table.shape) < 0.2] = prior_ref.UNKNOWN
        ctx.attach_prior(bn.Prior(0, table, THR, rerank=True), top_k=4)
        ctx.set_prior_site(1)
        enter *= 0.7
    dev = bn.Tracker(0, 2, n, enter, 2, 1, use_prior=with_prior)
    ref = track_ref.Tracker(2, n, enter, 2, 1, prior=(table, THR, True) if with_prior else None)
    ctx.attach_track(dev)
    ctx.set_track_source(1)
    parts = []
    for (first, m), w in zip(batches, want):
        ctx.step_windows(rec, S, first, m, 5, 0.01, sync=False)
        ctx.synchronize()
        got = ctx.step_results(m)
        for a, b in zip(got, w):
            assert a.tobytes() == b.tobytes()              # the step's own logits and top-K: bit-identical to a context without a tracker
        ev, dropped, stale = ctx.step_track_results()
        assert (dropped, stale) == (0, 0)
        _same(ev, ref.update(got[0], [1] * m, range(first, first + m), sites=[1] * m))
        parts.append(ev)
    assert dev.open_events() == ref.open_events() == dev.open_events(1) and dev.open_events(0) == 0
    fl = dev.flush()[0]
    _same(fl, ref.flush())
    every = track_ref.concat(parts + [fl])
    assert len(every) > 0 and (every["source"] == 1).all() and (every["hits"] >= 2).all()
    assert ctx.stats()["capture_fallbacks"] == 0 and plain.stats()["capture_fallbacks"] == 0 and ctx.stats()["replays"] > 0
    # bn_step_device rows carry no window number: not tracked, the last tracked step's results stay
    ctx.step_device(ctx.input_device()[0], 2, 5, 0.01, sync=True)
    assert dev.open_events() == 0 and len(ctx.step_track_results()[0]) == len(parts[-1])
    # detach restores the plain step
    ctx.attach_track(None)
    ctx.step_windows(rec, S, 0, B, 5, 0.01, sync=True)
    for a, b in zip(ctx.step_results(B), want[0]):
        assert a.tobytes() == b.tobytes()
    assert dev.open_events() == 0
    with pytest.raises(bn.EngineError) as e:
        ctx.step_track_results()
    assert e.value.status == 1


def test_live_two_contexts_in_flight_on_one_pool_and_stale_rows(bn, model):
    n, B, n_src = int(model.config.num_species), 3, 4
    S = int(model.config.sample_count)
    live = bn.Live(0, n_src, S, S, 8 * S, 1)
    pushes = (1, 4, 2, 3)                                  # windows per source: uneven
    for s, w in enumerate(pushes):
        live.push(s, _pcm(model, w, seed=s)[0])
    probe = bn.Context(model, B)
    probe.step_windows(bn.Recording(_pcm(model, 3, seed=1)[0]), S, 0, 3, 5, None, sync=True)
    enter = _enter_for(probe.step_results(3)[0])
    dev, ref = bn.Tracker(0, n_src, n, enter, 1, 0), track_ref.Tracker(n_src, n, enter, 1, 0)
    ctxs = [bn.Context(model, B), bn.Context(model, B)]
    for c in ctxs:
        c.attach_track(dev)
    parts, want, seen = [], [], 0
    while True:
        taken = [c.step_live(live, B, 5, None, sync=False) for c in ctxs]   # both in flight on the one pool and the one tracker
        if not any(len(t[0]) for t in taken):
            break
        for c, (src, win) in zip(ctxs, taken):             # the tracker's updates were applied in this order
            if not len(src):
                continue
            c.synchronize()
            ev, dropped, stale = c.step_track_results()
            assert (dropped, stale) == (0, 0)
            w = ref.update(c.step_results(len(src))[0], src, win)
            _same(ev, w, (src, win))
            parts.append(ev)
            want.append(w)
            seen += len(src)
    assert seen == sum(pushes) and all(c.stats()["capture_fallbacks"] == 0 for c in ctxs)
    assert dev.open_events() == ref.open_events() > 0
    # bn_live_reset without bn_track_reset: the new stream's windows 0, 1 do not exceed source 1's last; source 0 goes on at window 1
    live.reset(1)
    live.push(1, _pcm(model, 2, seed=9)[0])
    open_before = dev.open_events()
    src, win = ctxs[0].step_live(live, B, 5, None, sync=True)
    assert list(src) == [1, 1] and list(win) == [0, 1]
    ev, dropped, stale = ctxs[0].step_track_results()
    assert (len(ev), dropped, stale) == (0, 0, 2) and dev.open_events() == open_before
    live.push(1, _pcm(model, 1, seed=10)[0])
    live.push(0, _pcm(model, 1, seed=11)[0])
    src, win = ctxs[1].step_live(live, B, 5, None, sync=True)
    assert list(zip(src, win)) == [(1, 2), (0, 1)]
    ev, dropped, stale = ctxs[1].step_track_results()
    assert (dropped, stale) == (0, 1)
    w = ref.update(ctxs[1].step_results(2)[0][1:], [0], [1])
    _same(ev, w)
    fl = dev.flush()[0]
    _same(fl, ref.flush())
    assert len(track_ref.concat(parts + [ev, fl])) > 0
    _same(track_ref.concat(parts + [ev, fl]), track_ref.concat(want + [w, fl]))


def test_refusals_change_nothing_and_lifetime_in_either_order(bn, model):
    n, B = int(model.config.num_species), 2
    pcm, S = _pcm(model, 8)
    rec = bn.Recording(pcm)
    x = np.full((2, n), 3.0, dtype=np.float32)
    dev = bn.Tracker(0, 2, n, ENTER)
    dev.update(x, [0, 1], [5, 5])
    with_prior = bn.Tracker(0, 2, n, ENTER, use_prior=True)
    prior = bn.Prior(0, np.full((2, n), 0.5, dtype=np.float32), THR)
    with_prior.update(x, [0, 1], [5, 5], prior=prior, sites=[0, 1])
    assert dev.open_events() == 2 * n == with_prior.open_events()
    ctx = bn.Context(model, B)
    ctx.attach_track(dev)
    ctx_p = bn.Context(model, B)                           # a BN_TRACK_PRIOR tracker on a context without a prior
    ctx_p.attach_track(with_prior)
    live3 = bn.Live(0, 3, S, S, 4 * S, 1)                  # more sources than the tracker
    for s in range(3):
        live3.push(s, pcm[s * S:(s + 1) * S])
    n_out, dr = C.c_size_t(), C.c_size_t()
    ev8 = np.empty(8, dtype=bn.EVENT_DTYPE)
    calls = [
        lambda: bn.Tracker(0, 0, n, ENTER),
        lambda: bn.Tracker(0, 2, 0, ENTER),
        lambda: bn.Tracker(0, 2, n, ENTER, max_events=0),
        lambda: bn.Tracker(0, 2, n, float("nan")),
        lambda: bn.Tracker(0, 2, n, float("-inf")),
        lambda: bn.Tracker(0, 2, n, ENTER, min_hits=0),
        lambda: bn.Tracker(0, 2, n, ENTER, flags=6),
        lambda: ctx.attach_track(bn.Tracker(0, 2, n + 1, ENTER)),              # n_species != the model's
        lambda: ctx.set_track_source(2),
        lambda: ctx.set_track_source(-1),
        lambda: bn.Context(model, B).set_track_source(0),                      # no tracker attached
        lambda: dev.update(x, [0, 2], [6, 6]),                                 # a source out of range
        lambda: dev.update(x, [0, -1], [6, 6]),
        lambda: dev.flush(2),
        lambda: dev.flush(-2),
        lambda: dev.reset(2),
        lambda: dev.reset(-1),
        lambda: dev.update(x, [0, 0], [6, 6]),                                 # rows that do not increase per source
        lambda: dev.update(x, [0, 0], [7, 6]),
        lambda: dev.update(x, [1, 0], [6, 5]),                                 # ... from the source's last window on
        lambda: dev.update(x, [0, 1], [6, 2 ** 31]),                           # window numbers are below 2^31
        lambda: with_prior.update(x, [0, 1], [6, 6]),                          # BN_TRACK_PRIOR without a prior
        lambda: with_prior.update(x, [0, 1], [6, 6], prior=prior),             # ... without sites
        lambda: with_prior.update(x, [0, 1], [6, 6], prior=prior, sites=[0, 2]),
        lambda: with_prior.update(x, [0, 1], [6, 6], prior=bn.Prior(0, np.full((2, n + 1), 0.5, dtype=np.float32), THR), sites=[0, 1]),
        lambda: ctx_p.step_windows(rec, S, 6, B, 5, None, sync=True),          # ... nor one attached
        lambda: ctx_p.step_live(live3, B, 5, None, sync=True),
        lambda: ctx.step_live(live3, B, 5, None, sync=True),                   # a pool with more sources than the tracker
        lambda: ctx.step_windows(rec, S, 0, B, 5, None, sync=True),            # first window 0 does not exceed source 0's last, 5
        lambda: ctx.step_windows(rec, S, 2, B, 5, None, sync=True),            # rows 2, 3: nor does 2
    ]
    for i, call in enumerate(calls):
        with pytest.raises(bn.EngineError) as e:
            call()
        assert e.value.status == 1 and bn.last_error(), i
        assert dev.open_events() == 2 * n == with_prior.open_events(), i
    assert live3.ready(0) == 1                             # the refused live steps took nothing from the pool
    f32p, i32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)
    src, win = np.array([0, 1], dtype=np.int32), np.array([6, 6], dtype=np.uint64)
    evp = ev8.ctypes.data_as(C.POINTER(bn.BnEvent))
    for args in ((None, 2, src.ctypes.data_as(i32p), win.ctypes.data_as(u64p), None, None, evp, 8, C.byref(n_out), C.byref(dr)),
                 (x.ctypes.data_as(f32p), 2, None, win.ctypes.data_as(u64p), None, None, evp, 8, C.byref(n_out), C.byref(dr)),
                 (x.ctypes.data_as(f32p), 2, src.ctypes.data_as(i32p), None, None, None, evp, 8, C.byref(n_out), C.byref(dr)),
                 (x.ctypes.data_as(f32p), 2, src.ctypes.data_as(i32p), win.ctypes.data_as(u64p), None, None, None, 8, C.byref(n_out), C.byref(dr)),
                 (x.ctypes.data_as(f32p), 2, src.ctypes.data_as(i32p), win.ctypes.data_as(u64p), None, None, evp, 8, None, C.byref(dr))):
        assert bn.lib.bn_track_update_host(dev._h, *args) == 1 and bn.last_error()
    assert bn.lib.bn_track_flush(dev._h, 0, None, 8, C.byref(n_out), C.byref(dr)) == 1
    assert bn.lib.bn_track_update_host(None, x.ctypes.data_as(f32p), 2, src.ctypes.data_as(i32p), win.ctypes.data_as(u64p), None, None, evp, 8,
                                       C.byref(n_out), C.byref(dr)) == 1
    assert bn.lib.bn_ctx_attach_track(None, dev._h) == 1 and bn.lib.bn_track_reset(None, 0) == 1
    assert dev.open_events() == 2 * n
    if bn.device_count() > 1:  # a tracker can only be made on a device that exists: one GPU cannot reach this refusal
        with pytest.raises(bn.EngineError) as e:
            ctx.attach_track(bn.Tracker(1, 2, n, ENTER))
        assert e.value.status == 1
    # the tracker still works as if none of that had happened: a miss in window 6 closes source 0's events of window 5
    got, _ = dev.update(np.full((1, n), -3.0, dtype=np.float32), [0], [6])
    assert len(got) == n and (got["last_window"] == 5).all() and (got["source"] == 0).all()
    # free before destroy: the context keeps the tracker alive
    c1 = bn.Context(model, B)
    t1 = bn.Tracker(0, 1, n, ENTER)
    c1.attach_track(t1)
    c1._track = None
    t1.close()
    c1.step_windows(rec, S, 0, B, 5, None, sync=True)
    ev, dropped, stale = c1.step_track_results()
    assert (dropped, stale) == (0, 0)
    c1.close()
    # destroy before free
    c2 = bn.Context(model, B)
    t2 = bn.Tracker(0, 1, n, ENTER)
    c2.attach_track(t2)
    c2.step_windows(rec, S, 1, B, 5, None, sync=False)     # in flight at destroy
    c2.close()
    opened = t2.open_events()
    assert len(t2.flush()[0]) == opened and t2.open_events() == 0
    t2.close()
