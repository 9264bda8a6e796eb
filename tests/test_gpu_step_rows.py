"""The packed top-K rows [idx: b*k][conf: b*k][count: b] of a step, of an attached head and of an attached prior, and their way
into pinned memory, compared byte for byte.

Shapes: max_batch 4 and 3 windows (batch < max_batch, so an offset computed from max_batch lands in the wrong place), the step's
k = 5 (batch * k odd: the confidence and count regions start at odd word offsets), then k = 40 -- past the 32 a context allocates at
creation, so the step's block and an AFTER_TOPK prior's block grow behind a drain -- then 5 again in the grown blocks.  The second
test runs the same step with the results copied by the copy engine (BN_SDMA_COPY=1) instead of the store kernel.

The last three tests are about the identity of a step's rows (source, window, site) on a context with a prior under a site map and a
tracker under BN_TRACK_PRIOR attached: max_batch 4, 2 sites, 3 sources on sites (1, 0, 1), the context's own site 0, so a row that
ran at the wrong site differs.  Every prior row is compared with prior_ref and every event list with track_ref, byte for byte."""
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import prior_ref
import track_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
THR, MAX_BATCH, B = 0.3, 4, 3


def _same(got, want, what):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, g, w)


def test_blocks_grow_and_shrink_without_moving_a_byte(bn):
    model = bn.Model(write_model(synth.birdnet_v30(num_species=70, width=0.25, depth=0.25, emb=64)))
    dim, n, S = int(model.config.embedding_dim), int(model.config.num_species), int(model.config.sample_count)
    rng = np.random.default_rng(3)
    head = bn.Head(0, rng.standard_normal((9, dim)).astype(np.float32), None)
    table = rng.uniform(0, 1, (2, n)).astype(np.float32)
    table[rng.uniform(size=table.shape) < 0.2] = prior_ref.UNKNOWN
    prior = bn.Prior(0, table, THR, after_topk=True, rerank=True)
    x = synth.synthetic_segments(1, S * B, int(model.config.sample_rate))[0]
    pcm = np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)

    def context():
        c = bn.Context(model, MAX_BATCH)
        c.attach_head(head, top_k=4)
        c.attach_prior(prior)
        c.set_prior_site(1)
        return c

    def step(c, k):
        c.step_windows(rec, S, 0, B, k, None, sync=True)
        return c.step_results(B), c.step_head_results(B), c.step_prior_results(B)

    ctx = context()
    stepped = []
    for k in (5, 40, 5):
        got = step(ctx, k)
        want = step(context(), k)
        for g, w, name in zip(got, want, ("step", "head", "prior")):
            _same(g, w, (name, k))
        assert got[0][1].shape == (B, k) and got[1][1].shape == (B, 4) and got[2][0].shape == (B, k)
        assert got[0][3].tolist() == [k] * B and got[1][3].tolist() == [4] * B
        _same(got[2], prior_ref.apply(got[0][0], table, [1] * B, THR, k, None, True, True), ("prior_ref", k))
        stepped.append(got[0])
    # the same three batches as host slices: the slot's pinned block grows and is reused the same way
    segs = pcm.reshape(B, S)
    for k, want in zip((5, 40, 5), stepped):
        logits, emb, idx, conf, cnt = ctx.collect(ctx.submit(segs, k, None))
        _same((logits, idx, conf, cnt), want, ("submit/collect", k))
    assert ctx.stats()["capture_fallbacks"] == 0


CHILD = textwrap.dedent('''
    import importlib, os, sys
    import numpy as np
    sys.path.insert(0, os.environ["BN_TEST_ROOT"]); sys.path.insert(0, os.path.join(os.environ["BN_TEST_ROOT"], "tests"))
    import prior_ref
    from gpu_helpers import write_model
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
    model = bn.Model(write_model(synth.birdnet_v30(num_species=70, width=0.25, depth=0.25, emb=64)))
    dim, n, S = int(model.config.embedding_dim), int(model.config.num_species), int(model.config.sample_count)
    rng = np.random.default_rng(3)
    head = bn.Head(0, rng.standard_normal((9, dim)).astype(np.float32), None)
    table = rng.uniform(0, 1, (2, n)).astype(np.float32)
    table[rng.uniform(size=table.shape) < 0.2] = prior_ref.UNKNOWN
    x = synth.synthetic_segments(1, S * 3, int(model.config.sample_rate))[0]
    pcm = np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32)
    ctx = bn.Context(model, 4)
    ctx.attach_head(head, top_k=4)
    ctx.attach_prior(bn.Prior(0, table, 0.3, rerank=True), top_k=6)
    ctx.set_prior_site(1)
    ctx.step_windows(bn.Recording(pcm), S, 0, 3, 5, None, sync=True)
    out = {}
    for name, arrays in (("step", ctx.step_results(3)), ("head", ctx.step_head_results(3)), ("prior", ctx.step_prior_results(3))):
        for i, a in enumerate(arrays):
            out[f"{name}{i}"] = a
    want = prior_ref.apply(out["step0"], table, [1] * 3, 0.3, 6, None, False, True)
    assert all(out[f"prior{i}"].tobytes() == w.tobytes() for i, w in enumerate(want)), "prior rows differ from prior_ref"
    assert ctx.stats()["capture_fallbacks"] == 0
    np.savez(sys.argv[1], **out)
    print("STEP_ROWS_OK", len(out))
''')


def test_copy_engine_fallback_delivers_the_same_bytes(tmp_path):
    """BN_SDMA_COPY is read once per process: one fresh child per setting, the second only after the first came back clean."""
    files = []
    for sdma in (True, False):
        path = str(tmp_path / f"rows_sdma{int(sdma)}.npz")
        env = dict(os.environ, BN_TEST_ROOT=ROOT)
        env.pop("BN_SDMA_COPY", None)
        if sdma:
            env["BN_SDMA_COPY"] = "1"
        r = subprocess.run([sys.executable, "-c", CHILD, path], capture_output=True, text=True, env=env, timeout=240)
        assert r.returncode == 0 and "STEP_ROWS_OK 11" in r.stdout, (sdma, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        files.append(np.load(path))
    a, b = files
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 11
    for name in a.files:
        assert a[name].shape == b[name].shape and a[name].dtype == b[name].dtype and a[name].tobytes() == b[name].tobytes(), name


# ---- the identity of a step's rows ----------------------------------------------------------------------------------
SOURCE_SITES = (1, 0, 1)
N_SRC, STEP_K, PRIOR_K = 3, 5, 3


@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v24(num_species=70, width=0.25, depth=0.25, head=32)))


@pytest.fixture(scope="module")
def audio(bn, model):
    """(pcm of 8 windows per source and one recording, S, table, enter_conf): the table has two sites, enter_conf makes about a
    fifth of a probe batch's confidences hits before the prior's rerank."""
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    n = int(model.config.num_species)
    rng = np.random.default_rng(11)
    pcm = [np.clip(synth.synthetic_segments(1, S * 8, sr)[0] + 0.05 * rng.standard_normal(S * 8), -1, 1).astype(np.float32) for _ in range(N_SRC + 1)]
    table = rng.uniform(0.2, 1, (2, n)).astype(np.float32)
    table[rng.uniform(size=table.shape) < 0.2] = prior_ref.UNKNOWN
    probe = bn.Context(model, MAX_BATCH)
    probe.step_windows(bn.Recording(pcm[0]), S, 0, MAX_BATCH, STEP_K, None, sync=True)
    enter = 0.7 * float(np.quantile(prior_ref.sigmoid_row(probe.step_results(MAX_BATCH)[0]), 0.8))
    return pcm, S, table, enter


class _Rig:
    """Contexts with one shared prior (site map) and one shared tracker attached, the references next to them, and one pool."""

    def __init__(self, bn, model, audio, after=False, n_ctx=1, source_sites=SOURCE_SITES):
        self.bn, self.after = bn, after
        self.pcm, self.S, self.table, enter = audio
        n = int(model.config.num_species)
        self.prior = bn.Prior(0, self.table, THR, after_topk=after, rerank=True)
        self.dev = bn.Tracker(0, N_SRC, n, enter, 1, 0, use_prior=True)
        self.ref = track_ref.Tracker(N_SRC, n, enter, 1, 0, prior=(self.table, THR, True))
        self.ctxs = [bn.Context(model, MAX_BATCH) for _ in range(n_ctx)]
        for c in self.ctxs:
            c.attach_prior(self.prior, source_sites=list(source_sites), top_k=PRIOR_K)
            c.attach_track(self.dev)
        self.ctx = self.ctxs[0]
        self.live = bn.Live(0, N_SRC, self.S, self.S, 8 * self.S, 1)
        self.pushed = [0] * N_SRC
        self.events = []

    def push(self, source, windows=1):
        a = self.pushed[source] * self.S
        self.live.push(source, self.pcm[source][a:a + windows * self.S])
        self.pushed[source] += windows

    def check(self, ctx, m, sites, sources=None, windows=None):
        """The last step of ctx (complete): its prior rows at `sites`; with sources, its events.  Returns (prior rows, events)."""
        logits = ctx.step_results(m)[0]
        k, after = (STEP_K, True) if self.after else (PRIOR_K, False)
        rows = ctx.step_prior_results(m)
        _same(rows, prior_ref.apply(logits, self.table, sites, THR, k, None, after, True), ("prior rows", sites))
        if sources is None:
            return rows, None
        ev, dropped, stale = ctx.step_track_results()
        want = self.ref.update(logits, sources, windows, sites=sites)
        assert (dropped, stale) == (0, 0) and ev.tobytes() == want.tobytes(), (sources, windows, ev, want)
        self.events.append(ev.copy())
        return rows, ev

    def live_step(self, ctx, max_windows, sync=True):
        src, win = ctx.step_live(self.live, max_windows, STEP_K, None, sync=sync)
        return [int(s) for s in src], [int(w) for w in win]

    def check_live(self, ctx, src, win):
        return self.check(ctx, len(src), [SOURCE_SITES[s] for s in src], src, win)

    def finish(self):
        """Flush compared; every event of the run, sorted."""
        fl = self.dev.flush()[0]
        assert fl.tobytes() == self.ref.flush().tobytes()
        assert all(c.stats()["capture_fallbacks"] == 0 for c in self.ctxs)
        return track_ref.concat(self.events + [fl])


@pytest.mark.parametrize("after", [False, True])
def test_no_row_identity_survives_a_call(bn, model, audio, after):
    rig = _Rig(bn, model, audio, after)
    ctx, S = rig.ctx, rig.S
    rec = bn.Recording(rig.pcm[N_SRC])
    for s in range(N_SRC):
        rig.push(s)
    src, win = rig.live_step(ctx, MAX_BATCH)                # 3 rows of 3 sources, at the mapped sites
    assert sorted(src) == [0, 1, 2] and win == [0, 0, 0]
    rig.check_live(ctx, src, win)
    ctx.set_track_source(2)                                # windows 5, 6 of source 2, at the context's site: closes its events of window 0
    ctx.step_windows(rec, S, 5, 2, STEP_K, None, sync=True)
    _, ev = rig.check(ctx, 2, [0, 0], [2, 2], [5, 6])
    before = (ev.tobytes(), ctx.step_track_results()[1:], [rig.dev.open_events(s) for s in (-1, 0, 1, 2)])
    ctx.step_device(ctx.input_device()[0], 3, STEP_K, None, sync=True)   # as many rows as the live step: at the context's site, untracked
    rig.check(ctx, 3, [0, 0, 0])
    got = ctx.step_track_results()
    assert (got[0].tobytes(), got[1:], [rig.dev.open_events(s) for s in (-1, 0, 1, 2)]) == before
    rig.push(1)
    rig.push(0)
    src, win = rig.live_step(ctx, MAX_BATCH)
    assert sorted(src) == [0, 1] and win == [1, 1]
    rig.check_live(ctx, src, win)
    assert len(rig.finish()) > 0


STEP_ROWS = (3, 1, 2, 3, 1, 2, 3, 2, 1)                     # nine steps: more than two trips round the four pinned blocks


def _nine_steps(rig):
    """The nine live steps with sync=0, issued round robin over rig.ctxs; a step's results are read, behind a synchronize of its own
    context only, after the NEXT step has been enqueued (on the other context, if there are two).  Returns the prior rows per step."""
    for _ in range(sum(STEP_ROWS) // N_SRC):
        for s in range(N_SRC):
            rig.push(s)                                    # the queue holds the sources' windows interleaved
    rows, waiting = [], None

    def read(ctx, src, win):
        ctx.synchronize()
        rows.append(rig.check_live(ctx, src, win)[0])

    for i, m in enumerate(STEP_ROWS):
        ctx = rig.ctxs[i % len(rig.ctxs)]
        if waiting is not None and waiting[0] is ctx:       # one context: its results would be overwritten by the next step
            read(*waiting)
            waiting = None
        src, win = rig.live_step(ctx, m, sync=False)
        assert len(src) == m
        if waiting is not None:
            read(*waiting)
        waiting = (ctx, src, win)
    read(*waiting)
    return rows


def test_the_ring_wraps(bn, model, audio):
    one = _Rig(bn, model, audio)
    rows_one = _nine_steps(one)
    events_one = one.finish()
    assert len(events_one) > 0
    two = _Rig(bn, model, audio, n_ctx=2)
    rows_two = _nine_steps(two)
    for a, b in zip(rows_one, rows_two):
        _same(a, b, "prior rows of one context and of two")
    assert two.finish().tobytes() == events_one.tobytes()


def test_a_refused_step_leaves_nothing_behind(bn, model, audio):
    S = audio[1]
    live4 = bn.Live(0, N_SRC + 1, S, S, 4 * S, 1)           # more sources than the site map and than the tracker
    for s in range(N_SRC + 1):
        live4.push(s, audio[0][s][:S])
    rec = bn.Recording(audio[0][N_SRC])

    def run(refused, source_sites=SOURCE_SITES):
        rig = _Rig(bn, model, audio, source_sites=source_sites)
        ctx = rig.ctx
        for _ in range(2):
            for s in range(N_SRC):
                rig.push(s)                                # the first step takes window 0 of every source
        out = [rig.check_live(ctx, *rig.live_step(ctx, 3))]
        if refused is not None:
            call, message = refused
            held = (ctx.step_track_results()[0].tobytes(), rig.dev.open_events(), rig.live.ready(0), live4.ready(0))
            with pytest.raises(bn.EngineError) as e:
                call(rig)
            assert e.value.status == 1 and bn.last_error() == message
            assert (ctx.step_track_results()[0].tobytes(), rig.dev.open_events(), rig.live.ready(0), live4.ready(0)) == held
        out.append(rig.check_live(ctx, *rig.live_step(ctx, 2)))
        ctx.set_track_source(1)
        ctx.step_windows(rec, S, 4, 2, STEP_K, None, sync=True)
        out.append(rig.check(ctx, 2, [0, 0], [1, 1], [4, 5]))
        return [[a.tobytes() for a in rows] + [ev.tobytes()] for rows, ev in out], rig.finish().tobytes()

    want = run(None)
    pool = lambda rig: rig.ctx.step_live(live4, 3, STEP_K, None, sync=True)
    windows = lambda rig: rig.ctx.step_windows(rec, S, 0, 2, STEP_K, None, sync=True)   # the context's source 0 has seen window 0
    assert run((pool, "the pool has 4 sources, the attached prior's site map 3")) == want
    assert run((pool, "the pool has 4 sources, the attached tracker 3"), SOURCE_SITES + (0,)) == want
    assert run((windows, "window 0 does not exceed the last tracked window 0 of source 0")) == want
