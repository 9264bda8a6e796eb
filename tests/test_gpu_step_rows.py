"""The packed top-K rows [idx: b*k][conf: b*k][count: b] of a step, of an attached head and of an attached prior, and their way
into pinned memory, compared byte for byte.

Shapes: max_batch 4 and 3 windows (batch < max_batch, so an offset computed from max_batch lands in the wrong place), the step's
k = 5 (batch * k odd: the confidence and count regions start at odd word offsets), then k = 40 -- past the 32 a context allocates at
creation, so the step's block and an AFTER_TOPK prior's block grow behind a drain -- then 5 again in the grown blocks.  The second
test runs the same step with the results copied by the copy engine (BN_SDMA_COPY=1) instead of the store kernel."""
import importlib
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import prior_ref
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
