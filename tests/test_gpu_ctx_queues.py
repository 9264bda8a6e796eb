"""The stream a context runs its plans on is created at a priority level of its own (capi.cpp, create_plan_stream): the runtime keeps
one pool of hardware queues per level, so four contexts no longer share the default level's GPU_MAX_HW_QUEUES queues with the null
stream.  What is checked here is that the level is the one chosen, that BN_CTX_STREAM_PRIO=0 restores the default level, and that the
level changes scheduling only -- never a bit of a result and never a capture.  No test asserts a time: the speed is in DESIGN.md 5.

Every case is a fresh child process, because the queue budget and the switch are read once per process.  Two children serve all
three tests (module fixture): both run under GPU_MAX_HW_QUEUES=4, touch the null stream with one torch copy, then create four
contexts of the tiny v2.4 model at batch 2.
  child "rr"     (switch unset): 8 asynchronous steps with distinct inputs round-robin over the four contexts, four in flight at a time
  child "serial" (BN_CTX_STREAM_PRIO=0): the same 8 inputs one by one, synchronously, on the first context alone
Then each child steps one further context with a head and a prior attached (both enqueue on the context's stream).  A v2.4 model has
no embedding output for a head to read, so that context is of the tiny v3.0 model the step-row tests use.
hipStreamGetPriority / hipDeviceGetStreamPriorityRange are called through the library's own ctypes handle, which resolves them in the
HIP runtime the library is linked to -- the one that made the streams."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CTX, BATCH, STEPS, TOP_K = 4, 2, 8, 5

CHILD = textwrap.dedent('''
    import ctypes as C, importlib, os, sys
    import numpy as np
    import torch
    root, out, mode = sys.argv[1:4]
    sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
    from gpu_helpers import write_model
    N_CTX, BATCH, STEPS, TOP_K = 4, 2, 8, 5
    torch.zeros(64).cuda().add_(1.0); torch.cuda.synchronize()          # the null stream has its hardware queue before any context
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
    hip = bn.lib                                                          # dlsym on the library's handle reaches the runtime it links
    hip.hipStreamGetPriority.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    hip.hipDeviceGetStreamPriorityRange.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int)]
    least, greatest = C.c_int(77), C.c_int(77)
    assert hip.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest)) == 0
    def priority(ctx):
        p = C.c_int(77)
        assert ctx.stream() and hip.hipStreamGetPriority(C.c_void_p(ctx.stream()), C.byref(p)) == 0
        return p.value
    res = {"range": np.array([least.value, greatest.value])}

    model = bn.Model(write_model(synth.birdnet_v24(num_species=64, width=0.25, depth=0.25, head=64)))
    S = int(model.config.sample_count)
    x = torch.from_numpy(synth.synthetic_segments(STEPS * BATCH, S, int(model.config.sample_rate))).cuda().view(STEPS, BATCH, S)
    ctxs = [bn.Context(model, BATCH) for _ in range(N_CTX)]
    res["prio"] = np.array([priority(c) for c in ctxs])
    def keep(i, c):
        for name, a in zip(("lg", "ix", "cf", "ct"), c.step_results(BATCH)):
            res[f"s{i}_{name}"] = a
    if mode == "rr":
        for first in range(0, STEPS, N_CTX):
            for j in range(N_CTX):
                ctxs[j].step_device(x[first + j].data_ptr(), BATCH, TOP_K)
            for j in range(N_CTX):
                ctxs[j].synchronize()
                keep(first + j, ctxs[j])
    else:
        for i in range(STEPS):
            ctxs[0].step_device(x[i].data_ptr(), BATCH, TOP_K, sync=True)
            keep(i, ctxs[0])
    res["fallbacks"] = np.array([c.stats()["capture_fallbacks"] for c in ctxs])
    res["captures"] = np.array([c.stats()["captures"] for c in ctxs])
    res["replays"] = np.array([c.stats()["replays"] for c in ctxs])

    m30 = bn.Model(write_model(synth.birdnet_v30(num_species=70, width=0.25, depth=0.25, emb=64)))
    dim, n, S30 = int(m30.config.embedding_dim), int(m30.config.num_species), int(m30.config.sample_count)
    rng = np.random.default_rng(3)
    head = bn.Head(0, rng.standard_normal((9, dim)).astype(np.float32), None)
    table = rng.uniform(0, 1, (2, n)).astype(np.float32)
    prior = bn.Prior(0, table, 0.3, rerank=True)
    hp = bn.Context(m30, BATCH)
    hp.attach_head(head, top_k=4)
    hp.attach_prior(prior, top_k=6)
    hp.set_prior_site(1)
    x30 = torch.from_numpy(synth.synthetic_segments(BATCH, S30, int(m30.config.sample_rate))).cuda()
    hp.step_device(x30.data_ptr(), BATCH, TOP_K, sync=True)
    res["hp_prio"] = np.array([priority(hp)])
    res["hp_fallbacks"] = np.array([hp.stats()["capture_fallbacks"]])
    for what, arrays in (("step", hp.step_results(BATCH)), ("head", hp.step_head_results(BATCH)), ("prior", hp.step_prior_results(BATCH))):
        for k, a in enumerate(arrays):
            res[f"hp_{what}{k}"] = a
    np.savez(out, **res)
    print("CTX_QUEUES_OK")
''')


def _child(tmp, mode, switch):
    out = str(tmp / f"{mode}.npz")
    env = {k: v for k, v in os.environ.items() if k != "BN_CTX_STREAM_PRIO"}
    env["GPU_MAX_HW_QUEUES"] = "4"
    if switch is not None:
        env["BN_CTX_STREAM_PRIO"] = switch
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, out, mode], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "CTX_QUEUES_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ctx_queues")
    return {"rr": _child(tmp, "rr", None), "serial": _child(tmp, "serial", "0")}


def test_context_streams_are_created_at_the_chosen_level(runs):
    least, greatest = (int(v) for v in runs["rr"]["range"])
    assert greatest <= 0 <= least, "the default level 0 lies outside the device's range"
    # the level chosen is the greatest priority (lower numbers are greater); a device with one level keeps the default
    want = greatest if least != greatest else 0
    assert runs["rr"]["prio"].tolist() == [want] * N_CTX and runs["rr"]["hp_prio"].tolist() == [want]
    if least != greatest:
        assert want != 0
    assert runs["serial"]["prio"].tolist() == [0] * N_CTX and runs["serial"]["hp_prio"].tolist() == [0]


def test_the_level_changes_scheduling_only(runs):
    rr, serial = runs["rr"], runs["serial"]
    for i in range(STEPS):
        for name in ("lg", "ix", "cf", "ct"):
            g, w = rr[f"s{i}_{name}"], serial[f"s{i}_{name}"]
            assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), (i, name)
        assert rr[f"s{i}_lg"].shape[0] == BATCH and np.isfinite(rr[f"s{i}_lg"]).all() and (rr[f"s{i}_ct"] == TOP_K).all()
    # distinct inputs gave distinct results: a step that read a sibling's buffers would show
    assert len({rr[f"s{i}_lg"].tobytes() for i in range(STEPS)}) == STEPS
    assert int(rr["fallbacks"].sum()) == 0 and int(serial["fallbacks"].sum()) == 0
    # every context captured its graph once and took its share of the steps through it
    assert rr["captures"].tolist() == [1] * N_CTX and rr["replays"].tolist() == [STEPS // N_CTX] * N_CTX


def test_head_and_prior_on_the_contexts_stream_give_the_same_rows(runs):
    rr, serial = runs["rr"], runs["serial"]
    names = sorted(k for k in rr if k.startswith(("hp_step", "hp_head", "hp_prior")))
    assert len(names) == 4 + 4 + 3
    counts = {"hp_prior": rr["hp_prior2"]}
    assert rr["hp_prior2"].tobytes() == serial["hp_prior2"].tobytes()
    for k in names:
        g, w = rr[k], serial[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        if k in ("hp_prior0", "hp_prior1"):  # a prior's row holds counts[r] entries; what lies past them is not a result
            for r, c in enumerate(counts["hp_prior"]):
                assert g[r, :c].tobytes() == w[r, :c].tobytes(), (k, r)
        else:
            assert g.tobytes() == w.tobytes(), k
    assert int(rr["hp_fallbacks"][0]) == 0 and int(serial["hp_fallbacks"][0]) == 0
