"""An index attached to a context (bn_ctx_attach_index): every step path also matches the step's embedding rows against the
snapshot, the step's own outputs and the other attachments' results stay bit for bit, and the match results are the thresholded
prefix of bn_index_search over the same embeddings.  Snapshot, shared index freed first, refusals, and the end-to-end watch list."""
import importlib

import numpy as np
import pytest

import match_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")


@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v30(num_species=300, width=0.5, depth=0.5, emb=256)))


def _pcm(model, n_windows, seed=0):
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    x = synth.synthetic_segments(1, S * n_windows, sr)[0]
    rng = np.random.default_rng(seed)
    return np.clip(x + 0.05 * rng.standard_normal(len(x)), -1, 1).astype(np.float32), S


def _varied_pcm(model, n_windows, seed):
    """windows that differ from each other strongly (tones of random pitch, noise of random level), so that their embeddings do"""
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    rng = np.random.default_rng(seed)
    t = np.arange(S) / sr
    wins = []
    for w in range(n_windows):
        if w % 2:
            x = sum(rng.uniform(0.1, 0.4) * np.sin(2 * np.pi * f * t + rng.uniform(0, 6)) for f in rng.uniform(300, 9000, 1 + w % 4))
        else:
            x = rng.uniform(0.02, 0.5) * rng.standard_normal(S) * np.sin(2 * np.pi * rng.uniform(0.2, 3) * t) ** 2
        wins.append(x)
    return np.clip(np.concatenate(wins), -1, 1).astype(np.float32), S


def _library(bn, rng, n, dim=256, capacity=None, tagged=True):
    idx = bn.Index(0, dim, capacity or n)
    idx.add((rng.standard_normal((n, dim)) * rng.uniform(0.1, 10, (n, 1))).astype(np.float32))
    if tagged:
        idx.set_tags(0, rng.integers(1, 65536, n).astype(np.uint32))
    return idx


def _same_bytes(got, want):
    for a, w in zip(got, want):
        assert a.tobytes() == w.tobytes()


def _check_match(idx, emb, got, top_m, min_score):
    """got == the thresholded prefix of bn_index_search over the embeddings, for a snapshot that holds all of idx"""
    assert got[4] == len(idx)
    want = match_ref.prefix(*idx.search(emb, top_m), min_score=min_score, tags=idx.tags())
    why = match_ref.same(got[:4], want)
    assert why is None, why


def test_step_paths_outputs_unchanged_and_match_results(bn, model):
    rng = np.random.default_rng(2)
    B, M = 6, 10
    eo = model.config.embedding_output
    idx = _library(bn, rng, 1000)
    pcm, S = _pcm(model, 2 * B)
    rec = bn.Recording(pcm)
    plain, ctx = bn.Context(model, B), bn.Context(model, B)
    plain.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    emb0 = plain.read_output(eo, B)
    t = float(np.median(idx.search(emb0, M)[1]))          # cuts inside the lists
    ctx.attach_index(idx, top_m=M, min_score=t)
    with pytest.raises(bn.EngineError) as e:
        ctx.step_index_results(B)                          # no step since the attach
    assert e.value.status == 1 and "no step has run" in bn.last_error()
    cut = 0
    for first, m in ((0, B), (B, B - 2)):
        plain.step_windows(rec, S, first, m, 10, 0.01, sync=True)
        want, wemb = plain.step_results(m), plain.read_output(eo, m)
        ctx.step_windows(rec, S, first, m, 10, 0.01, sync=True)
        _same_bytes(ctx.step_results(m), want)
        emb = ctx.read_output(eo, m)
        assert emb.tobytes() == wemb.tobytes()
        res = ctx.step_index_results(m)
        assert res[0].shape == (m, M) and res[0].dtype == np.uint64
        _check_match(idx, emb, res, M, t)
        cut += int((res[3] < M).sum())
        # bn_step_device on the context's own input buffer, asynchronous
        ctx.step_device(ctx.input_device()[0], m, 10, 0.01, sync=False)
        ctx.synchronize()
        _same_bytes(ctx.step_results(m), want)
        _same_bytes(ctx.step_index_results(m)[:4], res[:4])
    assert cut > 0
    # bn_step_live
    live = bn.Live(0, 2, S, S, 4 * S, 1)
    live.push(0, pcm[:2 * S])
    live.push(1, pcm[2 * S:4 * S])
    src, win = ctx.step_live(live, B, 10, 0.01, sync=True)
    assert len(src) == 4
    order = [int(s) * 2 + int(w) for s, w in zip(src, win)]
    plain.step_windows(rec, S, 0, 4, 10, 0.01, sync=True)
    for a, w in zip(ctx.step_results(4), plain.step_results(4)):
        assert a.tobytes() == w[order].tobytes()
    _check_match(idx, ctx.read_output(eo, 4), ctx.step_index_results(4), M, t)
    assert ctx.stats()["capture_fallbacks"] == 0 and plain.stats()["capture_fallbacks"] == 0 and ctx.stats()["replays"] > 0
    # detach restores the plain step
    ctx.attach_index(None)
    ctx.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    plain.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    _same_bytes(ctx.step_results(B), plain.step_results(B))
    with pytest.raises(bn.EngineError) as e:
        ctx.step_index_results(B)
    assert e.value.status == 1


def test_two_query_passes_in_one_step(bn, model):
    """B = 70 on a context of max_batch 80: the scan's grid has two query passes"""
    rng = np.random.default_rng(3)
    B, M = 70, 10
    eo = model.config.embedding_output
    idx = _library(bn, rng, 4097 + 64)
    pcm, S = _pcm(model, B, seed=2)
    rec = bn.Recording(pcm)
    plain, ctx = bn.Context(model, 80), bn.Context(model, 80)
    ctx.attach_index(idx, top_m=M)
    plain.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    ctx.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
    _same_bytes(ctx.step_results(B), plain.step_results(B))
    emb = ctx.read_output(eo, B)
    assert emb.tobytes() == plain.read_output(eo, B).tobytes()
    res = ctx.step_index_results(B)
    _check_match(idx, emb, res, M, None)
    assert np.all(res[3] == M)
    # the entry point does not matter: bn_index_match on the same embeddings
    assert match_ref.same(idx.match(emb, M), res[:4]) is None
    assert ctx.stats()["capture_fallbacks"] == 0


def test_all_four_attachments_together(bn, model):
    rng = np.random.default_rng(4)
    n, dim, B = int(model.config.num_species), int(model.config.embedding_dim), 5
    pcm, S = _pcm(model, B, seed=3)
    rec = bn.Recording(pcm)
    head = bn.Head(0, rng.standard_normal((9, dim)).astype(np.float32), None, l2norm=True)
    prior = bn.Prior(0, rng.uniform(0.2, 1, (2, n)).astype(np.float32), 0.3)
    idx = _library(bn, rng, 500)
    trackers = [bn.Tracker(0, 2, n, 0.05, 1, 0) for _ in range(2)]

    def run(with_head, with_prior, with_track, with_index):
        c = bn.Context(model, B)
        if with_head:
            c.attach_head(head, top_k=3)
        if with_prior:
            c.attach_prior(prior, top_k=4)
        if with_track is not None:
            c.attach_track(trackers[with_track])
        if with_index:
            c.attach_index(idx, top_m=7, min_score=0.0)
        c.step_windows(rec, S, 0, B, 10, 0.01, sync=True)
        assert c.stats()["capture_fallbacks"] == 0
        return c

    every = run(True, True, 0, True)
    own = every.step_results(B)
    _same_bytes(own, run(False, False, None, False).step_results(B))
    _same_bytes(every.step_head_results(B), run(True, False, None, False).step_head_results(B))
    _same_bytes(every.step_prior_results(B), run(False, True, None, False).step_prior_results(B))
    ev, dropped, stale = every.step_track_results()
    ev1, dropped1, stale1 = run(False, False, 1, False).step_track_results()
    assert ev.tobytes() == ev1.tobytes() and (dropped, stale) == (dropped1, stale1)
    alone = run(False, False, None, True)
    res = every.step_index_results(B)
    _same_bytes(res[:4], alone.step_index_results(B)[:4])
    _check_match(idx, every.read_output(model.config.embedding_output, B), res, 7, 0.0)


def test_snapshot_and_reattach(bn, model):
    rng = np.random.default_rng(5)
    B, M, n0 = 4, 5, 300
    eo = model.config.embedding_output
    idx = _library(bn, rng, n0, capacity=1000)
    frozen = _library(bn, np.random.default_rng(5), n0)    # the same first n0 rows, and never more
    pcm, S = _varied_pcm(model, B, seed=4)
    rec = bn.Recording(pcm)
    ctx = bn.Context(model, B)
    ctx.attach_index(idx, top_m=M)
    ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
    emb = ctx.read_output(eo, B)
    before = ctx.step_index_results(B)
    first = idx.add(emb)                                    # copies of the queries: each would be its query's first hit
    assert first == n0 and len(idx) == n0 + B
    idx.fill_tags(first, B, 77)
    ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
    after = ctx.step_index_results(B)
    assert after[4] == n0 and np.all(after[0] < n0)
    _same_bytes(after[:4], before[:4])
    # the same library as a prefix of a larger index gives the same bytes as on its own
    assert match_ref.same(frozen.match(emb, M), after[:4]) is None
    ctx.attach_index(idx, top_m=M)                          # a new snapshot
    ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
    again = ctx.step_index_results(B)
    assert again[4] == n0 + B
    print("snapshot: first hits", again[0][:, 0], "scores", again[1][:, :2])
    assert np.array_equal(again[0][:, 0], first + np.arange(B)) and np.all(again[2][:, 0] == 77)
    _check_match(idx, emb, again, M, None)
    # an empty snapshot: every count 0
    empty = bn.Index(0, 256, 8)
    ctx.attach_index(empty, top_m=M)
    ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
    res = ctx.step_index_results(B)
    assert res[4] == 0 and np.all(res[3] == 0)


def test_two_contexts_share_an_index_freed_first(bn, model):
    rng = np.random.default_rng(6)
    B, eo = 4, model.config.embedding_output
    idx = _library(bn, rng, 700)
    keep = _library(bn, np.random.default_rng(6), 700)      # the same rows and tags, for the expected results
    pcm, S = _pcm(model, 2 * B, seed=5)
    rec = bn.Recording(pcm)
    c1, c2 = bn.Context(model, B), bn.Context(model, B)
    c1.attach_index(idx, top_m=256)
    c2.attach_index(idx, top_m=3, min_score=0.05)
    c1._index = c2._index = None
    idx.close()                                             # the contexts keep the slab alive
    for _ in range(2):
        c1.step_windows(rec, S, 0, B, 10, None, sync=False)
        c2.step_windows(rec, S, B, B, 10, None, sync=False)
        c1.synchronize()
        c2.synchronize()
        _check_match(keep, c1.read_output(eo, B), c1.step_index_results(B), 256, None)
        _check_match(keep, c2.read_output(eo, B), c2.step_index_results(B), 3, 0.05)
    c1.close()
    c2.close()


def test_refusals_leave_the_attachment_in_place(bn, model):
    rng = np.random.default_rng(7)
    B, M, eo = 2, 4, model.config.embedding_output
    idx = _library(bn, rng, 200)
    pcm, S = _pcm(model, B, seed=6)
    rec = bn.Recording(pcm)
    ctx = bn.Context(model, B)
    ctx.attach_index(idx, top_m=M, min_score=-1.0)
    v24 = bn.Model(write_model(synth.birdnet_v24(num_species=64, width=0.25, depth=0.25, head=64)))
    calls = [
        (lambda: bn.Context(v24, 2).attach_index(bn.Index(0, 64, 4)), "no embedding output"),
        (lambda: ctx.attach_index(bn.Index(0, 255, 4)), "differs from the model's embedding_dim"),
        (lambda: ctx.attach_index(idx, top_m=0), "top_m must be in 1..256"),
        (lambda: ctx.attach_index(idx, top_m=257), "top_m must be in 1..256"),
        (lambda: ctx.attach_index(idx, top_m=M, min_score=float("nan")), "finite"),
        (lambda: ctx.attach_index(idx, top_m=M, min_score=float("-inf")), "finite"),
    ]
    if bn.device_count() > 1:  # an index can only be made on a device that exists: one GPU cannot reach this refusal
        calls.append((lambda: ctx.attach_index(bn.Index(1, 256, 4)), "the index on"))
    for call, word in calls:
        with pytest.raises(bn.EngineError) as e:
            call()
        assert e.value.status == 1 and word in bn.last_error(), word
        ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
        _check_match(idx, ctx.read_output(eo, B), ctx.step_index_results(B), M, -1.0)


def test_end_to_end_watch_list(bn, model):
    cfg = model.config
    S, B, n_win = int(cfg.sample_count), 4, 10
    pcm, _ = _varied_pcm(model, n_win, seed=8)
    rec = bn.Recording(pcm)
    ctx = bn.Context(model, B)
    idx = bn.Index(0, int(cfg.embedding_dim), n_win)
    batches = [(0, 4), (4, 4), (8, 2)]
    for k, (first, m) in enumerate(batches):
        ctx.step_windows(rec, S, first, m, 10, None, sync=True)
        assert idx.add_context(ctx, m) == first
        idx.fill_tags(first, m, 100 + k)
    stored = idx.read()
    valid = np.abs(stored).sum(axis=1) > 0
    assert valid.any()
    ctx.attach_index(idx, top_m=3, min_score=0.5)
    for k, (first, m) in enumerate(batches):
        ctx.step_windows(rec, S, first, m, 10, None, sync=True)
        ids, scores, tags, counts, n = ctx.step_index_results(m)
        assert n == n_win
        probe = bn.Index(0, int(cfg.embedding_dim), m)      # the queries' normalised bits: what an append of them stores
        probe.add(ctx.read_output(cfg.embedding_output, m))
        qn = probe.read()
        for i in range(m):
            if not valid[first + i]:
                assert counts[i] == 0
                continue
            assert counts[i] >= 1
            hit = int(ids[i, 0])
            print("window", first + i, "first hit", hit, "scores", scores[i, :counts[i]])
            assert stored[hit].tobytes() == qn[i].tobytes()
            assert tags[i, 0] == 100 + [b for b, (f, n_b) in enumerate(batches) if f <= hit < f + n_b][0]
