"""bn_step_window_list / bn_recording_window_list on the GPU: a step over an explicit list of (recording, start) rows against
bn_step_windows over the same samples, byte for byte.

The tiny synthetic v2.4 model (S = 144000), windows at step S / 4.  Four recordings of 13 windows each, the last three windows
padded: I16 mono, F32 mono, stereo I24 mixed down, and one created resampled (32 kHz -> 48 kHz; mono f32 once it exists, so it
shares the F32 mono reader).  Lists of 8 contiguous rows, 9 scrambled rows of the four recordings (three readers), one list over the
four other interleaved readers (I16, F32, I32, U8), unaligned starts, 129 rows (the second launch of a reader), gated subsets with
a tracker, the gated loop end to end over a recording of silence with three bursts, and the host mirror over the same entry
points."""
import ctypes as C
import importlib

import numpy as np
import pytest

import levels_ref
import pcm_ref
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
K, MAX_BATCH, N_WIN = 5, 16, 13


@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v24(num_species=70, width=0.25, depth=0.25, head=32)))


@pytest.fixture(scope="module")
def rig(bn, model):
    """The model's S and step, the four recordings (name -> recording), and one context without attachments."""
    S, sr = int(model.config.sample_count), int(model.config.sample_rate)
    step = S // 4
    n = (N_WIN - 1) * step + 100
    rng = np.random.RandomState(21)

    def audio(m, rate):
        x = synth.synthetic_segments(1, m, rate)[0]
        return np.clip(x + 0.05 * rng.standard_normal(m), -1, 1).astype(np.float32)

    i16 = np.round(audio(n, sr) * 32767).astype(np.int16)
    left, right = np.round(audio(n, sr) * 4e6).astype(np.int64), np.round(audio(n, sr) * 4e6).astype(np.int64)
    recs = {
        "i16": bn.Recording(i16),
        "f32": bn.Recording(audio(n, sr)),
        "i24": bn.Recording.from_layout(pcm_ref.pack(np.stack([left, right], axis=1), pcm_ref.I24), bn.BN_PCM_I24, 2, bn.BN_PCM_MIX),
        "rs": bn.Recording(audio(n * 2 // 3, 32000), src_rate=32000, dst_rate=sr),
    }
    for r in recs.values():
        assert r.n_windows(step) == N_WIN and r.n_samples < (N_WIN - 1) * step + S
    return {"S": S, "step": step, "recs": recs, "ctx": bn.Context(model, MAX_BATCH), "model": model}


def _results(ctx, m):
    """every output of the last (complete) step of m rows, as bytes"""
    cfg = ctx.model.config
    out = [a.tobytes() for a in ctx.step_results(m)]
    if cfg.has_embedding:
        out.append(ctx.read_output(cfg.embedding_output, m).tobytes())
    return out


def _windows_step(bn, ctx, rows, S):
    """bn_step_windows over host f32 rows [m, S] as one recording of m windows: the reference step of the same samples and batch"""
    rec = bn.Recording(np.ascontiguousarray(rows, dtype=np.float32).reshape(-1))
    ctx.step_windows(rec, S, 0, len(rows), K, None, sync=True)
    return _results(ctx, len(rows))


def test_contiguous_list_is_step_windows(bn, rig):
    ctx, S, step, rec = rig["ctx"], rig["S"], rig["step"], rig["recs"]["i16"]
    ctx.step_windows(rec, step, 3, 8, K, None, sync=True)
    want = _results(ctx, 8)
    ctx.step_window_list([(rec, k * step, 0, k) for k in range(3, 11)], K, None, sync=True)
    got = _results(ctx, 8)
    assert len(got) >= 4 and got == want
    # asynchronous, then synchronised: the same bytes
    ctx.step_window_list([(rec, k * step) for k in range(3, 11)], K, None, sync=False)
    ctx.synchronize()
    assert _results(ctx, 8) == want
    assert ctx.stats()["capture_fallbacks"] == 0


def test_scrambled_mixed_list(bn, rig):
    ctx, S, step, recs = rig["ctx"], rig["S"], rig["step"], rig["recs"]
    rows = [("i24", 5), ("i16", 0), ("rs", 7), ("f32", 12), ("i16", 9), ("i24", 1), ("f32", 3), ("rs", 2), ("i16", 4)]   # ("f32", 12): a padded tail
    refs = [(recs[name], k * step, i % 3, 100 + i) for i, (name, k) in enumerate(rows)]
    gathered = bn.recording_window_list(refs, S)
    own = np.concatenate([recs[name].windows(S, step, k, 1) for name, k in rows])
    assert gathered.shape == (9, S) and gathered.tobytes() == own.tobytes()
    assert not gathered[3, 100:].any() and gathered[3, :100].any()
    ctx.step_window_list(refs, K, None, sync=True)
    got = _results(ctx, 9)
    assert got == _windows_step(bn, ctx, own, S)
    # every row against the row bn_step_windows gives for its own recording and window
    logits = np.frombuffer(got[0], dtype=np.float32).reshape(9, -1)
    for i, (name, k) in enumerate(rows):
        ctx.step_windows(recs[name], step, k, 1, K, None, sync=True)
        assert ctx.step_results(1)[0].tobytes() == logits[i].tobytes(), (i, name, k)
    assert ctx.stats()["capture_fallbacks"] == 0


def test_every_interleaved_reader(bn):
    """The readers the four recordings above do not reach: interleaved I16, F32, I32 and U8 (and I24 once more), two rows each,
    scrambled, against pcm_ref's samples and against bn_recording_windows row for row."""
    S, n = 1028, 3000
    rng = np.random.RandomState(17)
    layouts = [(pcm_ref.I16, 2, pcm_ref.MIX), (pcm_ref.F32, 2, 1), (pcm_ref.I32, 1, 0), (pcm_ref.U8, 3, pcm_ref.MIX), (pcm_ref.I24, 3, 2),
               (pcm_ref.I32, 2, pcm_ref.MIX), (pcm_ref.U8, 1, 0), (pcm_ref.I16, 4, 3), (pcm_ref.F32, 3, pcm_ref.MIX)]
    recs, mono = [], []
    for fmt, channels, channel in layouts:
        raw = pcm_ref.test_data(rng, fmt, n, channels)
        if fmt == pcm_ref.F32:      # finite samples only: a generated NaN's bits are the implementation's (pcm_ref.test_data)
            raw = pcm_ref.pack(rng.uniform(-1, 1, (n, channels)).astype(np.float32), fmt)
        recs.append(bn.Recording.from_layout(raw, fmt, channels, channel))
        mono.append(pcm_ref.mono(raw, fmt, channels, channel))
    starts = [0, 1, 777, n - S, n - S + 1, n - 1, 1500, 2, n - 500]
    order = rng.permutation(2 * len(layouts))
    refs = [(recs[j % len(layouts)], starts[(j * 5 + j // len(layouts)) % len(starts)]) for j in order]
    got = bn.recording_window_list(refs, S)
    for i, (j, (r, start)) in enumerate(zip(order, refs)):
        assert got[i].tobytes() == levels_ref.window(mono[j % len(layouts)], S, start).tobytes(), (i, layouts[j % len(layouts)], start)
        assert got[i].tobytes() == r.windows(S, 1, start, 1).tobytes(), (i, layouts[j % len(layouts)], start)


def test_host_mirror(bn, rig, tmp_path):
    """birdnet::Recording::levels and Classifier::predict_window_list (bnh_*): the engine's bits, the library's refusals as errors."""
    S, step, recs = rig["S"], rig["step"], rig["recs"]
    rng = np.random.RandomState(31)
    v = rng.randint(-20000, 20000, size=3 * S + 100).astype(np.int16)
    stereo = np.stack([v.astype(np.int64) * 256, np.zeros(len(v), dtype=np.int64)], axis=1)
    a, b = bn.HostRecording(v), bn.HostRecording(pcm_ref.pack(stereo, pcm_ref.I24), bn.BN_PCM_I24, 2, 0)
    ea, eb = bn.Recording(v), bn.Recording.from_layout(pcm_ref.pack(stereo, pcm_ref.I24), bn.BN_PCM_I24, 2, 0)
    assert a.n_samples == len(v) == b.n_samples
    want = ea.levels(S, step)
    assert a.levels(S, step).tobytes() == want.tobytes() == b.levels(S, step).tobytes()
    assert a.levels(S, step, 2, 3).tobytes() == want[2:5].tobytes() and len(a.levels(S, step, len(want), 0)) == 0
    with pytest.raises(bn.Error) as e:
        a.levels(S + 2, step)
    assert e.value.kind == bn.ErrorKind.Inference and "multiple of 4" in str(e.value)
    with pytest.raises(bn.Error) as e:
        a.levels(S, step, 1, len(want))
    assert "exceeds the" in str(e.value)
    path = tmp_path / "m.onnx"
    path.write_bytes(synth.birdnet_v24(num_species=70, width=0.25, depth=0.25, head=32))
    clf = bn.Classifier.builder().model_path(str(path)).labels([f"Species_{i}" for i in range(70)]).top_k(K).with_rocm(0).build()
    hctx = clf.create_native_batch_context(4)
    rows = [(b, 5), (a, 2 * step, 1, 7), (a, 3 * S + 99), (b, step)]
    res = clf.predict_window_list(hctx, rows)
    ctx = bn.Context(bn.Model(str(path)), 4)
    ctx.step_window_list([(eb, 5), (ea, 2 * step), (ea, 3 * S + 99), (eb, step)], K, None, sync=True)
    logits, idx, conf, cnt = ctx.step_results(4)
    assert len(res) == 4
    for i, r in enumerate(res):
        assert np.asarray(r.raw_scores, dtype=np.float32).tobytes() == logits[i].tobytes(), i
        assert [p.index for p in r.predictions] == idx[i, :cnt[i]].tolist()
        assert np.array([p.confidence for p in r.predictions], dtype=np.float32).tobytes() == conf[i, :cnt[i]].tobytes()
    for bad, word in (([(a, len(v))], "row 0: start"), ([(a, 0), (None, 0)], "row 1: null recording"), ([], "empty window list"),
                      ([(a, 0)] * 5, "exceeds context max 4")):
        with pytest.raises(bn.Error) as e:
            clf.predict_window_list(hctx, bad)
        assert e.value.kind == bn.ErrorKind.Inference and word in str(e.value), (word, str(e.value))
    again = clf.predict_window_list(hctx, rows)      # the context is still usable, with the same bits
    assert all(np.asarray(x.raw_scores).tobytes() == np.asarray(y.raw_scores).tobytes() for x, y in zip(res, again))


def test_unaligned_starts(bn, rig):
    S, recs = rig["S"], rig["recs"]
    refs, want = [], []
    for name, start in (("f32", 12345), ("i24", 1), ("i24", recs["i24"].n_samples - 1001), ("rs", recs["rs"].n_samples - 1), ("f32", 0)):
        r = recs[name]
        refs.append((r, start))
        want.append(levels_ref.window(r.read_f32(start, min(S, r.n_samples - start)), S, 0))
    got = bn.recording_window_list(refs, S)
    assert got.tobytes() == np.stack(want).tobytes()
    ctx = rig["ctx"]
    ctx.step_window_list(refs, K, None, sync=True)
    assert _results(ctx, 5) == _windows_step(bn, ctx, got, S)


def test_129_rows_take_a_second_launch(bn, rig):
    S, recs, model = 1028, rig["recs"], rig["model"]
    rng = np.random.RandomState(4)
    names = ["i16"] * 129 + ["i24"] * 3
    order = rng.permutation(len(names))
    refs = [(recs[names[j]], int(rng.randint(0, recs[names[j]].n_samples))) for j in order]
    got = bn.recording_window_list(refs, S)
    for i, (r, start) in enumerate(refs):
        assert got[i].tobytes() == r.windows(S, 1, start, 1).tobytes(), i   # step 1: window `start` starts at frame `start`
    # a step of count == max_batch == 129 over one recording (launches of 128 rows and of 1), against the same rows through bn_step_windows
    S, step = rig["S"], rig["step"]
    ctx = bn.Context(model, 129)
    rows = [(recs["i16"], (i % 12) * step + i) for i in range(129)]
    ctx.step_window_list(rows, K, None, sync=True)
    got = _results(ctx, 129)
    assert got == _windows_step(bn, ctx, bn.recording_window_list(rows, S), S)
    with pytest.raises(bn.EngineError):
        ctx.step_window_list(rows + rows[:1], K, None, sync=True)
    assert "exceeds context max 129" in bn.last_error()
    assert ctx.stats()["capture_fallbacks"] == 0


def test_tracker_sees_the_lists_sources_and_windows(bn, rig, model):
    S, step, recs = rig["S"], rig["step"], rig["recs"]
    n = int(model.config.num_species)
    probe = rig["ctx"]
    probe.step_windows(recs["i16"], step, 0, 8, K, None, sync=True)
    conf = 1.0 / (1.0 + np.exp(-probe.step_results(8)[0].astype(np.float64)))
    enter = float(np.quantile(conf, 0.8))
    dev, host = bn.Tracker(0, 2, n, enter, 1, 1), bn.Tracker(0, 2, n, enter, 1, 1)
    ctx = bn.Context(model, MAX_BATCH)
    ctx.attach_track(dev)
    # a gated subset: two recordings as two sources, gaps in the window numbers, the sources interleaved in the first list
    lists = [[("i16", 0, 0), ("f32", 1, 1), ("i16", 0, 1), ("i16", 0, 4), ("f32", 1, 2), ("f32", 1, 6)],
             [("i16", 0, 5), ("i16", 0, 9), ("f32", 1, 7), ("f32", 1, 12)]]
    total = 0
    for rows in lists:
        refs = [(recs[name], k * step, source, k) for name, source, k in rows]
        ctx.step_window_list(refs, K, None, sync=True)
        ev, dropped, stale = ctx.step_track_results()
        want, wdropped = host.update(ctx.step_results(len(rows))[0], [r[1] for r in rows], [r[2] for r in rows])
        assert (dropped, stale, wdropped) == (0, 0, 0)
        assert ev.dtype == want.dtype and len(ev) == len(want)
        for field in ev.dtype.names:    # the existing tracker tests hold every field, the confidences included, to equal bits
            assert ev[field].tobytes() == want[field].tobytes(), (field, ev, want)
        total += len(ev)
    # a row whose window does not exceed its source's last is a stale row, as after bn_step_live
    ctx.step_window_list([(recs["i16"], 0, 0, 9), (recs["i16"], step, 0, 10)], K, None, sync=True)
    assert ctx.step_track_results()[2] == 1
    host.update(ctx.step_results(2)[0][1:], [0], [10])
    fl, wfl = dev.flush()[0], host.flush()[0]
    assert fl.tobytes() == wfl.tobytes() and total + len(fl) > 0
    assert ctx.stats()["capture_fallbacks"] == 0


def test_gated_loop_end_to_end(bn, rig, model):
    S = rig["S"]
    n_win = 24
    rng = np.random.RandomState(8)
    x = np.zeros(n_win * S, dtype=np.int16)
    burst = lambda m: np.round(8000 * np.sin(np.arange(m) * 0.3) + 200 * rng.standard_normal(m)).astype(np.int16)
    x[3 * S + 5000:3 * S + 25000] = burst(20000)                 # inside window 3
    x[11 * S - 9000:11 * S + 9000] = burst(18000)                # across the boundary of windows 10 and 11
    x[20 * S + 140000:20 * S + 143000] = burst(3000)             # at the end of window 20
    rec = bn.Recording(x)
    lv = rec.levels(S, S)
    assert len(lv) == n_win and not lv["flags"].any()
    keep = levels_ref.gate(lv["peak"], 0.01, 1)
    assert keep.tolist() == [2, 3, 4, 9, 10, 11, 12, 19, 20, 21] and {3, 10, 11, 20} <= set(keep.tolist())
    assert (lv["peak"][[k for k in range(n_win) if k not in (3, 10, 11, 20)]] == 0).all()
    ctx = rig["ctx"]
    full = []
    for first in range(0, n_win, 8):
        ctx.step_windows(rec, S, first, 8, K, None, sync=True)
        full.append([a.copy() for a in ctx.step_results(8)])
    full = [np.concatenate([f[i] for f in full]) for i in range(4)]
    for cut in (keep[:6], keep[6:]):
        ctx.step_window_list([(rec, int(k) * S, 0, int(k)) for k in cut], K, None, sync=True)
        for got, want in zip(ctx.step_results(len(cut)), full):
            assert got.tobytes() == want[cut].tobytes(), cut
    assert ctx.stats()["capture_fallbacks"] == 0


def test_asynchronous_recording_in_the_list(bn, rig):
    ctx, S, step = rig["ctx"], rig["S"], rig["step"]
    rng = np.random.RandomState(2)
    v = rng.randint(-20000, 20000, size=(N_WIN - 1) * step + 100).astype(np.int16)
    sync_rec, async_rec = bn.Recording(v), bn.Recording(v, async_upload=True)
    rows = [(12, 0), (0, 17), (7, 5)]
    ctx.step_window_list([(sync_rec, k * step + off) for k, off in rows] + [(rig["recs"]["f32"], 0)], K, None, sync=True)
    want = _results(ctx, 4)
    ctx.step_window_list([(async_rec, k * step + off) for k, off in rows] + [(rig["recs"]["f32"], 0)], K, None, sync=True)
    assert _results(ctx, 4) == want
    async_rec.wait()


def test_refusals_leave_the_context_usable(bn, rig, model):
    S, step, recs = rig["S"], rig["step"], rig["recs"]
    n = int(model.config.num_species)
    ctx = bn.Context(model, 4)
    rec = recs["i16"]
    ctx.step_windows(rec, step, 2, 3, K, None, sync=True)
    want = _results(ctx, 3)
    good = [(rec, 0), (recs["f32"], 5)]
    size = C.sizeof(bn.BnWindowRef)

    def refused(word, refs=good, count=None, struct_size=size, top_k=K):
        arr, keep = bn.window_refs(refs)
        st = bn.lib.bn_step_window_list(ctx._h, arr, len(keep) if count is None else count, struct_size, top_k, 0, 0.0, 1)
        assert st == 1 and word in bn.last_error(), (word, st, bn.last_error())
        assert _results(ctx, 3) == want       # the last step's results are still there

    refused("empty window list", count=0)
    refused("exceeds context max 4", refs=good * 3)
    refused("row 1: null recording", refs=[(rec, 0), (None, 0)])
    refused("row 1: start " + str(rec.n_samples), refs=[(rec, 0), (rec, rec.n_samples)])
    refused("row 0: start", refs=[(rec, 2 ** 64 - 1)])
    refused("struct_size", struct_size=size - 1)
    refused("top_k", top_k=0)
    refused("source -1 is negative", refs=[(rec, 0, -1, 0)])
    assert bn.lib.bn_step_window_list(ctx._h, None, 1, size, K, 0, 0.0, 1) == 1 and "null window list" in bn.last_error()
    # what the attached tracker refuses of a live step over these sources: more sources than it has
    tracker = bn.Tracker(0, 2, n, 0.5, 1, 0)
    ctx.attach_track(tracker)
    refused("the pool has 3 sources, the attached tracker 2", refs=[(rec, 0, 2, 0)])
    # the list brings its own window numbers: one the tracker cannot hold is refused before anything is enqueued, not inside the step
    refused("row 1: a tracked window number must be below 2^31", refs=[(rec, 0, 0, 5), (rec, step, 1, 2 ** 31)])
    assert tracker.open_events() == 0
    ctx.attach_track(None)
    # counts that no list can have are refused before anything is sized by them
    arr, _ = bn.window_refs(good)
    out = np.zeros(8, dtype=np.float32)
    f32p = out.ctypes.data_as(C.POINTER(C.c_float))
    assert bn.lib.bn_recording_window_list(arr, 2 ** 32, size, 4, f32p) == 1 and "2^32" in bn.last_error()
    assert bn.lib.bn_recording_window_list(arr, 2 ** 32 - 1, size, 2 ** 32 - 4, f32p) == 1 and "address space" in bn.last_error()
    assert bn.lib.bn_step_window_list(ctx._h, arr, 2 ** 63, size, K, 0, 0.0, 1) == 1 and "exceeds context max 4" in bn.last_error()
    with pytest.raises(bn.EngineError):
        bn.recording_window_list([(rec, rec.n_samples)], S)
    assert "row 0: start" in bn.last_error()
    with pytest.raises(bn.EngineError):
        bn.recording_window_list(good, S + 2)
    assert "multiple of 4" in bn.last_error()
    # the context still steps, with the right bits
    ctx.step_window_list([(rec, k * step) for k in (2, 3, 4)], K, None, sync=True)
    assert _results(ctx, 3) == want
    ctx.step_windows(rec, step, 2, 3, K, None, sync=True)
    assert _results(ctx, 3) == want
    assert ctx.stats()["capture_fallbacks"] == 0
