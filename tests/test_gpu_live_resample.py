"""The resampling live pool (bn_live_create_rates): sources that each deliver PCM at their own rate, converted to the model's
rate on the device as pushes arrive.  Per source every window must be bit-identical to the same window of
bn_recording_create_resampled over the concatenation of that source's pushes -- whatever the chunking, across ring wraps, after
a reset, at close (zero-padded tail) -- and the steps through the network bit-identical to bn_step_windows over that recording.
Readiness follows F(pushed) = bn_live_resampled_samples; room is in source samples and never refuses a close."""
import importlib

import numpy as np
import pytest

import test_gpu_live as plain
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")

I16, F32 = 0, 1
PAIRS = [(48000, 32000), (44100, 48000), (16000, 48000), (96000, 32000), (44100, 32000)]


def signal(rng, n, rate, fmt):
    """two tones and a little noise, as test_device_resampler_matches_the_oracle feeds the batch resampler"""
    t = np.arange(n) / rate
    x = 0.5 * np.sin(2 * np.pi * 1500.0 * t + rng.uniform(0, 6)) + 0.2 * np.sin(2 * np.pi * 5200.0 * t) + 0.05 * rng.standard_normal(n)
    if fmt == I16:
        return np.clip(np.round(x * 32767), -32768, 32767).astype(np.int16)
    return x.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


def factors(bn, src, dst, zc=0):
    _, L, M, T = bn.resample_table(src, dst, zc)
    return int(L), int(M), int(T)


def min_ring(bn, S, step, src, dst):
    L, M, T = factors(bn, src, dst)
    return S + step + -(-(T // 2 + 1) * L // M)


def recording_windows(bn, pcm, src, dst, S, step):
    """every window of the resampled recording of pcm: f32 [G, S]"""
    if len(pcm) == 0:
        return np.zeros((0, S), np.float32)
    rec = bn.Recording(pcm, src_rate=src, dst_rate=dst)
    G = rec.n_windows(step)
    assert rec.n_samples == bn.live_resampled_samples(src, dst, len(pcm), True)
    return rec.windows(S, step, 0, G)


def ready_count(bn, src, dst, pushed, S, step, closed=False):
    F = bn.live_resampled_samples(src, dst, pushed, closed)
    if closed:
        return -(-F // step)
    return (F - S) // step + 1 if F >= S else 0


def push_stream_and_check(bn, live, s, pcm, src, dst, S, step, sizes, what):
    """push pcm to source s in chunks of the given sizes (cycled), checking readiness and every newly ready window against the
    recording of the COMPLETE signal; then close and check the tail.  Returns the windows read, f32 [G, S]."""
    want = recording_windows(bn, pcm, src, dst, S, step)
    got = np.zeros_like(want)
    pos, seen, i = 0, 0, 0
    while pos < len(pcm):
        n = min(sizes[i % len(sizes)], len(pcm) - pos)
        i += 1
        assert n <= live.room(s), (what, pos, n, live.room(s))
        live.push(s, pcm[pos:pos + n])
        pos += n
        r = ready_count(bn, src, dst, pos, S, step)
        assert live.ready(s) == r, (what, pos, live.ready(s), r)
        for k in range(seen, r):
            got[k] = live.read_window(s, k)
            assert bits(got[k]) == bits(want[k]), (what, "window", k, "after", pos, float(np.abs(got[k] - want[k]).max()))
        seen = r
    live.close(s)
    assert live.ready(s) == len(want) == ready_count(bn, src, dst, len(pcm), S, step, True), what
    for k in range(seen, len(want)):
        got[k] = live.read_window(s, k)
        assert bits(got[k]) == bits(want[k]), (what, "tail window", k, float(np.abs(got[k] - want[k]).max()))
    return got


# ---- 1. ring content, 2. against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [I16, F32])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_ring_content_is_the_resampled_recording(bn, src, dst, fmt):
    import oracle
    from oracle import resample as R
    L, M, T = factors(bn, src, dst)
    S, step = 1000, 400
    rng = np.random.RandomState(src // 100 + dst // 1000 + fmt)
    # a ring near its minimum: nothing is stepped here, so every stream fills it once; the resets between the streams move the
    # ring base, so that over the rounds the streams wrap the ring at different places
    ring = min_ring(bn, S, step, src, dst) + 37
    live = bn.Live(0, 2, S, step, ring, fmt, dst_rate=dst, src_rates=[src, src])
    assert live.source_rate(0) == src and live.source_rate(1) == src
    small = [1, 1, 2, T - 1, 3, T // 2, 1, T + 5, 7, 250, 1, 33]
    for rnd in range(4):
        room = live.room(0)
        assert room == (ring * M) // L, (rnd, room)
        n = room if rnd % 2 == 0 else room - rng.randint(1, 300)
        pcm = signal(rng, n, src, fmt)
        sizes = list(rng.permutation(small)) + [int(rng.randint(1, 400))]
        got = push_stream_and_check(bn, live, 0, pcm, src, dst, S, step, sizes, (src, dst, fmt, "round", rnd))
        # 2. the same windows against the float64 oracle, at the tolerance the batch resampler is held to
        y = R.resample(pcm, src, dst)
        for k in range(len(got)):
            ref = oracle.chunk_fill(y, S, k * step)
            assert np.abs(got[k] - ref).max() <= 3e-6, (src, dst, fmt, rnd, k, float(np.abs(got[k] - ref).max()))
        live.reset(0)
        assert live.ready(0) == 0
    # chunks larger than one tile of the scatter (4096 outputs), in a ring that holds them; source 1 of a second pool
    big_ring = min_ring(bn, S, step, src, dst) + 3 * 4096 + 11
    live2 = bn.Live(0, 2, S, step, big_ring, fmt, dst_rate=dst, src_rates=[src, src])
    live2.push(1, signal(rng, 777, src, fmt))
    live2.reset(1)  # the stream starts 777 source samples' outputs into the ring, with a stale history behind it
    n = live2.room(1) - 5
    pcm = signal(rng, n, src, fmt)
    tile_in = 4096 * M // L
    sizes = [tile_in + 100 + T, 1, 2 * tile_in + 3, T - 1, tile_in // 2]
    push_stream_and_check(bn, live2, 1, pcm, src, dst, S, step, sizes, (src, dst, fmt, "big"))


def test_zero_crossings_8_and_an_empty_stream(bn):
    src, dst, S, step = 48000, 32000, 1000, 400
    L, M, T = factors(bn, src, dst, 8)
    assert T == 24
    rng = np.random.RandomState(8)
    live = bn.Live(0, 2, S, step, 4000, I16, dst_rate=dst, src_rates=[src, src], zero_crossings=8)
    pcm = signal(rng, 5000, src, I16)
    rec = bn.Recording(pcm, src_rate=src, dst_rate=dst, zero_crossings=8)
    want = rec.windows(S, step, 0, rec.n_windows(step))
    for a, b in [(0, 5), (5, 6), (6, 3000), (3000, 5000)]:
        live.push(0, pcm[a:b])
    live.close(0)
    live.close(1)  # closed with nothing pushed: no windows
    assert live.ready(0) == len(want) and live.ready(1) == 0
    for k in range(len(want)):
        assert bits(live.read_window(0, k)) == bits(want[k]), k


# ---- 3. through the network -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models(bn):
    v24 = bn.Model(write_model(synth.birdnet_v24(num_species=500, width=0.5, depth=0.5, head=256)))
    v30 = bn.Model(write_model(synth.birdnet_v30(num_species=300, width=0.5, depth=0.5, emb=256)))
    return {"v24": v24, "v30": v30}


def resampled_reference(bn, ctx, pcm, src, dst, step, top_k, min_conf):
    """bn_step_windows over the resampled recording of pcm: (logits, idx, conf, cnt) per window"""
    if len(pcm) == 0:
        return []
    rec = bn.Recording(pcm, src_rate=src, dst_rate=dst)
    G = rec.n_windows(step)
    out = []
    for f in range(0, G, ctx.max_batch):
        m = min(ctx.max_batch, G - f)
        ctx.step_windows(rec, step, f, m, top_k, min_conf, sync=True)
        lg, ix, cf, ct = ctx.step_results(m)
        out += [(lg[i], ix[i], cf[i], ct[i]) for i in range(m)]
    return out


def check_sources(bn, model, got, pcms, rates, dst, step):
    ref_ctx = bn.Context(model, 4)
    for s, pcm in enumerate(pcms):
        want = resampled_reference(bn, ref_ctx, pcm, rates[s], dst, step, 5, 0.02)
        assert sorted(got[s]) == list(range(len(want))), (s, sorted(got[s]), len(want))
        for k in range(len(want)):
            plain.check_row(got[s][k], want[k], (s, k))


@pytest.mark.parametrize("name,src,fmt", [("v30", 48000, I16), ("v24", 44100, F32)])
def test_steps_are_bit_identical_to_the_resampled_recording(bn, models, name, src, fmt):
    model = models[name]
    S, dst = model.config.sample_count, model.config.sample_rate
    step = S - dst // 2
    L, M, T = factors(bn, src, dst)
    rng = np.random.RandomState(17 + fmt)
    lens_out = [0, S // 3, S, 2 * S + 5, 3 * S + step // 2]
    pcms = [signal(rng, n * M // L, src, fmt) for n in lens_out]
    ctxs = [bn.Context(model, 4), bn.Context(model, 3)]
    live = bn.Live(0, len(pcms), S, step, min_ring(bn, S, step, src, dst) + 4096, fmt, dst_rate=dst, src_rates=[src] * len(pcms))
    got = plain.drive(bn, live, ctxs, pcms, fmt, rng, 5, 0.02, False, 2 * src)
    check_sources(bn, model, got, pcms, [src] * len(pcms), dst, step)
    for c in ctxs:
        assert c.stats()["capture_fallbacks"] == 0


# ---- 4. mixed pool --------------------------------------------------------------------------------------------------
def test_mixed_rates_and_a_pass_through_source_in_one_pool(bn, models):
    model = models["v30"]
    S, dst = model.config.sample_count, model.config.sample_rate
    step = S // 2
    rates = [48000, 44100, 16000, dst]
    rng = np.random.RandomState(41)
    pcms = [signal(rng, int((2 * S + 1234 * (s + 1)) * r / dst), r, I16) for s, r in enumerate(rates)]
    ring = max(min_ring(bn, S, step, r, dst) for r in rates[:3]) + 1000
    live = bn.Live(0, 4, S, step, ring, I16, dst_rate=dst, src_rates=rates)
    assert [live.source_rate(s) for s in range(4)] == rates
    ctx = bn.Context(model, 6)
    got = plain.drive(bn, live, [ctx], pcms, I16, rng, 5, 0.02, True, dst)
    check_sources(bn, model, got, pcms, rates, dst, step)
    assert ctx.stats()["capture_fallbacks"] == 0
    # the pass-through source: bit for bit what a plain pool yields
    plain_live = bn.Live(0, 1, S, step, ring, I16)
    got_plain = plain.drive(bn, plain_live, [ctx], [pcms[3]], I16, np.random.RandomState(42), 5, 0.02, True, dst)
    assert sorted(got_plain[0]) == sorted(got[3])
    for k in got_plain[0]:
        plain.check_row(got[3][k], got_plain[0][k], ("pass-through", k))


# ---- 5. room and refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(48000, 32000), (16000, 48000), (44100, 32000)])
def test_room_is_exact_and_a_close_always_fits(bn, models, src, dst):
    import ctypes as C
    L, M, T = factors(bn, src, dst)
    S, step = 1000, 400
    ring = min_ring(bn, S, step, src, dst) + 5
    rng = np.random.RandomState(src // 100)
    live = bn.Live(0, 2, S, step, ring, I16, dst_rate=dst, src_rates=[src, src])
    room = live.room(0)
    assert room == (ring * M) // L
    pcm = signal(rng, room + 1, src, I16)
    first = room * 4 // 5  # enough for a first ready window
    live.push(0, pcm[:first])
    room = live.room(0)
    assert room == (ring * M) // L - first
    state = (live.ready(0), live.room(0), live.ready(-1))
    before = [live.read_window(0, k) for k in range(live.ready(0))]
    with pytest.raises(bn.EngineError):
        live.push(0, pcm[first:first + room + 1])  # one sample past the room: refused whole
    with pytest.raises(bn.EngineError):
        live.push_many([1, 0], [pcm[:10], pcm[first:first + room + 1]])
    assert "source 0" in bn.last_error()
    assert (live.ready(0), live.room(0), live.ready(-1)) == state and live.room(1) == (ring * M) // L
    live.push(0, pcm[first:first + room])  # exactly the room
    assert live.room(0) == 0
    with pytest.raises(bn.EngineError):
        live.push(0, pcm[:1])
    live.close(0)  # the ring as full as pushes can make it: the tail still fits
    want = recording_windows(bn, pcm[:first + room], src, dst, S, step)
    assert live.ready(0) == len(want)
    for k in range(len(want)):
        w = live.read_window(0, k)
        assert bits(w) == bits(want[k]), k
        if k < len(before):
            assert bits(before[k]) == bits(w), ("changed by a refused push", k)
    # refusals
    h = C.c_void_p()
    rates = (C.c_uint32 * 2)(src, 0)
    assert bn.lib.bn_live_create_rates(0, 2, 0, S, step, ring, dst, rates, 0, C.byref(h)) == 1  # BN_ERR_INVALID_ARG
    rates[1] = src
    assert bn.lib.bn_live_create_rates(0, 2, 0, S, step, S + step, dst, rates, 0, C.byref(h)) == 1  # no space for the tail
    ctx = bn.Context(models["v24"], 2)
    with pytest.raises(bn.EngineError):
        ctx.step_live(live, 1, 3)  # a context of another segment length
    assert live.ready(0) == len(want)
    # a pair whose table is beyond what a pool accepts is refused with the source and the pair named
    with pytest.raises(bn.EngineError):
        bn.Live(0, 2, S, step, 100000, I16, dst_rate=1000, src_rates=[1000, 48000])  # 1536 taps per phase
    assert "source 1" in bn.last_error() and "48000" in bn.last_error()


# ---- 6. reset mid-stream --------------------------------------------------------------------------------------------
def test_reset_mid_stream_leaks_no_history(bn, models):
    model = models["v30"]
    S, dst, src = model.config.sample_count, model.config.sample_rate, 48000
    step = S // 2
    L, M, T = factors(bn, src, dst)
    ring = min_ring(bn, S, step, src, dst) + 100
    rng = np.random.RandomState(6)
    ctx = bn.Context(model, 4)
    ref_ctx = bn.Context(model, 4)
    live = bn.Live(0, 1, S, step, ring, I16, dst_rate=dst, src_rates=[src])
    old = signal(rng, live.room(0), src, I16)
    live.push(0, old)
    want_old = resampled_reference(bn, ref_ctx, old, src, dst, step, 3, None)
    n_ready = live.ready(0)
    assert n_ready >= 2
    src_ids, win = ctx.step_live(live, 1, 3, None, sync=True)
    assert win.tolist() == [0]
    src_ids, win = ctx.step_live(live, 1, 3, None, sync=False)  # in flight across the reset
    assert src_ids.tolist() == [0] and win.tolist() == [1]
    live.reset(0)
    assert live.ready(0) == 0 and live.room(0) == (ring * M) // L
    new = signal(rng, live.room(0) - 17, src, I16)
    for a, b in [(0, 3), (3, T), (T, len(new))]:
        live.push(0, new[a:b])  # overwrites the ring the in-flight step reads
    ctx.synchronize()
    lg, ix, cf, ct = ctx.step_results(1)
    plain.check_row((lg[0], ix[0], cf[0], ct[0]), want_old[1], "in-flight step across reset")
    live.close(0)
    want_win = recording_windows(bn, new, src, dst, S, step)
    assert live.ready(0) == len(want_win)
    assert bits(live.read_window(0, 0)) == bits(want_win[0])  # the first outputs saw zeros, not the old stream
    want_new = resampled_reference(bn, ref_ctx, new, src, dst, step, 3, None)
    rows = {}
    while live.ready(-1):
        src_ids, win = ctx.step_live(live, 4, 3, None, sync=True)
        lg, ix, cf, ct = ctx.step_results(len(src_ids))
        for r, k in enumerate(win.tolist()):
            rows[k] = (lg[r], ix[r], cf[r], ct[r])
    assert sorted(rows) == list(range(len(want_new)))
    for k in rows:
        plain.check_row(rows[k], want_new[k], ("after reset", k))


# ---- 7. host mirror -------------------------------------------------------------------------------------------------
def test_predict_live_matches_predict_recording_of_the_resampled_signal(bn):
    num = 500
    path = write_model(synth.birdnet_v24(num_species=num, width=0.5, depth=0.5, head=256))
    labels = [f"Species_{i}" for i in range(num)]
    clf = bn.Classifier.builder().model_path(path).labels(labels).top_k(5).min_confidence(0.02).with_rocm(0).build()
    ctx = clf.create_batch_context(4)
    S, dst = 144000, 48000
    overlap = 1.0
    rates = [44100, 16000, 48000]
    rng = np.random.RandomState(12)
    pcms = [signal(rng, int(n * r / dst), r, I16) for n, r in zip((3 * S + 1000, S // 2, 2 * S), rates)]
    live = bn.LiveSources(clf, len(pcms), I16, overlap, 0, source_rates=rates)
    rows = {s: {} for s in range(len(pcms))}
    pos = [0] * len(pcms)
    for _ in range(300):
        if not (any(pos[s] < len(p) for s, p in enumerate(pcms)) or live.ready() > 0):
            break
        for s, p in enumerate(pcms):
            n = min(rates[s], len(p) - pos[s])
            if n > 0:
                try:
                    live.push(s, p[pos[s]:pos[s] + n])
                    pos[s] += n
                    if pos[s] == len(p):
                        live.close(s)
                except bn.Error:
                    pass  # no room yet: the step below frees it
        for s, k, t, r in clf.predict_live(ctx, live, 3):
            rows[s][k] = (t, r)
    for s, p in enumerate(pcms):
        # a source at the model's rate is a plain upload (an i16 recording): predict_recording takes its samples as they are
        resampled = p if rates[s] == dst else bn.Recording(p, src_rate=rates[s], dst_rate=dst).read_f32()
        want = clf.predict_recording(ctx, resampled, overlap)
        assert sorted(rows[s]) == list(range(len(want))), s
        for k, (t, r) in enumerate(want):
            gt, gr = rows[s][k]
            assert np.float32(gt).tobytes() == np.float32(t).tobytes(), (s, k, gt, t)
            assert [x.species for x in gr.predictions] == [x.species for x in r.predictions], (s, k)
            assert [np.float32(x.confidence).tobytes() for x in gr.predictions] == [np.float32(x.confidence).tobytes() for x in r.predictions]
            assert np.array_equal(np.asarray(gr.raw_scores, dtype=np.float32).view(np.uint32),
                                  np.asarray(r.raw_scores, dtype=np.float32).view(np.uint32))
