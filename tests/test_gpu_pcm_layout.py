"""PCM layouts on the device (include/birdnet_hip.h, "PCM layouts"): interleaved multi-channel I16 / F32 / I24 / I32 / U8 read
as one channel or mixed down, for recordings and live pools.  The invariant under test: every consumer of a layout input sees
exactly the f32 sample tests/pcm_ref.py defines, so every path over a layout input equals, byte for byte, the same path over a
mono f32 input holding those samples.  All comparisons are tobytes() equalities."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pcm_ref as P
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")

N, S, STEP = 1003, 256, 100  # 1003 frames: the I24 byte phase of a frame hits all four residues
CHANNELS = [1, 2, 3, 4, 16]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).tobytes()


def ops(channels):
    return list(range(channels)) + [P.MIX]


def seed(fmt, channels, extra=0):
    return 1000 * fmt + 10 * channels + extra


@pytest.fixture(scope="module")
def model(bn):
    return bn.Model(write_model(synth.birdnet_v24(num_species=500, width=0.5, depth=0.5, head=256)))


# ---- 1. windows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("fmt", P.FORMATS)
def test_windows_are_the_rule(bn, fmt, channels):
    raw = P.test_data(np.random.RandomState(seed(fmt, channels)), fmt, N, channels)
    for op in ops(channels):
        want = P.chunk_audio(P.mono(raw, fmt, channels, op), S, STEP)
        rec = bn.Recording.from_layout(raw, fmt, channels, op)
        assert rec.n_samples == N and rec.n_windows(STEP) == len(want) == 11
        got = rec.windows(S, STEP, 0, len(want))  # the last windows reach past frame 1003: the zero-padded tail
        assert bits(got) == bits(want), (P.NAMES[fmt], channels, op, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        assert bits(rec.windows(S, STEP, 7, 3)) == bits(want[7:10]), (P.NAMES[fmt], channels, op, "first_window 7")


# ---- 2. read_f32 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,channels,op", [(P.I24, 2, P.MIX), (P.I24, 3, 1), (P.U8, 3, 2), (P.I32, 4, P.MIX), (P.I16, 2, 1), (P.F32, 2, P.MIX), (P.I24, 1, 0),
                                             (P.F32, 1, 0), (P.I16, 1, 0)])
def test_read_f32_at_unaligned_first(bn, fmt, channels, op):
    raw = P.test_data(np.random.RandomState(seed(fmt, channels, 1)), fmt, N, channels)
    want = P.mono(raw, fmt, channels, op)
    rec = bn.Recording.from_layout(raw, fmt, channels, op)
    for first, count in ((0, N), (1, 1), (3, 997), (5, 2), (N - 1, 1), (N, 0), (501, 6)):
        assert bits(rec.read_f32(first, count)) == bits(want[first:first + count]), (P.NAMES[fmt], channels, op, first, count)
    with pytest.raises(bn.EngineError):
        rec.read_f32(N - 1, 2)
    # what the mono entry point refused, it still refuses
    if fmt == P.I16 and channels == 1:
        with pytest.raises(bn.EngineError):
            bn.Recording(np.frombuffer(raw, np.int16)).read_f32(0, 1)
        assert "not f32" in bn.last_error()


# ---- 3. view_channel ------------------------------------------------------------------------------------------------------
def test_view_channel_shares_one_upload(bn):
    raw = P.test_data(np.random.RandomState(3), P.I24, N, 2)
    parent = bn.Recording.from_layout(raw, P.I24, 2, 0)
    views = {c: parent.view_channel(c) for c in (0, 1, P.MIX)}
    for c, v in views.items():
        assert v.n_samples == N
        assert bits(v.windows(S, STEP, 0, 11)) == bits(bn.Recording.from_layout(raw, P.I24, 2, c).windows(S, STEP, 0, 11)), c
    # the parent goes first: the views keep the device bytes
    want = {c: P.chunk_audio(P.mono(raw, P.I24, 2, c), S, STEP) for c in views}
    parent.__del__()
    for c, v in views.items():
        assert bits(v.windows(S, STEP, 0, 11)) == bits(want[c]), ("after the parent was freed", c)
        assert bits(v.read_f32(3, 500)) == bits(P.mono(raw, P.I24, 2, c)[3:503])
    # a view of a view, and the view going first
    vv = views[1].view_channel(0)
    for v in views.values():
        v.__del__()
    assert bits(vv.windows(S, STEP, 0, 11)) == bits(want[0])


# ---- 4. asynchronous upload -----------------------------------------------------------------------------------------------
def test_async_upload_cuts_chunks_at_frame_boundaries(bn, monkeypatch):
    monkeypatch.setenv("BN_UPLOAD_CHUNK_MB", "1")  # the smallest chunk; the switch is read at every creation
    chunk_frames = (1 << 20) // 6                  # 174762 frames of 6 bytes: 4 bytes of every MiB belong to no whole frame
    n = 2 * chunk_frames + 12345                   # three chunks
    rng = np.random.RandomState(4)
    raw = P.pack(rng.randint(-8388608, 8388608, size=2 * n, dtype=np.int64), P.I24)
    sync = bn.Recording.from_layout(raw, P.I24, 2, P.MIX)
    rec = bn.Recording.from_layout(raw, P.I24, 2, P.MIX, async_upload=True)
    assert rec.n_samples == n
    x = P.mono(raw, P.I24, 2, P.MIX)
    for k in (1, 2):
        b = k * chunk_frames
        first = (b - S) // STEP - 1
        count = 6  # windows that end before, straddle and start after the boundary
        assert first * STEP + S <= b < (first + count - 1) * STEP
        got = rec.windows(S, STEP, first, count)
        assert bits(got) == bits(sync.windows(S, STEP, first, count)), ("chunk boundary", k)
        assert bits(got) == bits(P.chunk_audio(x[first * STEP:(first + count - 1) * STEP + S], S, STEP)[:count]), ("chunk boundary", k)
        assert bits(rec.read_f32(b - 3, 7)) == bits(x[b - 3:b + 4]), ("frames across chunk boundary", k)
    last = rec.n_windows(STEP) - 3
    assert bits(rec.windows(S, STEP, last, 3)) == bits(sync.windows(S, STEP, last, 3))
    rec.wait()
    view = rec.view_channel(1)
    assert bits(view.read_f32(chunk_frames - 2, 5)) == bits(P.mono(raw, P.I24, 2, 1)[chunk_frames - 2:chunk_frames + 3])


# ---- 5. resampled ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [(44100, 48000), (16000, 32000)])
def test_resampled_layout_is_the_resampled_mono_recording(bn, src, dst):
    n = 5003
    t = np.arange(n) / src
    rng = np.random.RandomState(src // 100)
    left = 0.5 * np.sin(2 * np.pi * 1500.0 * t) + 0.05 * rng.standard_normal(n)
    right = 0.3 * np.sin(2 * np.pi * 3100.0 * t + 1.0) + 0.05 * rng.standard_normal(n)
    v = np.clip(np.round(np.stack([left, right], axis=1) * 8388607), -8388608, 8388607).astype(np.int64)
    v[:3, 0], v[:3, 1] = [-8388608, 8388607, 0], [8388607, -8388608, -1]
    raw = P.pack(v, P.I24)
    for op in (P.MIX, 1):
        want = bn.Recording(P.mono(raw, P.I24, 2, op), src_rate=src, dst_rate=dst)
        got = bn.Recording.from_layout(raw, P.I24, 2, op, src_rate=src, dst_rate=dst)
        assert got.n_samples == want.n_samples
        assert bits(got.read_f32()) == bits(want.read_f32()), (src, dst, op)
    # the result is mono f32: channel 0 or MIX of it are views, anything else is refused
    assert bits(got.view_channel(P.MIX).read_f32(1, 100)) == bits(want.read_f32(1, 100))
    with pytest.raises(bn.EngineError):
        got.view_channel(1)
    assert "no storage-format bytes left" in bn.last_error()


# ---- 6. the model path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,channels,op", [(P.U8, 3, 1), (P.I32, 4, P.MIX)])
def test_step_windows_over_a_layout_recording(bn, model, fmt, channels, op):
    ctx = bn.Context(model, 3)
    seg = 144000
    n = 2 * seg + 5001  # three windows, the last zero-padded
    raw = P.test_data(np.random.RandomState(seed(fmt, channels, 6)), fmt, n, channels)
    lay = bn.Recording.from_layout(raw, fmt, channels, op)
    ref = bn.Recording(P.mono(raw, fmt, channels, op))
    assert lay.n_windows(seg) == ref.n_windows(seg) == 3
    out = {}
    for name, rec in (("ref", ref), ("layout", lay)):
        rows = []
        for rnd in range(2):  # the second step replays the context's captured graph
            ctx.step_windows(rec, seg, 0, 3, 5, 0.01, sync=True)
            lg, ix, cf, ct = ctx.step_results(3)
            rows.append((lg.tobytes(), ix.tobytes(), cf.tobytes(), ct.tobytes()))
        out[name] = rows
    assert out["layout"][0] == out["ref"][0], "logits / top-K rows differ from the f32-mono recording"
    assert out["layout"][1] == out["ref"][1], "... on the replayed graph"
    assert out["layout"][0] == out["layout"][1]


# ---- 7. live pools --------------------------------------------------------------------------------------------------------
RATES = [44100, 16000, 48000]


def frames_of(raw, fmt, channels, a, b):
    fb = P.SAMPLE_BYTES[fmt] * channels
    return raw[a * fb:b * fb]


def feed(pool, ref_pool, s, raw, x, fmt, channels, sizes):
    """the same frames to the layout pool (storage bytes) and the f32-mono pool (the rule's samples), in uneven pushes"""
    pos, i, n = 0, 0, len(x)
    while pos < n:
        k = min(sizes[i % len(sizes)], n - pos)
        i += 1
        pool.push(s, frames_of(raw, fmt, channels, pos, pos + k))
        ref_pool.push(s, x[pos:pos + k])
        pos += k


@pytest.mark.parametrize("resample", [False, True])
@pytest.mark.parametrize("fmt,channels,op", [(P.I24, 2, P.MIX), (P.U8, 3, 1)])
def test_live_windows_equal_the_f32_mono_pool(bn, fmt, channels, op, resample):
    ring = 4000
    kw = dict(dst_rate=48000, src_rates=RATES) if resample else {}
    pool = bn.Live(0, 3, S, STEP, ring, layout=(fmt, channels, op), **kw)
    ref_pool = bn.Live(0, 3, S, STEP, ring, P.F32, **kw)
    rng = np.random.RandomState(seed(fmt, channels, 7 + resample))
    for rnd in range(2):  # the reset between the rounds moves the ring base: the second stream wraps the ring
        for s in range(3):
            room = pool.room(s)
            assert room == ref_pool.room(s)
            n = room - 11 - s
            outputs = n * 48000 // RATES[s] if resample else n
            assert outputs > 2200, (n, "more than half the ring, so two rounds wrap it")
            raw = P.test_data(rng, fmt, n, channels)
            x = P.mono(raw, fmt, channels, op)
            feed(pool, ref_pool, s, raw, x, fmt, channels, [1, 7, 1000])
            pool.close(s), ref_pool.close(s)
            g = pool.ready(s)
            assert g == ref_pool.ready(s) and g > 20
            if not resample or RATES[s] == 48000:
                want = P.chunk_audio(x, S, STEP)
                assert g == len(want)
            for k in range(g):
                got = pool.read_window(s, k)
                assert bits(got) == bits(ref_pool.read_window(s, k)), (P.NAMES[fmt], channels, op, resample, "round", rnd, "source", s, "window", k)
                if not resample or RATES[s] == 48000:
                    assert bits(got) == bits(want[k])
            pool.reset(s), ref_pool.reset(s)


@pytest.mark.parametrize("resample", [False, True])
def test_step_live_equals_the_f32_mono_pool(bn, model, resample):
    fmt, channels, op, seg = P.I24, 2, P.MIX, 144000
    kw = dict(dst_rate=48000, src_rates=RATES) if resample else {}
    ring = 2 * seg + 4000
    pool = bn.Live(0, 3, seg, seg, ring, layout=(fmt, channels, op), **kw)
    ref_pool = bn.Live(0, 3, seg, seg, ring, P.F32, **kw)
    rng = np.random.RandomState(70 + resample)
    for s in range(3):
        rate = RATES[s] if resample else 48000
        n = (seg + 3000) * rate // 48000  # one whole window and a tail
        raw = P.test_data(rng, fmt, n, channels)
        feed(pool, ref_pool, s, raw, P.mono(raw, fmt, channels, op), fmt, channels, [1, 7, 1000, 20000])
    assert pool.ready() == ref_pool.ready() == 3
    ctx = bn.Context(model, 4)
    rows = []
    for p in (ref_pool, pool):
        src, win = ctx.step_live(p, 4, 5, 0.01, sync=True)
        assert list(src) == [0, 1, 2] and list(win) == [0, 0, 0]
        lg, ix, cf, ct = ctx.step_results(3)
        rows.append((lg.tobytes(), ix.tobytes(), cf.tobytes(), ct.tobytes()))
    assert rows[0] == rows[1], "bn_step_live over the layout pool differs from the f32-mono pool"


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_write_no_handle(bn):
    L = bn.lib
    pcm = (C.c_uint8 * 96)()
    rates = (C.c_uint32 * 1)(44100)

    def refused(call, needle):
        h = C.c_void_p(0xdead)
        assert call(h) == 1, needle  # BN_ERR_INVALID_ARG
        assert h.value is None, needle
        assert needle in bn.last_error(), (needle, bn.last_error())

    bad = ((bn.BnPcmLayout(5, 1, 0), "unknown PCM format"), (bn.BnPcmLayout(2, 0, 0), "channels"), (bn.BnPcmLayout(2, 17, 0), "channels"),
           (bn.BnPcmLayout(2, 2, 2), "channel"), (bn.BnPcmLayout(2, 2, -2), "channel"))
    for lay, needle in bad:
        sz = C.sizeof(lay)
        refused(lambda h: L.bn_recording_create_layout(0, pcm, 2, C.byref(lay), sz, C.byref(h)), needle)
        refused(lambda h: L.bn_recording_create_layout_async(0, pcm, 2, C.byref(lay), sz, C.byref(h)), needle)
        refused(lambda h: L.bn_recording_create_layout_resampled(0, pcm, 2, C.byref(lay), sz, 44100, 48000, 0, C.byref(h)), needle)
        refused(lambda h: L.bn_live_create_layout(0, 1, C.byref(lay), sz, 256, 100, 1024, 0, None, 0, C.byref(h)), needle)
        refused(lambda h: L.bn_live_create_layout(0, 1, C.byref(lay), sz, 256, 100, 4096, 48000, rates, 0, C.byref(h)), needle)
    refused(lambda h: L.bn_recording_create_layout(0, pcm, 2, None, 12, C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_recording_create_layout_async(0, pcm, 2, None, 12, C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_recording_create_layout_resampled(0, pcm, 2, None, 12, 44100, 48000, 0, C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_live_create_layout(0, 1, None, 12, 256, 100, 1024, 0, None, 0, C.byref(h)), "null PCM layout")
    # view_channel: outside [-1, channels) of the recording's own layout; a resampled recording is mono f32
    stereo = bn.Recording.from_layout(bytes(96), P.I24, 2, 0)
    for c in (2, -2, 16):
        refused(lambda h: L.bn_recording_view_channel(stereo._h, c, C.byref(h)), "channel")
    res = bn.Recording.from_layout(bytes(96), P.I24, 2, P.MIX, src_rate=16000, dst_rate=32000)
    refused(lambda h: L.bn_recording_view_channel(res._h, 1, C.byref(h)), "no storage-format bytes left")
    refused(lambda h: L.bn_recording_view_channel(None, 0, C.byref(h)), "null recording")
    # a push to a layout pool counts frames: more frames than the room is refused whole
    pool = bn.Live(0, 1, 256, 100, 1024, layout=(P.I24, 2, P.MIX))
    assert pool.room(0) == 1024
    with pytest.raises(bn.EngineError):
        pool.push(0, bytes(6 * 1025))
    pool.push(0, bytes(6 * 1024))
    assert pool.room(0) == 0


# ---- 9. unchanged bits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [P.I16, P.F32])
def test_mono_entry_point_and_its_layout_give_identical_windows(bn, fmt):
    raw = P.test_data(np.random.RandomState(9 + fmt), fmt, N, 1)
    a = np.frombuffer(raw, np.int16 if fmt == P.I16 else np.float32)
    old = bn.Recording(a)
    for op in (0, P.MIX):
        new = bn.Recording.from_layout(raw, fmt, 1, op)
        assert bits(old.windows(S, STEP, 0, 11)) == bits(new.windows(S, STEP, 0, 11)) == bits(P.chunk_audio(P.mono(raw, fmt, 1, 0), S, STEP))
    assert bits(bn.Recording(a, async_upload=True).windows(S, STEP, 0, 11)) == bits(old.windows(S, STEP, 0, 11))


# ---- 10. read_f32 past its first piece ------------------------------------------------------------------------------------
def test_read_f32_converts_in_pieces_of_2_to_the_24(bn):
    """a converting read runs the window kernel over at most 2^24 frames at a time: 2^24 + 5 frames take two pieces"""
    piece = 1 << 24
    n = piece + 5
    pcm = np.random.RandomState(24).randint(-32768, 32768, size=(n, 2)).astype(np.int16)
    want = pcm[:, 1].astype(np.float32) / np.float32(32768.0)  # exact: an int16 over a power of two
    rec = bn.Recording.from_layout(pcm, P.I16, 2, 0).view_channel(1)
    assert rec.n_samples == n
    assert bits(rec.read_f32()) == bits(want)
    assert bits(rec.read_f32(piece - 3, 7)) == bits(want[piece - 3:piece + 4])
