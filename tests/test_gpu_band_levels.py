"""bn_recording_band_levels on the GPU against tests/band_levels_ref.py (float64, numpy.fft.rfft over frames cut by the rule).

Every float is compared within the header's bound, 2 eps sqrt(P T) + eps^2 T + delta P with eps and delta from BN_BAND_EPS_ULPS and
BN_BAND_SUM_DEPTH as the header declares them (band_levels_ref.bound); flags and n_frames exactly; the invariance runs byte for byte.
tests/test_band_levels_cpu.py shows on the random-audio inputs below that four wrong rules leave that bound.  Each test prints its
worst error as a share of the bound.

Shapes: every frame length with hops N, N/2 and 100 at S = 8192 (5 windows at step S/3, the last three padded), the model's segment
with 280 frames, and 1, 3, 4, 5 and 9 frames for the four waves of a workgroup."""
import ctypes as C

import numpy as np
import pytest

import band_levels_ref as ref
import pcm_ref

pytestmark = pytest.mark.gpu
SEG, RATE = 144000, 48000
VOICE = (43, 214)  # 2 - 10 kHz at 48 kHz and frames of 1024: band_bins(48000, 1024, 2000, 10000)


def _floats(got, nb):
    return {"mean": got["mean"][:, :nb].astype(np.float64), "max": got["max"][:, :nb].astype(np.float64),
            "total_mean": got["total_mean"].astype(np.float64), "total_max": got["total_max"].astype(np.float64)}


def _check(bn, got, r, nb, what):
    """flags and n_frames exactly, bands the spec does not have 0, every float within the header's bound; returns the worst share"""
    assert got.dtype == bn.BAND_DTYPE and len(got) == len(r["flags"]), what
    assert got["flags"].tolist() == r["flags"].tolist(), what
    assert got["n_frames"].tolist() == r["n_frames"].tolist(), what
    assert not got["mean"][:, nb:].any() and not got["max"][:, nb:].any(), what
    g, b = _floats(got, nb), ref.bounds(r)
    share = ref.worst_share(g, r)
    print(what, "worst error / bound", share)
    for k in b:
        err = np.abs(g[k] - r[k])
        assert (err <= b[k]).all(), (what, k, err, b[k])
    return share


def _f32(v):
    return pcm_ref.mono(pcm_ref.pack(v, pcm_ref.I16), pcm_ref.I16, 1, 0)


def _tone(n, hz, amp, rate=RATE, phase=0.0):
    return amp * np.sin(2 * np.pi * hz * np.arange(n) / rate + phase)


def test_known_answers(bn):
    S, N, hop = 4096, 256, 128
    n = np.arange(S)
    x = np.concatenate([0.5 * np.sin(2 * np.pi * 10 * n / N + 0.2) + 0.1 * np.sin(2 * np.pi * 40 * n / N), 0.25 * (-1.0) ** n, np.full(S, -0.75)]).astype(np.float32)
    bands = [(9, 12), (39, 42), (0, 2), (127, 129)]
    got = bn.Recording(x).band_levels(S, S, N, hop, bands)
    r = ref.band_levels(x, S, S, N, hop, bands)
    _check(bn, got, r, 4, "known answers")
    assert got["n_frames"].tolist() == [31, 31, 31] and got["flags"].tolist() == [0, 0, 0]
    # a bin-centred sine of amplitude A reads A^2 / 2 in its band, mean and max alike; the constant and the alternating signal their square
    for kind in ("mean", "max"):
        assert abs(got[kind][0, 0] - 0.125) < 1e-5 and abs(got[kind][0, 1] - 0.005) < 1e-6 and got[kind][0, 2] < 1e-9 and got[kind][0, 3] < 1e-9
        assert abs(got[kind][1, 3] - 0.0625) < 1e-6 and got[kind][1, :3].max() < 1e-9
        assert abs(got[kind][2, 2] - 0.5625) < 1e-5 and got[kind][2, [0, 1, 3]].max() < 1e-9
    assert abs(got["total_mean"][0] - 0.13) < 1e-5 and abs(got["total_mean"][1] - 0.0625) < 1e-6 and abs(got["total_max"][2] - 0.5625) < 1e-5


@pytest.mark.parametrize("N", ref.FRAMES)
def test_random_audio_against_float64(bn, N):
    worst = 0.0
    for hop in (N, N // 2, 100):
        v, S, step, bands = ref.random_case(N, hop)
        rec = bn.Recording(v)
        assert rec.n_windows(step) == 5
        r = ref.band_levels(_f32(v), S, step, N, hop, bands)
        assert r["flags"].tolist() == [0, 0, ref.PADDED, ref.PADDED, ref.PADDED]
        worst = max(worst, _check(bn, rec.band_levels(S, step, N, hop, bands), r, len(bands), ("random", N, hop)))
    print("frame", N, "worst error / bound over hops N, N/2, 100:", worst)


def test_random_audio_at_the_models_segment(bn):
    N, hop = 1024, 512
    v = np.random.RandomState(11).randint(-20000, 20000, size=3 * SEG).astype(np.int16)
    bands = [VOICE, (0, 43), (200, 513)]
    r = ref.band_levels(_f32(v), SEG, SEG, N, hop, bands)
    assert r["n_frames"].tolist() == [280, 280, 280]
    share = _check(bn, bn.Recording(v).band_levels(SEG, SEG, N, hop, bands), r, 3, ("segment", N, hop))
    print("frame 1024 at S = 144000: worst error / bound", share)


@pytest.mark.parametrize("frames", (1, 3, 4, 5, 9))
def test_frames_per_wave(bn, frames):
    """four waves take frames w, w + 4, ...: waves with no frame, one frame and several"""
    N, hop = 256, 64
    S = N + (frames - 1) * hop
    v = np.random.RandomState(frames).randint(-32768, 32768, size=2 * S).astype(np.int16)
    bands = [(0, 129), (3, 17), (100, 129)]
    r = ref.band_levels(_f32(v), S, S, N, hop, bands)
    got = bn.Recording(v).band_levels(S, S, N, hop, bands)
    assert got["n_frames"].tolist() == [frames, frames]
    _check(bn, got, r, 3, ("frames", frames))


def test_a_window_depends_on_its_samples_alone(bn):
    S, N, hop, step = 2048, 512, 200, 1024
    bands = [(1, 40), (30, 257)]
    v = np.random.RandomState(21).randint(-32768, 32768, size=7 * step).astype(np.int16)
    v[5] = -32768
    x = _f32(v)
    rec = bn.Recording(v)
    whole = rec.band_levels(S, step, N, hop, bands)
    assert len(whole) == 7 and whole["flags"].tolist() == [0] * 6 + [ref.PADDED]
    _check(bn, whole, ref.band_levels(x, S, step, N, hop, bands), 2, "invariance base")
    # the same samples as F32 mono, as a selected channel of stereo I24 (a view of a recording created on the other channel) and as
    # the mix of two equal channels: (a + a) * 0.5 is a
    assert bn.Recording(x).band_levels(S, step, N, hop, bands).tobytes() == whole.tobytes()
    other = np.random.RandomState(22).randint(-2 ** 23, 2 ** 23, size=len(v)).astype(np.int64)
    raw = pcm_ref.pack(np.stack([v.astype(np.int64) * 256, other], axis=1), pcm_ref.I24)
    assert pcm_ref.mono(raw, pcm_ref.I24, 2, 0).tobytes() == x.tobytes()
    i24 = bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 1).view_channel(0)
    assert i24.band_levels(S, step, N, hop, bands).tobytes() == whole.tobytes()
    raw = pcm_ref.pack(np.stack([v.astype(np.int64) * 256] * 2, axis=1), pcm_ref.I24)
    assert pcm_ref.mono(raw, pcm_ref.I24, 2, pcm_ref.MIX).tobytes() == x.tobytes()
    assert bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, bn.BN_PCM_MIX).band_levels(S, step, N, hop, bands).tobytes() == whole.tobytes()
    # one call over [0, 7) against [0, 3), [3, 1) and [4, 3)
    parts = np.concatenate([rec.band_levels(S, step, N, hop, bands, 0, 3), rec.band_levels(S, step, N, hop, bands, 3, 1), rec.band_levels(S, step, N, hop, bands, 4, 3)])
    assert parts.tobytes() == whole.tobytes()
    assert len(rec.band_levels(S, step, N, hop, bands, 7, 0)) == 0
    # window k at step S is window 2 k at step S / 2
    wide = rec.band_levels(S, 2 * step, N, hop, bands)
    assert len(wide) == 4 and wide.tobytes() == whole[::2].tobytes()
    # the same samples deep inside a longer recording
    deep = bn.Recording(np.concatenate([np.random.RandomState(23).randint(-32768, 32768, size=37 * step).astype(np.int16), v]))
    assert deep.band_levels(S, step, N, hop, bands, 37, 7).tobytes() == whole.tobytes()


def test_padding_and_short_recordings(bn):
    S, N, hop = 4096, 256, 128
    bands = [(0, 129), (5, 60)]
    v = np.random.RandomState(31).randint(-32768, 32768, size=5000).astype(np.int16)
    got = bn.Recording(v).band_levels(S, S, N, hop, bands)
    assert got["flags"].tolist() == [0, ref.PADDED]
    _check(bn, got, ref.band_levels(_f32(v), S, S, N, hop, bands), 2, "padded")
    # the values are those of the same recording with the zeros stored
    full = bn.Recording(np.concatenate([v, np.zeros(2 * S - 5000, dtype=np.int16)])).band_levels(S, S, N, hop, bands)
    assert full["flags"].tolist() == [0, 0]
    for k in ("mean", "max", "total_mean", "total_max", "n_frames"):
        assert got[k].tobytes() == full[k].tobytes(), k
    # shorter than one frame: one window, n_frames from the rule, the frames past the end all zero
    short = bn.Recording(v[:100]).band_levels(S, S, N, hop, bands)
    assert short["n_frames"].tolist() == [31] and short["flags"].tolist() == [ref.PADDED]
    _check(bn, short, ref.band_levels(_f32(v[:100]), S, S, N, hop, bands), 2, "short")
    silent = bn.Recording(np.zeros(100, dtype=np.int16)).band_levels(S, S, N, hop, bands)
    assert silent["n_frames"].tolist() == [31] and silent["flags"].tolist() == [ref.PADDED]
    assert all(silent[k].tobytes() == bytes(silent[k].nbytes) for k in ("mean", "max", "total_mean", "total_max"))   # 0.0 exactly, not -0.0


def test_nonfinite_samples_and_the_unread_tail(bn):
    S, N, hop = 512, 256, 100    # 3 frames cover positions [0, 456): 56 are not read
    bands = [(0, 129), (10, 20)]
    x = np.random.RandomState(41).uniform(-1, 1, 4 * S).astype(np.float32)
    clean = bn.Recording(x).band_levels(S, S, N, hop, bands)
    _check(bn, clean, ref.band_levels(x, S, S, N, hop, bands), 2, "clean")
    y = x.copy()
    y[S + 200] = np.nan
    y[2 * S + 500] = np.inf
    got = bn.Recording(y).band_levels(S, S, N, hop, bands)
    r = ref.band_levels(y, S, S, N, hop, bands)
    assert got["flags"].tolist() == r["flags"].tolist() == [0, ref.NONFINITE, 0, 0] and got["n_frames"].tolist() == [3] * 4
    assert (got["mean"][1, :2] == np.inf).all() and (got["max"][1, :2] == np.inf).all() and got["total_mean"][1] == np.inf and got["total_max"][1] == np.inf
    assert not got["mean"][1, 2:].any() and not got["max"][1, 2:].any()
    # the Inf in the tail no frame covers is not read: that window, like the neighbours, has the clean bits
    assert got[[0, 2, 3]].tobytes() == clean[[0, 2, 3]].tobytes()
    for bad in (np.inf, -np.inf):
        y = x.copy()
        y[3 * S + 455] = bad     # the last position a frame reads
        assert bn.Recording(y).band_levels(S, S, N, hop, bands)["flags"].tolist() == [0, 0, 0, ref.NONFINITE]


def test_loudest_frame(bn):
    """a 20 ms call in a 3 s window is diluted in the mean and stands in the max"""
    N, hop = 1024, 512
    x = np.zeros(SEG)
    x[70000:70960] = _tone(960, 4000.0, 0.1)
    v = np.round(x * 32768).astype(np.int16)
    r = ref.band_levels(_f32(v), SEG, SEG, N, hop, [VOICE])
    got = bn.Recording(v).band_levels(SEG, SEG, N, hop, [VOICE])
    _check(bn, got, r, 1, "burst")
    print("burst: max / mean", got["max"][0, 0] / got["mean"][0, 0], "reference", r["max"][0, 0] / r["mean"][0, 0])
    assert got["max"][0, 0] > 8 * got["mean"][0, 0] > 0


def test_rumble_hides_a_call_from_the_peak_gate_but_not_from_the_band(bn):
    N, hop = 1024, 512
    assert bn.band_bins(RATE, N, 2000.0, 10000.0) == VOICE
    rumble = _tone(2 * SEG, 60.0, 0.1)                       # -20 dBFS
    call = np.concatenate([np.zeros(SEG), _tone(SEG, 5000.0, 10 ** -2.5)])   # -50 dBFS, second window only
    v = np.round((rumble + call) * 32768).astype(np.int16)
    r = ref.band_levels(_f32(v), SEG, SEG, N, hop, [VOICE])
    rec = bn.Recording(v)
    got = rec.band_levels(SEG, SEG, N, hop, [VOICE])
    _check(bn, got, r, 1, "rumble")
    for kind in ("mean", "max"):
        threshold = np.sqrt(r[kind][0, 0] * r[kind][1, 0])
        print("rumble:", kind, "quiet", got[kind][0, 0], "threshold", threshold, "call", got[kind][1, 0])
        assert r[kind][0, 0] < threshold < r[kind][1, 0] and got[kind][0, 0] < threshold < got[kind][1, 0]
    peak = rec.levels(SEG, SEG)["peak"]
    assert abs(peak[1] - peak[0]) < 0.05 * peak[0] and (peak >= 0.01).all()    # the broadband gate keeps both and cannot tell them apart


def test_overlapping_and_full_bands(bn):
    N, hop = 512, 256
    v, S, step, _ = ref.random_case(N, hop)
    x, rec, half = _f32(v), bn.Recording(v), N // 2
    bands = [(0, half + 1), (10, 100), (50, 200)]
    r = ref.band_levels(x, S, step, N, hop, bands)
    got = rec.band_levels(S, step, N, hop, bands)
    _check(bn, got, r, 3, "overlapping")
    # the band of all bins is the total, within delta (same terms, the same tree)
    delta = (bn.BN_BAND_SUM_DEPTH + -(-got["n_frames"].astype(np.float64) // 4)) * 2.0 ** -24
    assert (np.abs(got["mean"][:, 0].astype(np.float64) - got["total_mean"]) <= delta * got["total_mean"]).all()
    assert (np.abs(got["max"][:, 0].astype(np.float64) - got["total_max"]) <= delta * got["total_max"]).all()
    # BN_BAND_MAX bands at once; each equals the same band asked for alone, bit for bit
    eight = [(b, half + 1 - 7 * b) for b in range(bn.BN_BAND_MAX)]
    g8 = rec.band_levels(S, step, N, hop, eight)
    _check(bn, g8, ref.band_levels(x, S, step, N, hop, eight), 8, "eight bands")
    alone = rec.band_levels(S, step, N, hop, [eight[5]])
    assert alone["mean"][:, 0].tobytes() == g8["mean"][:, 5].tobytes() and alone["max"][:, 0].tobytes() == g8["max"][:, 5].tobytes()


def test_refusals_and_struct_size(bn):
    S, N, hop, step = 2048, 512, 256, 1024
    v = np.random.RandomState(51).randint(-32768, 32768, size=6 * step).astype(np.int16)
    rec = bn.Recording(v)
    good = bn.band_spec(N, hop, [(0, 10), (5, 257)])
    sizes = (C.sizeof(bn.BnBandSpec), C.sizeof(bn.BnWindowBands))

    def call(seg=S, stp=step, first=0, count=2, spec=good, spec_size=sizes[0], out=True, struct_size=sizes[1]):
        buf = np.full(2 * 24, 0xA5A5A5A5, dtype=np.uint32)
        st = bn.lib.bn_recording_band_levels(rec._h, seg, stp, first, count, None if spec is None else C.byref(spec), spec_size,
                                             buf.ctypes.data_as(C.POINTER(bn.BnWindowBands)) if out else None, struct_size)
        return st, buf

    eight = [(0, 1)] * 8
    nine = bn.band_spec(N, hop, eight)
    nine.n_bands = 9
    cases = ((dict(seg=S + 2), "multiple of 4"), (dict(stp=0), "step_samples"), (dict(first=5, count=2), "exceeds the 6 windows"),
             (dict(first=7, count=0), "exceeds the 6 windows"), (dict(out=False), "null"), (dict(struct_size=sizes[1] - 1), "struct_size"),
             (dict(spec=None), "null band spec"), (dict(spec_size=sizes[0] - 1), "spec_size"), (dict(spec=bn.band_spec(300, 100, [(0, 10)])), "frame"),
             (dict(spec=bn.band_spec(4096, 100, [(0, 10)])), "frame"), (dict(seg=256), "below the frame"), (dict(spec=bn.band_spec(N, 0, [(0, 10)])), "hop"),
             (dict(spec=bn.band_spec(N, N + 1, [(0, 10)])), "hop"), (dict(spec=bn.band_spec(N, hop, [])), "n_bands"), (dict(spec=nine), "n_bands"),
             (dict(spec=bn.band_spec(N, hop, [(0, 10), (7, 7)])), "band 1"), (dict(spec=bn.band_spec(N, hop, [(9, 3)])), "band 0"),
             (dict(spec=bn.band_spec(N, hop, [(0, 258)])), "band 0"))
    for kw, word in cases:
        st, buf = call(**kw)
        assert st == 1 and word in bn.last_error() and bn.last_error(), (kw, bn.last_error())
        assert (buf == 0xA5A5A5A5).all(), kw
    st, buf = call(count=0)
    assert st == 0 and (buf == 0xA5A5A5A5).all()
    # a caller compiled against a longer struct: its stride is kept, the bytes behind this header's fields are left alone
    st, buf = call(first=1, struct_size=96)
    rows = buf.reshape(2, 24)
    assert st == 0 and rows[:, :20].tobytes() == rec.band_levels(S, step, N, hop, [(0, 10), (5, 257)], 1, 2).tobytes() and (rows[:, 20:] == 0xA5A5A5A5).all()
    with pytest.raises(bn.EngineError) as e:
        rec.band_levels(S, step, 300, 100, [(0, 10)])
    assert e.value.status == 1


def test_host_mirror_and_asynchronous_upload(bn):
    N, hop = 1024, 512
    v = np.random.RandomState(61).randint(-32768, 32768, size=2 * SEG + 999).astype(np.int16)
    bands = [VOICE, (0, 43)]
    want = bn.Recording(v).band_levels(SEG, SEG, N, hop, bands)
    assert len(want) == 3
    host = bn.HostRecording(v)
    assert host.band_levels(SEG, SEG, N, hop, bands).tobytes() == want.tobytes()
    assert host.band_levels(SEG, SEG, N, hop, bands, 1, 2).tobytes() == want[1:].tobytes()
    with pytest.raises(bn.Error) as e:
        host.band_levels(SEG, SEG, 1000, hop, bands)
    assert e.value.kind == bn.ErrorKind.Inference
    a = bn.Recording(v, async_upload=True)
    assert a.band_levels(SEG, SEG, N, hop, bands).tobytes() == want.tobytes()
    a.wait()


def test_a_second_piece_continues_the_first(bn):
    """A call runs at most 2^20 windows per launch: 2^20 + 3 windows of one 256-sample frame at step 1 take two.  The rows either
    side of the cut (three whole windows, two that reach past the end) are those of a call on just that range (one piece), byte for
    byte, and the float64 reference's."""
    N = S = min(ref.FRAMES)
    piece, bands = 1 << 20, [(3, 40)]
    count = piece + 3
    v = np.random.RandomState(2021).randint(-32768, 32768, size=count + S - 3).astype(np.int16)
    rec = bn.Recording(v)
    whole = rec.band_levels(S, 1, N, N, bands, 0, count)
    first, n = piece - 2, 5
    edge = rec.band_levels(S, 1, N, N, bands, first, n)
    assert len(whole) == count and whole[first:].tobytes() == edge.tobytes()
    r = ref.band_levels(_f32(v[first:]), S, 1, N, N, bands, 0, n)  # the samples these windows read: the last S + 2
    assert r["flags"].tolist() == [0, 0, 0, ref.PADDED, ref.PADDED] and r["n_frames"].tolist() == [1] * n
    _check(bn, whole[first:], r, 1, "across the piece boundary")
