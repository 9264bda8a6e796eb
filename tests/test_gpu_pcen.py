"""bn_recording_pcen on the GPU against tests/pcen_ref.py (float64, a plain loop over frames).

The reference's input is the float32 image the device's own spectrogram() returns for the same range, so only the new stage is
under test.  Every float is compared within the header's two bounds (the smoother through state_out, the value per element), U8
images byte for byte against the table applied to the F32 image, the invariance byte for byte.  Each comparison prints its worst
error as a share of the bound and the worst value error in units of u * (V + delta^r) with the smoother's share taken off: the
figure BN_PCEN_VALUE_DEPTH is four times of ("PCEN").

The issue's row case "bins 0..260 at frame 512" does not exist (frame 512 has 257 bins); all 257 bins are four row blocks and one
row, the same edge."""
import ctypes as C

import numpy as np
import pytest

import pcm_ref
import pcen_ref as ref

pytestmark = pytest.mark.gpu
CHUNK, HOP, GAIN, T_MAX = 128, 100, 1e5, 3 * 128 + 5
PARAMS = ((0.98, 2.0, 0.5, 1e-6), (0.8, 10.0, 0.25, 1e-9), (1.0, 0.0, 1.0, 1e-6))
ROWS = {"1": (256, (5, 6)), "3": (256, (5, 8)), "64": (256, (5, 69)), "65": (256, (5, 70)), "257": (512, (0, 257)), "mel": (512, None)}
SCENES = {}


def _samples(n, seed=3):
    """white int16 noise with a 40 dB level step up at 40 % and a short loud burst at 70 %: M rises, and decays"""
    rng = np.random.RandomState(seed)
    level = np.where(np.arange(n) < 0.4 * n, 30.0, 3000.0)
    level[int(0.7 * n):int(0.7 * n) + 700] = 30000.0
    return np.clip(rng.standard_normal(n) * level / 3.0, -32768, 32767).astype(np.int16)


def _scene(bn, rows):
    """(recording, frame, the spectrogram's row arguments, its float32 image of T_MAX frames), made once per kind of rows"""
    if rows not in SCENES:
        N, bins = ROWS[rows]
        rec = bn.Recording(_samples((T_MAX - 1) * HOP + N))
        kw = {"bins": bins} if bins else {"bank": bn.Filterbank(0, N, bn.mel_filterbank(48000, N, 40, 0.0, 24000.0))}
        SCENES[rows] = (rec, N, kw, rec.spectrogram(0, T_MAX, N, HOP, **kw))
    return SCENES[rows]


def _check(got, state, E, s, p, what, state_in=None, keep=None):
    """the image within the value bound (+Inf exactly where the reference has it), state_out within the smoother's"""
    V, M, B, bound, M_end, B_end = ref.pcen(E, s, GAIN, *p, state=state_in, keep=keep)
    assert got.dtype == np.float32 and got.shape == V.shape and state.dtype == np.float32, what
    inf = np.isinf(V)
    assert (np.isinf(got) == inf).all() and (got[inf] > 0).all(), what
    err, y = np.abs(np.where(inf, 0.0, got).astype(np.float64) - np.where(inf, 0.0, V))[~inf], (V + np.float32(p[1]).astype(np.float64) ** float(np.float32(p[2])))[~inf]
    alpha, r, eps = (float(np.float32(v)) for v in (p[0], p[2], p[3]))
    ratio = (err / y - alpha * r * (B / (eps + M))[~inf]) / ref.U if err.size else np.zeros(1)
    share, m_share = (err / bound[~inf]).max() if err.size else 0.0, (np.abs(state - M_end) / np.maximum(B_end, 1e-300)).max()
    print(what, "value error / bound", share, "| in u (V + delta^r), smoother's share off", ratio.max(), "| state error / bound", m_share)
    assert share <= 1.0 and ((np.abs(state - M_end) <= B_end)).all(), (what, share, m_share)
    return V


@pytest.mark.parametrize("n_frames", (1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5))
@pytest.mark.parametrize("rows", sorted(ROWS))
def test_against_float64(bn, rows, n_frames):
    """one frame, a chunk less one, a whole chunk, one frame into the next, three chunks and a partial one; a lane, three, a full
    wave, one row into the next wave, four row blocks and a row, a bank; a slow, a very slow and no smoother; three compressions"""
    rec, N, kw, E = _scene(bn, rows)
    for s in (0.025, 0.001, 1.0):
        for p in PARAMS:
            got, state = rec.pcen(0, n_frames, N, HOP, smooth=s, gain=GAIN, alpha=p[0], delta=p[1], r=p[2], eps=p[3], **kw)
            _check(got, state, E[:n_frames], s, p, (rows, n_frames, s, p))
            if s == 1.0:  # M is x, exactly
                assert state.tobytes() == (np.float32(GAIN) * E[n_frames - 1]).tobytes()


def test_state_continues_a_range(bn):
    rec, N, kw, E = _scene(bn, "65")
    cut, n, p = CHUNK + 7, 2 * CHUNK + 50, PARAMS[0]
    a, st = rec.pcen(0, cut, N, HOP, smooth=0.025, gain=GAIN, **kw)
    b, st2 = rec.pcen(cut * HOP, n - cut, N, HOP, smooth=0.025, gain=GAIN, state=st, **kw)
    _check(np.concatenate([a, b]), st2, E[:n], 0.025, p, "split at CHUNK + 7")
    # a caller's state is where M starts; no frames: it comes back
    got, state = rec.pcen(0, 40, N, HOP, smooth=0.025, gain=GAIN, state=np.full(65, 0.5, np.float32), **kw)
    _check(got, state, E[:40], 0.025, p, "a state of 0.5", state_in=np.full(65, 0.5, np.float32))
    assert rec.pcen(0, 0, N, HOP, state=st, **kw)[1].tobytes() == st.tobytes() and not rec.pcen(0, 0, N, HOP, **kw)[1].any()


@pytest.mark.parametrize("rows", ("3", "257"))
def test_u8_is_the_table(bn, rows):
    rec, N, kw, _ = _scene(bn, rows)
    img, st = rec.pcen(0, T_MAX, N, HOP, smooth=0.025, gain=GAIN, **kw)
    mx = float(np.percentile(img, 90))
    codes, st8 = rec.pcen(0, T_MAX, N, HOP, smooth=0.025, gain=GAIN, u8=mx, **kw)
    assert codes.dtype == np.uint8 and len(np.unique(codes)) > 100 and st8.tobytes() == st.tobytes()
    assert codes.tobytes() == np.searchsorted(bn.pcen_thresholds(mx), img, side="right").astype(np.uint8).tobytes()


def test_non_finite_elements_are_skipped(bn):
    """a NaN sample in frame 0 alone, one in frames 126 .. 128 (a chunk's last two frames and the next one's first), one in frames
    198 .. 200 (the middle of a chunk): +Inf / 255 there, and the bound of the reference that skips them everywhere else"""
    N, n = 256, 2 * CHUNK + 9
    x = _samples((n - 1) * HOP + N).astype(np.float32) / 32768.0
    x[[50, 128 * HOP + 20, 200 * HOP + 50]] = np.nan
    rec = bn.Recording(x)
    E = rec.spectrogram(0, n, N, HOP, bins=(5, 70))
    bad = np.isinf(E[:, 0])
    assert np.flatnonzero(bad).tolist() == [0, 126, 127, 128, 198, 199, 200]
    for s in (0.025, 1.0):
        got, state = rec.pcen(0, n, N, HOP, bins=(5, 70), smooth=s, gain=GAIN)
        _check(got, state, E, s, PARAMS[0], ("NaN frames", s))
        codes, _ = rec.pcen(0, n, N, HOP, bins=(5, 70), smooth=s, gain=GAIN, u8=4.0)
        assert (codes[bad] == 255).all() and codes.tobytes() == np.searchsorted(bn.pcen_thresholds(4.0), got, side="right").astype(np.uint8).tobytes()
    # an overflowing gain * E is such an element too
    loud = bn.Recording((np.random.RandomState(1).standard_normal(3 * HOP + N) * 1e15).astype(np.float32))
    assert np.isfinite(loud.spectrogram(0, 3, N, HOP, bins=(5, 70))).all()
    got, state = loud.pcen(0, 3, N, HOP, bins=(5, 70), smooth=0.025, gain=1e30)
    assert np.isinf(got).all() and not state.any()


def test_a_launch_piece_is_crossed(bn):
    """all 1025 bins of frame 2048 at hop 1: the second launch piece starts at frame 65 408.  Compared: every 97th frame, the two
    chunks in front of the cut and everything behind it, and state_out"""
    N, piece = 2048, ((2 ** 26 // 1025) & ~15) // CHUNK * CHUNK
    n = ((2 ** 26 // 1025) & ~15) + CHUNK + 3
    rec = bn.Recording(_samples(n + N))
    E = rec.spectrogram(0, n, N, 1, bins=(0, 1025))
    got, state = rec.pcen(0, n, N, 1, bins=(0, 1025), smooth=0.001, gain=GAIN)
    keep = np.zeros(n, bool)
    keep[::97], keep[piece - 2 * CHUNK:] = True, True
    _check(got[keep], state, E, 0.001, PARAMS[0], "two pieces", keep=keep)


def test_invariance_byte_for_byte(bn):
    s0, n, rng, N = 333, CHUNK + 40, np.random.RandomState(5), 256
    vals = rng.randint(-2 ** 23, 2 ** 23, size=(s0 + (n + 5) * HOP + N - 77, 2))
    raw = pcm_ref.pack(vals, pcm_ref.I24)
    kind = {"bins": (2, 80), "smooth": 0.025, "gain": GAIN, "u8": 3.0}
    rec = bn.Recording(pcm_ref.mono(raw, pcm_ref.I24, 2, 1))
    whole, state = rec.pcen(s0, n, N, HOP, **kind)
    for other in (rec, bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 1), bn.HostRecording(raw, bn.BN_PCM_I24, 2, 1)):
        again, state2 = other.pcen(s0, n, N, HOP, **kind)
        assert again.tobytes() == whole.tobytes() and state2.tobytes() == state.tobytes()
    # a longer call: the same bits in front
    assert rec.pcen(s0, n + 5, N, HOP, **kind)[0][:n].tobytes() == whole.tobytes()


def test_refusals_leave_the_output_untouched(bn):
    L, N = bn.lib, 256
    rec, fb = bn.Recording(np.zeros(1000, dtype=np.float32)), bn.Filterbank(0, N, np.ones((3, 129), np.float32))
    out, st = np.full(4 * 40 + 2, 0x5A5A5A5A, dtype=np.uint32), np.full(41, 0x5A5A5A5A, dtype=np.uint32)
    good = (0, 0.025, 1e5, 0.98, 2.0, 0.5, 1e-6, 0.0)

    def call(r=rec._h, first=0, n=4, spec=(N, 100, 0, 40, 0, 0.0, 0.0), size=28, bank=None, pcen=good, psize=32, o=out, nbytes=4 * 40 * 4, **field):
        sp, ps = bn.BnSpectrogramSpec(*spec) if spec else None, bn.BnPcenSpec(*pcen) if pcen else None
        for k, v in field.items():
            setattr(ps, k, v)
        return L.bn_recording_pcen(r, first, n, C.byref(sp) if sp else None, size, bank, C.byref(ps) if ps else None, psize, None,
                                   st.ctypes.data_as(C.POINTER(C.c_float)), o.ctypes.data_as(C.c_void_p) if o is not None else None, nbytes)

    nan, inf = float("nan"), float("inf")
    for kw, word in (({"r": None}, "null recording"), ({"spec": None}, "null spectrogram spec"), ({"size": 27}, "spec_size"), ({"spec": (1000, 100, 0, 40, 0, 0.0, 0.0)}, "frame 1000"),
                     ({"spec": (N, 0, 0, 40, 0, 0.0, 0.0)}, "hop 0"), ({"spec": (N, 100, 5, 5, 0, 0.0, 0.0)}, "bins ["), ({"spec": (N, 100, 0, 40, 2, 0.0, 0.0)}, "unknown spectrogram format"),
                     ({"bank": fb._h}, "must both be 0"), ({"first": 1001}, "first_sample 1001"), ({"spec": (N, 100, 0, 40, 1, 1.0, 80.0)}, "F32"),
                     ({"pcen": None}, "null PCEN spec"), ({"psize": 31}, "pcen_size"), ({"format": 2}, "unknown PCEN format 2"),
                     ({"smooth": 0.0}, "smooth"), ({"smooth": 1.5}, "smooth"), ({"smooth": nan}, "smooth"), ({"gain": 0.0}, "gain"), ({"gain": inf}, "gain"), ({"gain": nan}, "gain"),
                     ({"alpha": -0.5}, "alpha"), ({"alpha": 1.5}, "alpha"), ({"alpha": nan}, "alpha"), ({"delta": -1.0}, "delta"), ({"delta": inf}, "delta"), ({"delta": nan}, "delta"),
                     ({"eps": 0.0}, "eps"), ({"eps": inf}, "eps"), ({"eps": nan}, "eps"),
                     ({"format": 1}, "max_value"), ({"format": 1, "max_value": inf}, "max_value"), ({"format": 1, "max_value": nan}, "max_value"),
                     ({"n": 2 ** 63}, "do not fit"), ({"o": None}, "null output"), ({"nbytes": 4 * 40 * 4 - 1}, "out_bytes")):
        assert call(**kw) == 1 and word in bn.last_error(), (kw, bn.last_error())
    ps = bn.BnPcenSpec(*good)
    for v in (0.0, 1.5, nan):  # the field r shares its name with the recording argument of call()
        ps.r = v
        assert L.bn_recording_pcen(rec._h, 0, 4, C.byref(bn.BnSpectrogramSpec(N, 100, 0, 40, 0, 0.0, 0.0)), 28, None, C.byref(ps), 32, None, None,
                                   out.ctypes.data_as(C.c_void_p), 640) == 1 and "r must" in bn.last_error()
    assert (out == 0x5A5A5A5A).all() and (st == 0x5A5A5A5A).all()
    assert call(n=0, nbytes=0, o=None) == 0 and (st == 0x5A5A5A5A).all()
    assert call() == 0 and (out[160:] == 0x5A5A5A5A).all() and not out[:160].any() and not st[:40].any() and st[40] == 0x5A5A5A5A  # silence: V is exactly 0
    with pytest.raises(bn.EngineError):
        bn.pcen_thresholds(0.0)
    assert "max_value" in bn.last_error()
