"""bn_recording_delay on the GPU against tests/delay_ref.py (float64, numpy.fft over frames cut by the rule).

Every float -- the curve, peak, before, after -- is compared within the header's bound (delay_ref.delay, from the BN_DELAY_* and
BN_BAND_* constants as the header declares them); peak_lag, flags and n_frames exactly; the invariance runs byte for byte.  peak_lag == d
is asserted wherever the reference's margin exceeds twice the bound, and tests/test_delay_cpu.py shows that this is every case.  Each test
prints its worst error as a share of the bound."""
import ctypes as C

import numpy as np
import pytest

import band_levels_ref as band
import delay_ref as ref
import denoise_ref
import pcm_ref

pytestmark = pytest.mark.gpu


def _check(bn, got, r, what):
    """got = (records, curves or None): flags and n_frames exactly, every float within the window's bound; returns the worst share"""
    rec, curve = got
    assert rec.dtype == bn.DELAY_DTYPE and rec["flags"].tolist() == r["flags"].tolist() and rec["n_frames"].tolist() == r["n_frames"].tolist(), what
    assert curve is None or (curve.dtype == np.float32 and curve.shape == r["curve"].shape), what
    share = ref.worst_share(rec, curve, r)
    print(what, "worst error / bound", share)
    assert share <= 1.0, (what, share)
    return share


@pytest.mark.parametrize("weighting", (ref.PLAIN, ref.PHAT))
@pytest.mark.parametrize("F", ref.FRAME_COUNTS)
@pytest.mark.parametrize("N", ref.FRAMES)
def test_against_float64_and_the_delay_is_found(bn, N, F, weighting):
    max_lag, worst, found = N // 8, 0.0, 0
    for d in ref.delays(N):
        a, b, S, hop = ref.pair(N, F, d)
        ra, rb = bn.Recording(a), bn.Recording(b)
        for bins in (ref.bands(N) if d == 3 else ref.bands(N)[:1]):
            r = ref.delay(ref.f32(a), ref.f32(b), S, S, N, hop, bins, max_lag, weighting)
            got = ra.delay(rb, S, S, N, hop, bins, max_lag, weighting, curve=True)
            worst = max(worst, _check(bn, got, r, (N, F, weighting, d, bins)))
            if bins == ref.bands(N)[0]:
                clear = r["margin"] > 2 * r["bound"]
                assert (got[0]["peak_lag"][clear] == d).all(), (N, F, weighting, d, got[0]["peak_lag"])
                found += int(clear.sum())
    assert found == 2 * len(ref.delays(N))  # no window of no delay was left out
    print("frame", N, "frames", F, "weighting", weighting, "worst error / bound:", worst)


@pytest.mark.parametrize("weighting", (ref.PLAIN, ref.PHAT))
def test_hop_of_one_sample(bn, weighting):
    N, F = 256, 5
    a, b, S, hop = ref.pair(N, F, -7, hop=1)
    assert S == 260
    got = bn.Recording(a).delay(bn.Recording(b), S, S, N, hop, (0, 129), 32, weighting, curve=True)
    _check(bn, got, ref.delay(ref.f32(a), ref.f32(b), S, S, N, hop, (0, 129), 32, weighting), ("hop 1", weighting))


def test_known_answers(bn):
    N, F, bins = 512, 5, (40, 104)
    a, _, S, hop = ref.pair(N, F, 0)
    x, ra = ref.f32(a), bn.Recording(a)
    # PLAIN against itself: r[0] is band levels' mean of the band, each within its own bound of the same float64 value
    r = ref.delay(x, x, S, S, N, hop, bins, 64, ref.PLAIN)
    rec = ra.delay(ra, S, S, N, hop, bins, 64, ref.PLAIN)[0]
    _check(bn, (rec, None), r, "self, plain")
    levels = ra.band_levels(S, S, N, hop, [bins])
    P = np.stack([band.frame_powers(x[k * S:(k + 1) * S].astype(np.float64), N, hop) for k in range(2)])
    level_bound = band.bound(P[:, :, bins[0]:bins[1]].sum(axis=2).mean(axis=1), P.sum(axis=2).mean(axis=1), F)
    assert rec["peak_lag"].tolist() == [0, 0] and (np.abs(rec["peak"].astype(np.float64) - levels["mean"][:, 0]) <= r["bound"] + level_bound).all()
    # PHAT against itself: one linear phase, the zero one
    r = ref.delay(x, x, S, S, N, hop, bins, 64, ref.PHAT)
    rec = ra.delay(ra, S, S, N, hop, bins, 64, ref.PHAT)[0]
    _check(bn, (rec, None), r, "self, phat")
    assert rec["peak_lag"].tolist() == [0, 0] and (np.abs(rec["peak"] - 1.0) <= r["bound"]).all()
    # bn_delay_refine on the device's record is the formula
    one = ra.delay(bn.Recording(np.roll(a, 3)), S, S, N, hop, (0, 257), 64, ref.PHAT)[0][0]
    p, bf, af = (np.float64(one[k]) for k in ("peak", "before", "after"))
    assert one["peak_lag"] == -3 and bn.delay_refine(one) == one["peak_lag"] + np.clip(0.5 * (bf - af) / (bf - 2 * p + af), -0.5, 0.5)
    # silence on either side: the all-zero record, lag 0 by the tie rule
    quiet = bn.Recording(np.zeros(2 * S, dtype=np.int16))
    for pair in ((ra, quiet), (quiet, ra), (quiet, quiet)):
        for weighting in (ref.PLAIN, ref.PHAT):
            rec, curve = pair[0].delay(pair[1], S, S, N, hop, bins, 64, weighting, curve=True)
            assert all(rec[k].tobytes() == bytes(8) for k in ("peak_lag", "peak", "before", "after", "flags")) and curve.tobytes() == bytes(curve.nbytes)


def test_sources(bn):
    N, F = 256, 5
    a, b, S, hop = ref.pair(N, F, 5, windows=3)
    args = (S, S, N, hop, (0, 129), 32)
    # two channel views of one I24 stereo upload
    stereo = bn.Recording.from_layout(pcm_ref.pack(np.stack([a.astype(np.int64) * 256 + 77, b.astype(np.int64) * 256 - 5], axis=1), pcm_ref.I24), bn.BN_PCM_I24, 2, 0)
    left, right = stereo.view_channel(0), stereo.view_channel(1)
    for weighting in (ref.PLAIN, ref.PHAT):
        got = left.delay(right, *args, weighting, curve=True)
        _check(bn, got, ref.delay(left.read_f32(), right.read_f32(), *args, weighting), ("I24 stereo views", weighting))
        assert got[0]["peak_lag"].tolist() == [5, 5, 5]
    # an asynchronous upload against a synchronous one
    late = bn.Recording(a, async_upload=True)
    _check(bn, late.delay(bn.Recording(b), *args, ref.PHAT, curve=True), ref.delay(ref.f32(a), ref.f32(b), *args, ref.PHAT), "async upload")
    # a denoised recording against its source, through a one-tap filter: both mono f32
    v, noise = denoise_ref.case(N, 3 * S)
    src = bn.Recording(v)
    clean, plain = src.denoised(N, noise, 2.0, 0.1), src.filtered([1.0])
    got = clean.delay(plain, *args, ref.PLAIN, curve=True)
    _check(bn, got, ref.delay(clean.read_f32(), plain.read_f32(), *args, ref.PLAIN), "denoised against its source")
    # the host mirror reaches the same entry point
    host = bn.HostRecording(a).delay(bn.HostRecording(b), *args, ref.PHAT, curve=True)
    mine = bn.Recording(a).delay(bn.Recording(b), *args, ref.PHAT, curve=True)
    assert host[0].tobytes() == mine[0].tobytes() and host[1].tobytes() == mine[1].tobytes()


@pytest.mark.parametrize("weighting", (ref.PLAIN, ref.PHAT))
def test_a_window_depends_on_its_samples_alone(bn, weighting):
    S, N, hop, step, bins, max_lag = 2048, 512, 200, 1024, (1, 257), 100
    rng = np.random.RandomState(21)
    a, b = (rng.randint(-32768, 32768, size=7 * step).astype(np.int16) for _ in range(2))
    ra, rb = bn.Recording(a), bn.Recording(b)
    whole, curves = ra.delay(rb, S, step, N, hop, bins, max_lag, weighting, curve=True)
    _check(bn, (whole, curves), ref.delay(ref.f32(a), ref.f32(b), S, step, N, hop, bins, max_lag, weighting), "invariance base")

    def same(got, rows=slice(None)):
        return got[0].tobytes() == whole[rows].tobytes() and got[1].tobytes() == curves[rows].tobytes()

    # without the curve: the same records, and None
    bare = ra.delay(rb, S, step, N, hop, bins, max_lag, weighting)
    assert bare[0].tobytes() == whole.tobytes() and bare[1] is None
    # one range against two calls; another first_window and step; f32 of the same samples; a shorter b ends the range, not the bits
    assert same(ra.delay(rb, S, step, N, hop, bins, max_lag, weighting, True, 0, 3), slice(0, 3))
    assert same(ra.delay(rb, S, step, N, hop, bins, max_lag, weighting, True, 3, 4), slice(3, 7))
    assert same(ra.delay(rb, S, 2 * step, N, hop, bins, max_lag, weighting, True, 1, 2), slice(2, 6, 2))
    assert same(bn.Recording(ref.f32(a)).delay(bn.Recording(ref.f32(b)), S, step, N, hop, bins, max_lag, weighting, True))
    longer = bn.Recording(np.concatenate([b, rng.randint(-32768, 32768, size=3 * step).astype(np.int16)]))
    assert same(ra.delay(longer, S, step, N, hop, bins, max_lag, weighting, True, 0, 5), slice(0, 5)) and len(ra.delay(longer, S, step, N, hop, bins, max_lag)[0]) == 7
    # a NaN in one window of b: that window is flagged and NaN, no other window changes a bit
    y = ref.f32(b).copy()
    y[3 * step + 1500] = np.nan  # windows 3 and 4 read it
    got = bn.Recording(ref.f32(a)).delay(bn.Recording(y), S, step, N, hop, bins, max_lag, weighting, True)
    _check(bn, got, ref.delay(ref.f32(a), y, S, step, N, hop, bins, max_lag, weighting), "a NaN in b")
    hit, rest = [3, 4], [0, 1, 2, 5, 6]
    assert got[0]["flags"][hit].tolist() == [ref.NONFINITE, ref.NONFINITE] and got[0]["peak_lag"][hit].tolist() == [0, 0] and np.isnan(got[1][hit]).all()
    assert all(np.isnan(got[0][k][hit]).all() for k in ("peak", "before", "after"))
    assert got[0][rest].tobytes() == whole[rest].tobytes() and got[1][rest].tobytes() == curves[rest].tobytes()


@pytest.mark.parametrize("kw,word", [
    (dict(a=False), "null recording"), (dict(b=False), "null recording"), (dict(spec=None), "null delay spec"), (dict(out=False), "null output"),
    (dict(spec_size=23), "spec_size"), (dict(struct_size=23), "struct_size"), (dict(seg=2050), "multiple of 4"), (dict(seg=256), "below the frame"),
    (dict(first=5), "exceeds the 6 windows"), (dict(spec=(300, 100, 5, 15, 10, 1)), "frame"), (dict(spec=(512, 0, 5, 15, 10, 1)), "hop"),
    (dict(spec=(512, 513, 5, 15, 10, 1)), "hop"), (dict(spec=(512, 256, 7, 7, 10, 1)), "bins ["), (dict(spec=(512, 256, 0, 258, 10, 1)), "bins ["),
    (dict(spec=(512, 256, 5, 15, 256, 1)), "max_lag"), (dict(spec=(512, 256, 5, 15, 10, 2)), "weighting"), (dict(mixed=True), "mono int16 and mono f32")])
def test_refusals(bn, kw, word):
    S, step = 2048, 1024
    v = np.arange(6 * step, dtype=np.int16)
    ra, rb = bn.Recording(v), bn.Recording(ref.f32(v) if kw.get("mixed") else v)
    buf, curve = np.full(2 * 6, 0xA5A5A5A5, dtype=np.uint32), np.full(2 * 21, 7.0, dtype=np.float32)
    spec = kw.get("spec", (512, 256, 5, 15, 10, 1))
    st = bn.lib.bn_recording_delay(ra._h if kw.get("a", True) else None, rb._h if kw.get("b", True) else None, kw.get("seg", S), step, kw.get("first", 0), 2,
                                   None if spec is None else C.byref(bn.BnDelaySpec(*spec)), kw.get("spec_size", 24),
                                   buf.ctypes.data_as(C.POINTER(bn.BnWindowDelay)) if kw.get("out", True) else None, kw.get("struct_size", 24),
                                   curve.ctypes.data_as(C.POINTER(C.c_float)))
    assert st == 1 and word in bn.last_error() and (buf == 0xA5A5A5A5).all() and (curve == 7.0).all(), bn.last_error()


def test_count_zero_and_a_longer_struct(bn):
    S, step, spec = 2048, 1024, (512, 256, 5, 15, 10, 1)
    rec = bn.Recording(np.random.RandomState(51).randint(-32768, 32768, size=6 * step).astype(np.int16))
    buf = np.full(2 * 8, 0xA5A5A5A5, dtype=np.uint32)
    out, sp = buf.ctypes.data_as(C.POINTER(bn.BnWindowDelay)), bn.BnDelaySpec(*spec)
    assert bn.lib.bn_recording_delay(rec._h, rec._h, S, step, 0, 0, C.byref(sp), 24, out, 24, None) == 0 and (buf == 0xA5A5A5A5).all()
    # a caller compiled against a longer struct: its stride is kept, the bytes behind this header's fields are left alone
    assert bn.lib.bn_recording_delay(rec._h, rec._h, S, step, 1, 2, C.byref(sp), 24, out, 32, None) == 0
    want = rec.delay(rec, S, step, 512, 256, (5, 15), 10, 1, first=1, count=2)[0]
    assert buf.reshape(2, 8)[:, :6].tobytes() == want.tobytes() and (buf.reshape(2, 8)[:, 6:] == 0xA5A5A5A5).all()
