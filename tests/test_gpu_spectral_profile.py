"""bn_recording_spectral_profile on the GPU against tests/spectral_profile_ref.py (float64, numpy.fft.rfft over frames cut by the rule).

Every float -- the three planes, aci, total_mean -- is compared within the header's bound (spectral_profile_ref.bounds, from the
BN_PROFILE_* and BN_BAND_* constants as the header declares them); flags and n_frames exactly; the invariance runs byte for byte.
tests/test_spectral_profile_cpu.py shows on the random-audio inputs below that four wrong rules leave those bounds and that the ACI
bound is below 1 % of the ACI.  Each test prints its worst error as a share of the bound."""
import ctypes as C

import numpy as np
import pytest

import pcm_ref
import spectral_profile_ref as ref

pytestmark = pytest.mark.gpu
SEG = 144000


def _check(bn, got, r, what):
    """got = (records, planes or None): flags and n_frames exactly, every float within its bound; returns the worst share"""
    rec, planes = got
    assert rec.dtype == bn.PROFILE_DTYPE and rec["flags"].tolist() == r["flags"].tolist() and rec["n_frames"].tolist() == r["n_frames"].tolist(), what
    g = {"aci": rec["aci"], "total_mean": rec["total_mean"]}
    if planes is not None:
        assert planes.dtype == np.float32 and planes.shape == r["planes"].shape, what
        g["planes"] = planes
    shares = ref.worst_share(g, r)
    print(what, "worst error / bound", shares)
    assert max(shares.values()) <= 1.0, (what, shares)
    return max(shares.values())


def _f32(v):
    return pcm_ref.mono(pcm_ref.pack(v, pcm_ref.I16), pcm_ref.I16, 1, 0)


def test_known_answers(bn):
    """window 0: a bin-centred sine whose amplitude alternates a, b from frame to frame; window 1: a steady sine; window 2: silence"""
    N, S, k0, a, b = 256, 4096, 20, 0.5, 0.2
    s = np.sin(2 * np.pi * k0 * np.arange(S) / N)
    x = np.concatenate([np.repeat(np.where(np.arange(S // N) % 2 == 0, a, b), N) * s, a * s, np.zeros(S)]).astype(np.float32)
    rec = bn.Recording(x)
    for bins in ((k0 - 1, k0 + 2), (0, N // 2 + 1)):
        got = rec.spectral_profile(S, S, N, N, bins)
        _check(bn, got, ref.profile(x, S, S, N, N, bins), ("known answers", bins))
    (p, planes), centre = got, np.sqrt(2.0 / 3.0)  # the centre bin of a Hann-windowed sine holds 2/3 of its power
    assert p["n_frames"].tolist() == [16] * 3 and p["flags"].tolist() == [0] * 3
    assert abs(planes[0, 2, k0] - 15 * (a - b) / np.sqrt(2) * centre) < 1e-5 and abs(planes[0, 1, k0] - 8 * (a + b) / np.sqrt(2) * centre) < 1e-5
    assert abs(planes[0, 0, k0 - 1:k0 + 2].sum() - (a * a + b * b) / 4) < 1e-6 and abs(p["total_mean"][0] - (a * a + b * b) / 4) < 1e-6
    narrow = rec.spectral_profile(S, S, N, N, (k0, k0 + 1))[0]
    assert abs(narrow["aci"][0] - 15 * (a - b) / (8 * (a + b))) < 1e-5 and 0 <= narrow["aci"][1] < 1e-5
    # silence: 0.0 everywhere, and an ACI of 0, not NaN
    assert planes[2].tobytes() == bytes(planes[2].nbytes) and p["aci"][2].tobytes() + p["total_mean"][2].tobytes() == bytes(8)


@pytest.mark.parametrize("N", ref.FRAMES)
def test_random_audio_against_float64(bn, N):
    worst = 0.0
    for hop in (N, N // 2, 100):
        v, S, step = ref.random_case(N, hop)
        rec, x = bn.Recording(v), _f32(v)
        for bins in ref.bin_ranges(N):
            r = ref.profile(x, S, step, N, hop, bins)
            assert r["flags"].tolist() == [0, 0, ref.PADDED, ref.PADDED, ref.PADDED]
            worst = max(worst, _check(bn, rec.spectral_profile(S, step, N, hop, bins), r, ("random", N, hop, bins)))
    print("frame", N, "worst error / bound over hops N, N/2, 100:", worst)


@pytest.mark.parametrize("frames", (1, 2, 3, 4, 5, 8, 9))
def test_frames_per_run(bn, frames):
    """runs of ceil(F / 4) frames: waves with no frame, with one frame and no successor, runs of uneven length; a difference across a
    run boundary that is lost or counted twice leaves plane 2's bound"""
    N, hop = 256, 64
    S = N + (frames - 1) * hop
    v = np.random.RandomState(frames).randint(-32768, 32768, size=2 * S).astype(np.int16)
    got = bn.Recording(v).spectral_profile(S, S, N, hop, (0, 129))
    assert got[0]["n_frames"].tolist() == [frames, frames]
    _check(bn, got, ref.profile(_f32(v), S, S, N, hop, (0, 129)), ("frames", frames))


def test_the_models_segment(bn):
    N, hop = 1024, 512
    v = np.random.RandomState(11).randint(-20000, 20000, size=2 * SEG).astype(np.int16)
    r = ref.profile(_f32(v), SEG, SEG, N, hop, (0, 513))
    assert r["n_frames"].tolist() == [280, 280]
    _check(bn, bn.Recording(v).spectral_profile(SEG, SEG, N, hop, (0, 513)), r, "segment: 280 frames in runs of 70")


def test_a_window_depends_on_its_samples_alone(bn):
    S, N, hop, step, bins = 2048, 512, 200, 1024, (1, 257)
    v = np.random.RandomState(21).randint(-32768, 32768, size=7 * step).astype(np.int16)
    x, rec = _f32(v), bn.Recording(v)
    whole, planes = rec.spectral_profile(S, step, N, hop, bins)
    _check(bn, (whole, planes), ref.profile(x, S, step, N, hop, bins), "invariance base")

    def same(got, rows=slice(None)):
        return got[0].tobytes() == whole[rows].tobytes() and got[1].tobytes() == planes[rows].tobytes()

    # without the planes: the same records, and None
    assert rec.spectral_profile(S, step, N, hop, bins, planes=False)[0].tobytes() == whole.tobytes() and rec.spectral_profile(S, step, N, hop, bins, planes=False)[1] is None
    # the same samples as F32 mono and as a channel view of stereo I24
    assert same(bn.Recording(x).spectral_profile(S, step, N, hop, bins))
    other = np.random.RandomState(22).randint(-2 ** 23, 2 ** 23, size=len(v)).astype(np.int64)
    raw = pcm_ref.pack(np.stack([v.astype(np.int64) * 256, other], axis=1), pcm_ref.I24)
    assert same(bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 1).view_channel(0).spectral_profile(S, step, N, hop, bins))
    # one range against two calls; another first_window and step; deep inside a longer recording; the host mirror
    assert same(rec.spectral_profile(S, step, N, hop, bins, 0, 3), slice(0, 3)) and same(rec.spectral_profile(S, step, N, hop, bins, 3, 4), slice(3, 7))
    assert same(rec.spectral_profile(S, 2 * step, N, hop, bins, 1, 2), slice(2, 6, 2))
    deep = bn.Recording(np.concatenate([np.random.RandomState(23).randint(-32768, 32768, size=37 * step).astype(np.int16), v]))
    assert same(deep.spectral_profile(S, step, N, hop, bins, 37, 7))
    assert same(bn.HostRecording(v).spectral_profile(S, step, N, hop, bins)) and len(rec.spectral_profile(S, step, N, hop, bins, 7, 0)[0]) == 0


def test_nonfinite_samples_and_the_unread_tail(bn):
    S, N, hop, bins = 512, 256, 100, (0, 129)    # 3 frames cover positions [0, 456): 56 are not read
    x = np.random.RandomState(41).uniform(-1, 1, 4 * S).astype(np.float32)
    clean = bn.Recording(x).spectral_profile(S, S, N, hop, bins)
    y = x.copy()
    y[S + 200] = np.nan
    y[2 * S + 500] = np.nan  # in the tail no frame covers
    got = bn.Recording(y).spectral_profile(S, S, N, hop, bins)
    _check(bn, got, ref.profile(y, S, S, N, hop, bins), "one NaN read, one not")
    assert got[0]["flags"].tolist() == [0, ref.NONFINITE, 0, 0] and got[0]["aci"][1] == np.inf and got[0]["total_mean"][1] == np.inf and (got[1][1] == np.inf).all()
    assert got[0][[0, 2, 3]].tobytes() == clean[0][[0, 2, 3]].tobytes() and got[1][[0, 2, 3]].tobytes() == clean[1][[0, 2, 3]].tobytes()


def test_refusals_and_struct_size(bn):
    S, N, hop, step = 2048, 512, 256, 1024
    rec = bn.Recording(np.random.RandomState(51).randint(-32768, 32768, size=6 * step).astype(np.int16))

    def call(seg=S, first=0, count=2, spec=(N, hop, 5, 15), spec_size=16, out=True, struct_size=16):
        buf, pl = np.full(2 * 6, 0xA5A5A5A5, dtype=np.uint32), np.full(2 * 3 * 10, 7.0, dtype=np.float32)
        sp = None if spec is None else C.byref(bn.BnProfileSpec(*spec))
        st = bn.lib.bn_recording_spectral_profile(rec._h, seg, step, first, count, sp, spec_size, buf.ctypes.data_as(C.POINTER(bn.BnWindowProfile)) if out else None,
                                                  struct_size, pl.ctypes.data_as(C.POINTER(C.c_float)))
        return st, buf, pl

    for kw, word in ((dict(seg=S + 2), "multiple of 4"), (dict(first=5), "exceeds the 6 windows"), (dict(out=False), "null"), (dict(struct_size=15), "struct_size"),
                     (dict(spec=None), "null profile spec"), (dict(spec_size=15), "spec_size"), (dict(spec=(300, 100, 5, 15)), "frame"), (dict(seg=256), "below the frame"),
                     (dict(spec=(N, 0, 5, 15)), "hop"), (dict(spec=(N, N + 1, 5, 15)), "hop"), (dict(spec=(N, hop, 7, 7)), "bins ["), (dict(spec=(N, hop, 0, 258)), "bins [")):
        st, buf, pl = call(**kw)
        assert st == 1 and word in bn.last_error() and (buf == 0xA5A5A5A5).all() and (pl == 7.0).all(), (kw, bn.last_error())
    st, buf, pl = call(count=0)
    assert st == 0 and (buf == 0xA5A5A5A5).all() and (pl == 7.0).all()
    # a caller compiled against a longer struct: its stride is kept, the bytes behind this header's fields are left alone
    st, buf, pl = call(first=1, struct_size=24)
    want = rec.spectral_profile(S, step, N, hop, (5, 15), 1, 2)
    assert st == 0 and buf.reshape(2, 6)[:, :4].tobytes() == want[0].tobytes() and (buf.reshape(2, 6)[:, 4:] == 0xA5A5A5A5).all() and pl.tobytes() == want[1].tobytes()
