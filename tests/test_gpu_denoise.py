"""bn_recording_create_denoised on the GPU against tests/denoise_ref.py (the rule in float64 on the same f32 samples): every output
block within the header's bound (denoise_ref.shares, from BN_DENOISE_* and BN_BAND_EPS_ULPS as the header declares them), the known
answers, the invariance bit for bit, the result as an ordinary recording, and the refusals.  tests/test_denoise_cpu.py shows on the
bound test's inputs that five wrong rules leave that bound.  W = 4 RUN H samples are one workgroup's; each test prints its worst
error as a share of the bound."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as ref
import pcm_ref

pytestmark = pytest.mark.gpu


def _worst(got, x, N, alpha, floor_gain, noise, what, want=None):
    y, E = ref.denoise(x, N, alpha, floor_gain, noise)
    s = ref.shares(got, y if want is None else want, E, N)
    print(what, "worst error / bound", s.max())
    assert len(got) == len(x) and s.max() <= 1.0, (what, int(s.argmax()), s.max())


# n = a + b H + c W: 1, H - 1, H, W, W + 1, 2 W + H + 3
@pytest.mark.parametrize("a,b,c", [(1, 0, 0), (-1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (3, 1, 2)])
@pytest.mark.parametrize("N", ref.FRAMES)
def test_noise_and_tone_against_float64(bn, N, a, b, c):
    H = N // 2
    n = a + b * H + c * 4 * bn.BN_DENOISE_RUN * H
    v, noise = ref.case(N, n)
    got = bn.Recording(v).denoised(N, noise, 2.0, 0.1).read_f32()
    _worst(got, v.astype(np.float32) / np.float32(32768.0), N, 2.0, 0.1, noise, ("random", N, n))


@pytest.mark.parametrize("kind", ["i24 stereo mix-down", "channel view", "asynchronous upload"])
def test_other_sources_against_float64(bn, kind):
    N, n = 512, 4 * bn.BN_DENOISE_RUN * 256 + 300
    v, noise = ref.case(N, n)
    if kind == "asynchronous upload":
        src = bn.Recording(v, async_upload=True)
    else:
        raw = pcm_ref.test_data(np.random.RandomState(2), pcm_ref.I24, n, 2)
        src = bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, bn.BN_PCM_MIX) if kind.startswith("i24") else bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 0).view_channel(1)
        noise = ref.white_level(N, 0.5)  # the I24 test data is full-scale white noise
    got = src.denoised(N, noise, 2.0, 0.1).read_f32()
    _worst(got, v.astype(np.float32) / np.float32(32768.0) if kind == "asynchronous upload" else src.read_f32(), N, 2.0, 0.1, noise, kind)


def test_known_answers(bn):
    """nothing to gate (all-zero noise; alpha 0) gives the source back; silence gives 0.0; white noise far below the threshold comes out
    at floor_gain times the source (floor_gain 0.75 so that EVERY bin is clamped: test_denoise_cpu.py)"""
    N, n = 512, 5000
    v, noise = ref.case(N, n)
    x = v.astype(np.float32) / np.float32(32768.0)
    rec = bn.Recording(v)
    _worst(rec.denoised(N, np.zeros(N // 2 + 1), 2.0, 0.1).read_f32(), x, N, 2.0, 0.1, np.zeros(N // 2 + 1), "all-zero noise", want=x.astype(np.float64))
    _worst(rec.denoised(N, noise, 0.0, 0.1).read_f32(), x, N, 0.0, 0.1, noise, "alpha 0", want=x.astype(np.float64))
    assert (bn.Recording(np.zeros(n, dtype=np.int16)).denoised(N, noise, 2.0, 0.1).read_f32() == 0.0).all()
    w = (np.random.RandomState(3).standard_normal(n) * 0.1).astype(np.float32)
    lvl = 4 * ref.white_level(N, 0.1)
    _worst(bn.Recording(w).denoised(N, lvl, 1.0, 0.75).read_f32(), w, N, 1.0, 0.75, lvl, "every bin clamped", want=0.75 * w.astype(np.float64))


@pytest.mark.parametrize("N", [256, 2048])
def test_an_output_depends_on_its_frames_alone(bn, N):
    H = N // 2
    W = 4 * bn.BN_DENOISE_RUN * H
    v, noise = ref.case(N, 2 * W + H + 3)
    x = v.astype(np.float32) / np.float32(32768.0)
    whole = bn.Recording(x).denoised(N, noise, 2.0, 0.1).read_f32()
    # a shorter recording: every sample further than N from its end; the same samples as int16
    for m in (W + 1, W - 77):
        assert bn.Recording(x[:m]).denoised(N, noise, 2.0, 0.1).read_f32()[:m - N].tobytes() == whole[:m - N].tobytes()
    assert bn.Recording(v).denoised(N, noise, 2.0, 0.1).read_f32().tobytes() == whole.tobytes()
    # a NaN changes no bit further than N samples from it
    at = W + 5
    bad = x.copy()
    bad[at] = np.nan
    got = bn.Recording(bad).denoised(N, noise, 2.0, 0.1).read_f32()
    far = np.abs(np.arange(len(x)) - at) > N
    assert got[far].tobytes() == whole[far].tobytes() and not np.isfinite(got[at])


def test_a_denoised_recording_is_a_recording(bn):
    N, S, step = 256, 1024, 768
    v, noise = ref.case(N, 6000)
    d = bn.Recording(v).denoised(N, noise, 2.0, 0.1)
    y = d.read_f32()
    assert d.levels(S, step).tobytes() == bn.Recording(y).levels(S, step).tobytes()
    with pytest.raises(bn.EngineError):
        d.view_channel(1)
    assert "a filtered recording has no storage-format bytes left" in bn.last_error()
    empty = bn.Recording(np.zeros(0, dtype=np.float32)).denoised(N, noise)
    assert empty.n_samples == 0 and len(empty.read_f32()) == 0
    assert bn.HostRecording(v).denoised(N, noise, 2.0, 0.1).n_samples == 6000  # the host mirror reaches the same entry point


def _bad_noise(v):
    nz = np.ones(129, dtype=np.float32)
    nz[7] = v
    return nz


@pytest.mark.parametrize("kw,word", [
    (dict(src=False), "null recording"), (dict(spec=None), "null denoise spec"), (dict(noise=None), "null noise"), (dict(out=False), "null argument"),
    (dict(spec_size=11), "spec_size"), (dict(spec=(300, 1.0, 0.1)), "frame 300"), (dict(spec=(256, -1.0, 0.1)), "alpha"), (dict(spec=(256, np.inf, 0.1)), "alpha"),
    (dict(spec=(256, np.nan, 0.1)), "alpha"), (dict(spec=(256, 1.0, -0.1)), "floor_gain"), (dict(spec=(256, 1.0, 1.5)), "floor_gain"),
    (dict(spec=(256, 1.0, np.nan)), "floor_gain"), (dict(noise=_bad_noise(-1.0)), "noise[7]"), (dict(noise=_bad_noise(np.inf)), "noise[7]"),
    (dict(noise=_bad_noise(np.nan)), "noise[7]")])
def test_refusals(bn, kw, word):
    rec = bn.Recording(np.ones(100, dtype=np.float32))
    spec, noise, h = kw.get("spec", (256, 1.0, 0.1)), kw.get("noise", np.ones(129, dtype=np.float32)), C.c_void_p(77)
    st = bn.lib.bn_recording_create_denoised(rec._h if kw.get("src", True) else None, None if spec is None else C.byref(bn.BnDenoiseSpec(*spec)), kw.get("spec_size", 12),
                                             None if noise is None else noise.ctypes.data_as(C.POINTER(C.c_float)), C.byref(h) if kw.get("out", True) else None)
    assert st == 1 and word in bn.last_error() and (h.value is None or not kw.get("out", True)), bn.last_error()
