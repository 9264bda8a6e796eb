"""bn_recording_create_filtered on the GPU: exact cases that pin indexing, halo, padding and centring bit for bit, random cases
against float64 (tests/fir_ref.py), the result as an ordinary recording, and the refusals.

The error of an output is counted in units of 2^-24 * D_n, D_n = sum_t |taps[t]| |x[n + c - t]| (the convention of
tests/test_gpu_b3_precision.py).  Its rms over a case's outputs must stay within 4 x the rms of a float32 direct-form chain of the
same case against the same float64 reference (the project's bf16x3 kernels measured 0.9 - 2.4 x their exact-f32 siblings; a kernel
that drops one small partial product sits 10 - 50 x above), its worst below 8 + K / 32 units (the dropped products' 2^-21, one rounding
per 32-deep step).  A case with fewer than 64 outputs is drawn again until 64 outputs are pooled: the rms of one output is no
statistic.  C = BN_FIR_CHUNK is the kernel's chunk; the lengths sit around it."""
import ctypes as C

import numpy as np
import pytest

import fir_ref as ref
import pcm_ref

pytestmark = pytest.mark.gpu


def _impulse(n_taps):
    t = np.zeros(n_taps, dtype=np.float32)
    t[(n_taps - 1) // 2] = 1.0
    return t


@pytest.mark.parametrize("n_taps", [1, 33])
def test_unit_impulse_taps_copy_the_source(bn, n_taps):
    rng, n = np.random.default_rng(n_taps), bn.BN_FIR_CHUNK + 37
    mono = bn.Recording(rng.uniform(-1, 1, n).astype(np.float32))
    stereo = bn.Recording.from_layout(pcm_ref.test_data(np.random.RandomState(n_taps), pcm_ref.I24, n, 2), bn.BN_PCM_I24, 2, bn.BN_PCM_MIX)
    for src in (mono, stereo):
        got = src.filtered(_impulse(n_taps))
        assert got.n_samples == n and np.array_equal(got.read_f32(), src.read_f32())


@pytest.mark.parametrize("at", range(6))
def test_unit_impulse_source_places_the_taps(bn, at):
    Ck = bn.BN_FIR_CHUNK
    n, n_taps = 2 * Ck + 40, 49
    pos = (0, 15, 16, Ck - 1, Ck, n - 1)[at]
    taps = np.random.default_rng(pos).uniform(-1, 1, n_taps).astype(np.float32)
    x = np.zeros(n, dtype=np.float32)
    x[pos] = 1.0
    want = ref.filt(x, taps).astype(np.float32)  # the taps around pos, cut at the ends: every product is with 1.0
    assert np.count_nonzero(want) == min(pos, 24) + 1 + min(n - 1 - pos, 24)
    assert np.array_equal(bn.Recording(x).filtered(taps).read_f32(), want)


def _units(y, x, taps):
    """|y - float64| per output in units of 2^-24 D_n"""
    d = ref.filt(np.abs(x), np.abs(taps)) * 2.0 ** -24
    return np.abs(y.astype(np.float64) - ref.filt(x, taps)) / np.where(d > 0, d, 1.0)


def _chain_f32(x, taps):
    """the direct form in float32: acc = acc + taps[t] * x[n + c - t], t ascending, every operation rounded"""
    c, n = (len(taps) - 1) // 2, len(x)
    xp = np.concatenate([np.zeros(c, np.float32), x, np.zeros(c, np.float32)])
    acc = np.zeros(n, dtype=np.float32)
    for t in range(len(taps)):
        acc = acc + taps[t] * xp[2 * c - t:2 * c - t + n]
    return acc


# (n_taps, n = a + b * C + d * n_taps): n in {1, 17, C - 1, C + 1, 2 C + n_taps}
@pytest.mark.parametrize("n_taps,a,b,d", [(3, 1, 0, 0), (17, 17, 0, 0), (19, -1, 1, 0), (49, 1, 1, 0), (51, 0, 2, 1), (2047, 0, 2, 1)])
def test_random_against_float64(bn, n_taps, a, b, d):
    n = a + b * bn.BN_FIR_CHUNK + d * n_taps
    rng = np.random.default_rng(n_taps)
    got, chain = [], []
    for _ in range(-(-64 // n)):
        x, taps = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n_taps).astype(np.float32)
        got.append(_units(bn.Recording(x).filtered(taps).read_f32(), x, taps))
        chain.append(_units(_chain_f32(x, taps), x, taps))
    got, chain = np.concatenate(got), np.concatenate(chain)
    rms, rms32, K = np.sqrt(np.mean(got ** 2)), np.sqrt(np.mean(chain ** 2)), (n_taps + 15 + 31) // 32 * 32
    print(f"n_taps {n_taps} n {n}: rms {rms:.3f} worst {got.max():.3f} units; float32 chain rms {rms32:.3f} worst {chain.max():.3f}")
    assert rms <= 4 * rms32
    assert got.max() < 8 + K / 32


def test_a_filtered_recording_is_a_recording(bn):
    S, step, rng = 1024, 768, np.random.default_rng(5)
    taps = rng.uniform(-1, 1, 33).astype(np.float32)
    v = rng.integers(-32768, 32768, 6000).astype(np.int16)
    for make in (lambda: bn.Recording(v.astype(np.float32) / np.float32(32768.0)), lambda: bn.Recording(v, src_rate=48000, dst_rate=32000)):
        src = make()
        f = src.filtered(taps)
        want = src.read_f32()
        del src  # the source goes first
        y = f.read_f32()
        assert len(y) == len(want) and np.abs(_units(y, want, taps)).max() < 8 + 2
        assert f.windows(S, step, 0, f.n_windows(step)).tobytes() == pcm_ref.chunk_audio(y, S, step).tobytes()
        assert f.view_channel(bn.BN_PCM_MIX).read_f32().tobytes() == y.tobytes()
        with pytest.raises(bn.EngineError):
            f.view_channel(1)
        assert "a filtered recording has no storage-format bytes left" in bn.last_error()


def test_refusals_and_the_empty_source(bn):
    src = bn.Recording(np.ones(100, dtype=np.float32))
    fp = C.POINTER(C.c_float)
    taps = np.ones(bn.BN_FIR_MAX_TAPS + 2, dtype=np.float32)
    h = C.c_void_p(77)
    for n_taps, word in ((2, "n_taps 2 "), (0, "n_taps 0 "), (bn.BN_FIR_MAX_TAPS + 2, "n_taps 2049 ")):
        assert bn.lib.bn_recording_create_filtered(src._h, taps.ctypes.data_as(fp), n_taps, C.byref(h)) == 1 and word in bn.last_error()
        assert h.value is None  # no handle
    bad = np.ones(5, dtype=np.float32)
    bad[3] = np.nan
    assert bn.lib.bn_recording_create_filtered(src._h, bad.ctypes.data_as(fp), 5, C.byref(h)) == 1 and "tap 3 is not finite" in bn.last_error()
    assert bn.lib.bn_recording_create_filtered(None, taps.ctypes.data_as(fp), 3, C.byref(h)) == 1 and "null recording" in bn.last_error()
    assert bn.lib.bn_recording_create_filtered(src._h, None, 3, C.byref(h)) == 1 and "null taps" in bn.last_error()
    assert bn.lib.bn_recording_create_filtered(src._h, taps.ctypes.data_as(fp), 3, None) == 1 and "null argument" in bn.last_error()
    empty = bn.Recording(np.zeros(0, dtype=np.float32)).filtered(taps[:3])
    assert empty.n_samples == 0 and len(empty.read_f32()) == 0
    host = bn.HostRecording(np.arange(100, dtype=np.int16)).filtered(_impulse(5))  # the host mirror reaches the same entry point
    assert host.n_samples == 100
    with pytest.raises(bn.Error):
        bn.HostRecording(np.arange(100, dtype=np.int16)).filtered(taps[:4])
