"""The float64 restatement of the delay estimate (tests/delay_ref.py) and bn_delay_refine, without a GPU: the PLAIN curve against a
time-domain circular correlation, the margin that lets test_gpu_delay.py assert peak_lag == d in every one of its cases, and the
host-only parabola through the library."""
import ctypes as C

import numpy as np
import pytest

import band_levels_ref as band
import delay_ref as ref


def test_plain_curve_is_the_circular_correlation_of_the_windowed_frames():
    N, F, max_lag = 256, 5, 32
    a, b, S, hop = ref.pair(N, F, 3, windows=1)
    r = ref.delay(ref.f32(a), ref.f32(b), S, S, N, hop, (0, N // 2 + 1), max_lag, ref.PLAIN)
    x, y, w = a.astype(np.float64) / 32768, b.astype(np.float64) / 32768, band.hann(N)
    brute = np.zeros(2 * max_lag + 1)
    for t in range(F):
        fa, fb = x[t * hop:t * hop + N] * w, y[t * hop:t * hop + N] * w
        brute += [np.dot(fa, np.roll(fb, tau)) for tau in range(-max_lag, max_lag + 1)]  # sum_n fa[n] fb[(n - tau) mod N]
    brute *= N / (F * N * (w ** 2).sum())
    assert np.abs(r["curve"][0] - brute).max() <= 1e-12 * np.abs(brute).max() and r["peak_lag"][0] == 3


@pytest.mark.parametrize("N", ref.FRAMES)
def test_every_gpu_case_has_its_peak_at_d_by_more_than_twice_the_bound(N):
    for F in ref.FRAME_COUNTS:
        for d in ref.delays(N):
            a, b, S, hop = ref.pair(N, F, d)
            for weighting in (ref.PLAIN, ref.PHAT):
                r = ref.delay(ref.f32(a), ref.f32(b), S, S, N, hop, ref.bands(N)[0], N // 8, weighting)
                assert r["peak_lag"].tolist() == [d, d] and (r["margin"] > 2 * r["bound"]).all(), (N, F, d, weighting, r["margin"], r["bound"])


def test_delay_refine_through_the_library(bn):
    def refine(lag, peak, before, after, flags=0, struct_size=None, out=True):
        w, got = bn.BnWindowDelay(lag, peak, before, after, flags, 4), C.c_double(99.0)
        st = bn.lib.bn_delay_refine(C.byref(w), C.sizeof(w) if struct_size is None else struct_size, C.byref(got) if out else None)
        return st, got.value

    # the parabola 1 - (t - 0.2)^2 sampled at t = -1, 0, 1 around lag 5: its vertex (the fields are f32)
    assert abs(refine(5, 1 - 0.04, 1 - 1.44, 1 - 0.64)[1] - 5.2) < 1e-6
    assert refine(-3, 1.0, 1.0, 1.0) == (0, -3.0)  # no curvature: the denominator is 0
    assert refine(2, 1.0, 0.0, 1.5) == (0, 2.5) and refine(2, 1.0, 1.5, 0.0) == (0, 1.5)  # clamped to half a sample
    assert refine(0, np.nan, np.nan, np.nan, flags=bn.BN_LEVEL_NONFINITE) == (0, 0.0)
    rec = np.zeros(1, dtype=bn.DELAY_DTYPE)
    rec[0] = (7, 2.0, 1.0, 1.5, 0, 4)
    assert bn.delay_refine(rec[0]) == 7 + 0.5 * (1.0 - 1.5) / (1.0 - 4.0 + 1.5)
    for kw, word in ((dict(struct_size=23), "struct_size"), (dict(out=False), "null")):
        st, got = refine(1, 1.0, 0.5, 0.5, **kw)
        assert st == 1 and word in bn.last_error() and got == 99.0
    assert bn.lib.bn_delay_refine(None, 24, C.byref(C.c_double())) == 1 and "null" in bn.last_error()
