"""bn_fir_bandpass without a GPU, against the float64 restatement of tests/fir_ref.py.

The stop band is asserted on the RESTATEMENT: 80 dB beyond lo - D and hi + D, D = WIDEN * 5.48 * fs / (n_taps - 1) (Kaiser's transition
estimate for beta 8.6, about 87 dB).  WIDEN is 1 where the restatement itself reaches 80 dB at the estimate; it is widened, never the
80, where it does not: a band-pass is the difference of two low-passes, whose ripples add."""
import ctypes as C

import numpy as np
import pytest

import fir_ref as ref

# (sample rate, lo_hz, hi_hz, n_taps, WIDEN)
CASES = [(48000, 150.0, 24000.0, 511, 1.0), (48000, 1000.0, 12000.0, 255, 1.0), (32000, 0.0, 8000.0, 63, 1.0), (48000, 1000.0, 12000.0, 1, None)]


@pytest.mark.parametrize("rate,lo,hi,n_taps,widen", CASES)
def test_designer_agrees_with_the_restatement(bn, rate, lo, hi, n_taps, widen):
    got, want = bn.fir_bandpass(rate, lo, hi, n_taps), ref.bandpass(rate, lo, hi, n_taps)
    assert got.dtype == np.float32 and got.shape == (n_taps,)
    if n_taps == 1:
        assert got.tolist() == [1.0]
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print("worst |tap - restatement| in ulps", float(np.max(np.abs(got - want) / ulp)))
    assert (np.abs(got - want) <= ulp).all()
    assert got.tobytes() == got[::-1].tobytes()  # symmetric bit for bit
    # the centre gain was 1 before each tap was rounded by at most 2^-24 of itself
    p_lo, p_hi = ref.band(rate, lo, hi)
    gain = ref.response(got, 0.5 * (p_lo + p_hi) / rate)
    assert abs(gain - 1.0) <= n_taps * 2.0 ** -24 * float(np.abs(got).max())
    if widen is None:
        return
    D = widen * 5.48 * rate / (n_taps - 1)
    f = np.arange(0.0, rate / 2.0 + 1.0, rate / 2.0 / 4096)
    stop = f[(f <= p_lo - D) | (f >= p_hi + D)]
    if len(stop) == 0:  # the 150 Hz high-pass at 511 taps: D = 516 Hz, the whole stop side lies inside the transition
        assert p_lo - D < 0.0 and p_hi == rate / 2.0
        return
    worst = max(abs(ref.response(want, x / rate)) for x in stop)
    print("stop band of the restatement", 20 * np.log10(worst), "dB at D =", D, "Hz")
    assert 20 * np.log10(worst) <= -80.0


def test_designer_refusals(bn):
    taps = (C.c_float * 4)(7, 7, 7, 7)
    for args, word in (((0, 100.0, 1000.0, 3), "sample_rate"), ((48000, 1000.0, 1000.0, 3), "lo_hz must be below hi_hz"),
                       ((48000, 2000.0, 1000.0, 3), "lo_hz must be below hi_hz"), ((48000, float("nan"), 1000.0, 3), "lo_hz must be below hi_hz"),
                       ((48000, 24000.0, 30000.0, 3), "half the sample rate"), ((48000, -5.0, 0.0, 3), "hi_hz must be positive"),
                       ((48000, 100.0, 1000.0, 4), "n_taps 4"), ((48000, 100.0, 1000.0, 0), "n_taps 0"),
                       ((48000, 100.0, 1000.0, bn.BN_FIR_MAX_TAPS + 2), "n_taps 2049")):
        assert bn.lib.bn_fir_bandpass(*args, taps) == 1 and word in bn.last_error(), (args, bn.last_error())
        assert list(taps) == [7, 7, 7, 7]  # a refusal writes nothing
        with pytest.raises(bn.EngineError):
            bn.fir_bandpass(*args)
    assert bn.lib.bn_fir_bandpass(48000, 100.0, 1000.0, 3, None) == 1 and "null" in bn.last_error()
