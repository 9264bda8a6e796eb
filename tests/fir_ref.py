"""Float64 restatements of the FIR rule of include/birdnet_hip.h ("FIR filtering"): the windowed-sinc designer and the centred,
zero-extended filter.  numpy only; nothing here touches the library."""
import numpy as np

BETA = 8.6


def band(rate, lo_hz, hi_hz):
    """the pass band in hertz, clipped to [0, rate / 2]"""
    return max(lo_hz, 0.0), min(hi_hz, rate / 2.0)


def bandpass(rate, lo_hz, hi_hz, n_taps) -> np.ndarray:
    lo, hi = band(rate, lo_hz, hi_hz)
    f1, f2 = lo / rate, (hi / rate if hi_hz < rate / 2.0 else 0.5)
    half = (n_taps - 1) / 2.0
    tau = np.arange(n_taps, dtype=np.float64) - half
    u = tau / half if half else np.zeros(1)
    w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - u * u))) / np.i0(BETA)
    h = (2 * f2 * np.sinc(2 * f2 * tau) - 2 * f1 * np.sinc(2 * f1 * tau)) * w
    return h / response(h, 0.5 * (lo + hi) / rate)


def response(h, f) -> float:
    """the (real) response of symmetric taps at f cycles per sample"""
    tau = np.arange(len(h), dtype=np.float64) - (len(h) - 1) / 2.0
    return float(np.sum(np.asarray(h, dtype=np.float64) * np.cos(2 * np.pi * f * tau)))


def filt(x, taps) -> np.ndarray:
    """y[n] = sum_t taps[t] x[n + c - t], c = (len(taps) - 1) / 2, x zero outside; float64 over the given values"""
    c = (len(taps) - 1) // 2
    return np.convolve(np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64))[c:c + len(x)]
