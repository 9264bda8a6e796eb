"""bn_recording_band_levels restated in float64 numpy (include/birdnet_hip.h, "bn_recording_band_levels"): a window's S samples are
levels_ref.window's -- the layout rule's f32 samples (tests/pcm_ref.py), zeros past the end -- cut into frames of N samples every
`hop`, frame j at window positions [j hop, j hop + N), n_frames = (S - N) // hop + 1, the tail no full frame covers unread.  A frame is
multiplied by the periodic Hann window in double, transformed with numpy.fft.rfft, and

    P_k = c_k |X_k|^2 / (N sum w^2),  c_k = 1 for k = 0 and k = N/2, 2 otherwise

summed over a band's bins [lo, hi) and over all bins (the total); a window reports the mean and the maximum over its frames.

bound() is the header's promise as a function of the header's constants, which header_constants() parses from the header.  Shared
by test_band_levels_cpu.py (this file against hand-computed cases, and the bound against perturbed references) and
test_gpu_band_levels.py."""
import os
import re

import numpy as np

import levels_ref

NONFINITE, PADDED = levels_ref.NONFINITE, levels_ref.PADDED
FRAMES = (256, 512, 1024, 2048)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants() -> dict:
    """BN_BAND_MAX, BN_BAND_EPS_ULPS and BN_BAND_SUM_DEPTH as include/birdnet_hip.h declares them"""
    text = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (BN_BAND_\w+) (\d+)\b", text, flags=re.M)}


def n_frames(S, N, hop) -> int:
    return (S - N) // hop + 1


def unread(S, N, hop) -> int:
    """trailing window positions that no full frame covers"""
    return S - ((n_frames(S, N, hop) - 1) * hop + N)


def hann(N) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def frame_powers(w, N, hop, window=None, one_sided=2.0, frames=None) -> np.ndarray:
    """P [n_frames, N/2 + 1] of one window's samples w (float64).  window / one_sided / frames exist for the perturbed references of
    test_band_levels_cpu.py: another window function, another factor for the inner bins, fewer frames"""
    w = np.asarray(w, dtype=np.float64)
    S = len(w)
    nf = n_frames(S, N, hop) if frames is None else frames
    win = hann(N) if window is None else np.asarray(window, dtype=np.float64)
    idx = np.arange(nf)[:, None] * hop + np.arange(N)[None, :]
    X = np.fft.rfft(w[idx] * win[None, :], axis=1)
    c = np.full(N // 2 + 1, float(one_sided))
    c[0] = c[-1] = 1.0
    return c[None, :] * (X.real ** 2 + X.imag ** 2) / (N * (win ** 2).sum())


def window_bands(w, padded, N, hop, bands, **perturb):
    """(mean [n_bands], max [n_bands], total_mean, total_max, flags, n_frames) of one window's f32 samples"""
    w = np.asarray(w, dtype=np.float32)
    nf = n_frames(len(w), N, hop)
    flags = PADDED if padded else 0
    read = (nf - 1) * hop + N
    if not np.isfinite(w[:read]).all():
        inf = np.full(len(bands), np.inf)
        return inf, inf.copy(), np.inf, np.inf, flags | NONFINITE, nf
    P = frame_powers(w.astype(np.float64), N, hop, **perturb)
    per = np.stack([P[:, lo:hi].sum(axis=1) for lo, hi in bands], axis=1)
    tot = P.sum(axis=1)
    return per.mean(axis=0), per.max(axis=0), float(tot.mean()), float(tot.max()), flags, nf


def band_levels(x, S, step, N, hop, bands, first=0, count=None, **perturb):
    """windows [first, first + count) of chunk_audio(x, S, step) as a dict of arrays: mean, max [count, n_bands] and total_mean,
    total_max [count] (float64), flags, n_frames (uint32)"""
    x = np.asarray(x, dtype=np.float32)
    total = (len(x) + step - 1) // step if len(x) else 0
    count = total - first if count is None else count
    assert 0 <= first and first + count <= total
    rows = [window_bands(levels_ref.window(x, S, k * step), k * step + S > len(x), N, hop, bands, **perturb) for k in range(first, first + count)]
    return {"mean": np.array([r[0] for r in rows], dtype=np.float64).reshape(count, len(bands)),
            "max": np.array([r[1] for r in rows], dtype=np.float64).reshape(count, len(bands)),
            "total_mean": np.array([r[2] for r in rows], dtype=np.float64), "total_max": np.array([r[3] for r in rows], dtype=np.float64),
            "flags": np.array([r[4] for r in rows], dtype=np.uint32), "n_frames": np.array([r[5] for r in rows], dtype=np.uint32)}


def bound(P, T, nf, consts=None):
    """the header's bound on |got - P| for a field whose reference value is P, T the reference total of the same kind (total_mean for
    a mean, total_max for a max), nf the window's frames: 2 eps sqrt(P T) + eps^2 T + delta P"""
    c = header_constants() if consts is None else consts
    u = 2.0 ** -24
    eps = c["BN_BAND_EPS_ULPS"] * u
    delta = (c["BN_BAND_SUM_DEPTH"] + -(-np.asarray(nf, dtype=np.float64) // 4)) * u
    P, T = np.asarray(P, dtype=np.float64), np.asarray(T, dtype=np.float64)
    return 2.0 * eps * np.sqrt(P * T) + eps * eps * T + delta * P


def bounds(ref, consts=None) -> dict:
    """bound() for every float field of a band_levels() result"""
    nf = ref["n_frames"].astype(np.float64)
    return {"mean": bound(ref["mean"], ref["total_mean"][:, None], nf[:, None], consts),
            "max": bound(ref["max"], ref["total_max"][:, None], nf[:, None], consts),
            "total_mean": bound(ref["total_mean"], ref["total_mean"], nf, consts),
            "total_max": bound(ref["total_max"], ref["total_max"], nf, consts)}


def worst_share(got, ref, consts=None) -> float:
    """max over the float fields of |got - ref| / bound; fields whose bound is 0 must match exactly (then 0, else inf)"""
    worst = 0.0
    for k, b in bounds(ref, consts).items():
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            share = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
        worst = max(worst, float(share.max()) if share.size else 0.0)
    return worst


def bins(rate, N, lo_hz, hi_hz):
    """bn_band_bins: the bins k in 0 .. N/2 whose centre k rate / N lies in [lo_hz, hi_hz), as (first, one past the last)"""
    ks = [k for k in range(N // 2 + 1) if lo_hz * N <= k * rate < hi_hz * N]
    return (ks[0], ks[-1] + 1) if ks else None


def random_case(N, hop, S=8192, windows=5):
    """the inputs of the GPU random-audio test, shared with the CPU test that shows the bound is not vacuous: int16 audio whose spectrum
    falls towards high frequencies plus one off-centre tone (so that bands differ), exactly `windows` windows of S at step S // 3 (the
    last ones reach past the end), three bands of which two overlap"""
    step = S // 3
    rng = np.random.RandomState(7 + N + hop)
    n = windows * step
    white = rng.standard_normal(n + 8)
    coloured = np.convolve(white, [0.4, 0.3, 0.15, 0.08, 0.04, 0.02, 0.007, 0.003], mode="valid")[:n]
    t = np.arange(n)
    v = np.clip(np.round(6000 * coloured + 3000 * np.sin(2 * np.pi * t * (N // 8 + 0.37) / N)), -32768, 32767).astype(np.int16)
    half = N // 2
    bands = [(1, half // 8), (half // 8, half // 2 + 3), (half // 2 - 5, half + 1)]
    return v, S, step, bands
