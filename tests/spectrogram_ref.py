"""bn_recording_spectrogram restated in float64 numpy (include/birdnet_hip.h, "Spectrograms"): frame t covers samples
[first + t * hop, first + t * hop + N) of the f32 samples, zeros past the end; the one-sided power P[t, k] is band_levels_ref's; rows
are the bins [lo, hi) or E = P W^T for a bank W; a frame that reads a non-finite sample is +Inf in every row.

bounds() is the header's promise as a function of the header's constants; mel_bank() and thresholds() restate the two host-only
designers.  `wrong` names one of four wrong rules, for test_spectrogram_cpu.py's proof that the bounds are not vacuous.  Shared
with test_gpu_spectrogram.py."""
import os
import re

import numpy as np

import band_levels_ref as band

FRAMES, ROOT = band.FRAMES, band.ROOT
WRONG = ("symmetric Hann window", "c_k missing", "bank applied to amplitudes", "bank row shifted by one bin")
U = 2.0 ** -24


def header_constants() -> dict:
    """BN_SPECTROGRAM_*, BN_FILTERBANK_* and BN_BAND_* as include/birdnet_hip.h declares them"""
    text = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (BN_(?:SPECTROGRAM|FILTERBANK|BAND)_\w+) (\d+)\b", text, flags=re.M)}


def noise(N, n_frames, hop, seed=0):
    """the GPU tests' input: white int16 noise that ends N // 3 samples short of the last frame's end"""
    n = (n_frames - 1) * hop + N - (N // 3 if n_frames > 1 else 0)
    return np.clip(np.round(6000 * np.random.RandomState(7 + N + n_frames + hop + seed).standard_normal(n)), -32768, 32767).astype(np.int16)


def random_bank(N, rows, seed=3):
    """a dense non-negative bank: every K step of every row tile is live"""
    return np.random.RandomState(seed + rows).uniform(0.0, 1.0, (rows, N // 2 + 1)).astype(np.float32)


def selection_bank(N):
    """row m selects bin 3 m + 1, the last row bin N/2: one weight of 1.0 per row"""
    cols = list(range(1, N // 2, 3)) + [N // 2]
    W = np.zeros((len(cols), N // 2 + 1), dtype=np.float32)
    W[np.arange(len(cols)), cols] = 1.0
    return W, cols


def powers(x, first, n_frames, N, hop, wrong=None):
    """(P [n_frames, N/2 + 1] float64, bad [n_frames]) of the f32 samples x; a bad frame's P is +Inf"""
    x = np.asarray(x, dtype=np.float32)
    pad = np.zeros(first + (n_frames - 1) * hop + N if n_frames else 0, dtype=np.float32)
    pad[:min(len(x), len(pad))] = x[:len(pad)]
    w = pad[first:]
    idx = np.arange(n_frames)[:, None] * hop + np.arange(N)[None, :]
    bad = ~np.isfinite(w[idx]).all(axis=1) if n_frames else np.zeros(0, dtype=bool)
    w = np.where(np.isfinite(w), w, 0.0)
    perturb = {"window": np.hanning(N)} if wrong == WRONG[0] else {"one_sided": 1.0} if wrong == WRONG[1] else {}
    P = band.frame_powers(w, N, hop, frames=n_frames, **perturb) if n_frames else np.zeros((0, N // 2 + 1))
    P[bad] = np.inf
    return P, bad


def image(x, first, n_frames, N, hop, bins=None, bank=None, wrong=None):
    """the float64 image [n_frames, n_rows] and the bound on every element of it"""
    c = header_constants()
    P, bad = powers(x, first, n_frames, N, hop, wrong)
    Pf = np.where(bad[:, None], 0.0, P)
    T, eps = Pf.sum(axis=1, keepdims=True), c["BN_BAND_EPS_ULPS"] * U
    b = 2.0 * eps * np.sqrt(Pf * T) + eps * eps * T + c["BN_SPECTROGRAM_POW_DEPTH"] * U * Pf
    if bank is None:
        img, bound = Pf[:, bins[0]:bins[1]], b[:, bins[0]:bins[1]]
    else:
        W = np.asarray(bank, dtype=np.float64)
        if wrong == WRONG[3]:
            W = np.roll(W, 1, axis=1)
        img = (np.sqrt(Pf) @ W.T) ** 2 if wrong == WRONG[2] else Pf @ W.T
        bound = b @ W.T + (2.0 ** -21 + c["BN_SPECTROGRAM_BANK_DEPTH"] * U) * img
    return np.where(bad[:, None], np.inf, img), np.where(bad[:, None], 0.0, bound)


def worst_share(got, want, bound) -> float:
    """max |got - want| / bound; an element whose bound is 0 (silence, +Inf) must match exactly"""
    g, fin = np.asarray(got, dtype=np.float64), np.isfinite(want)
    if g.shape != want.shape or not (g[~fin] == want[~fin]).all() or not np.isfinite(g[fin]).all():
        return np.inf
    err, bf = np.abs(g[fin] - want[fin]), bound[fin]
    share = np.where(bf > 0, err / np.where(bf > 0, bf, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(share.max()) if share.size else 0.0


def mel_bank(rate, N, n_mels, fmin, fmax):
    """bn_mel_filterbank: HTK triangles with peak 1 at the bin centres, float64"""
    mel, hz = (lambda f: 2595.0 * np.log10(1.0 + f / 700.0)), (lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0))
    pt = hz(mel(fmin) + (mel(fmax) - mel(fmin)) * np.arange(n_mels + 2) / (n_mels + 1))
    f = np.arange(N // 2 + 1) * rate / N
    a, b, c = pt[:-2, None], pt[1:-1, None], pt[2:, None]
    return np.where((f <= a) | (f >= c), 0.0, np.where(f <= b, (f - a) / (b - a), (c - f) / (c - b)))


def thresholds(ref_power, range_db):
    """bn_spectrogram_thresholds: 255 float32, non-decreasing"""
    j = np.arange(1, 256, dtype=np.float64)
    ref_power, range_db = float(np.float32(ref_power)), float(np.float32(range_db))
    return np.maximum.accumulate((ref_power * 10.0 ** (((j - 0.5) * range_db / 255.0 - range_db) / 10.0)).astype(np.float32))


def codes(thr, img):
    """the U8 image of a float32 image: per pixel the number of thresholds that are <= it"""
    return np.searchsorted(thr, img, side="right").astype(np.uint8)
