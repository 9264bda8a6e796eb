"""bn_recording_create_denoised restated in float64 numpy (include/birdnet_hip.h, "Noise reduction"): frames of N samples at hop
H = N / 2, frame t over source positions [(t - 1) H, (t + 1) H), the window sin(pi j / N) before numpy.fft.rfft and after irfft, the
memoryless gain max(floor_gain, 1 - alpha noise[k] / P), overlap-add.  `wrong` names one of five wrong rules, for
test_denoise_cpu.py's proof that the bound is not vacuous.  Shared with test_gpu_denoise.py."""
import os
import re

import numpy as np

FRAMES = (256, 512, 1024, 2048)
WRONG = ("no synthesis window", "gain from the neighbouring bin", "floor_gain ignored", "frames shifted by one sample", "last frame dropped")
U = 2.0 ** -24
SIGMA, TONE = 3000, 8000  # case(): the noise's standard deviation and the tone's amplitude, in int16 steps


def header_constants() -> dict:
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "birdnet_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (BN_(?:DENOISE|BAND)_\w+) (\d+)\b", text, flags=re.M)}


def white_level(N, sigma):
    """E P[t, k] of white noise of standard deviation sigma: c_k sigma^2 / N"""
    c = np.full(N // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    return (c * sigma * sigma / N).astype(np.float32)


def case(N, n):
    """the bound test's input: n int16 samples of white noise plus an off-centre tone well above it, and the true noise level per bin"""
    rng = np.random.RandomState(N + n % 1000)
    tone = TONE * np.sin(2 * np.pi * np.arange(n) * (N // 8 + 0.37) / N)
    return np.clip(np.round(SIGMA * rng.standard_normal(n) + tone), -32768, 32767).astype(np.int16), white_level(N, SIGMA / 32768.0)


def denoise(x, N, alpha, floor_gain, noise, wrong=None):
    """(y [n], E [B + 2]) in float64: the rule on the f32 samples x, and E[t] = ||w x_t||_2 per frame t = 0 .. B (E[B + 1] unused, 0)"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, H = len(x), N // 2
    B = -(-n // H)
    shift = 1 if wrong == WRONG[3] else 0
    w = np.sin(np.pi * np.arange(N) / N)
    xp = np.zeros((B + 2) * H + 1)  # xp[H + i] = x[i]: frame t starts at xp[t H]
    xp[H:H + n] = x
    fr = xp[np.arange(B + 1)[:, None] * H + np.arange(N)[None, :] + shift] * w
    X = np.fft.rfft(fr, axis=1)
    c = np.full(H + 1, 2.0)
    c[0] = c[-1] = 1.0
    P = c * (X.real ** 2 + X.imag ** 2) / (N * (w ** 2).sum())
    a = float(np.float32(alpha)) * np.asarray(noise, dtype=np.float32).astype(np.float64)
    a = np.roll(a, 1) if wrong == WRONG[1] else a
    fl = 0.0 if wrong == WRONG[2] else float(np.float32(floor_gain))
    g = np.where(a == 0, 1.0, np.where(P == 0, fl, np.maximum(fl, 1.0 - a / np.where(P == 0, 1.0, P))))
    y = np.fft.irfft(g * X, n=N, axis=1) * (1.0 if wrong == WRONG[0] else w)
    if wrong == WRONG[4]:
        y[B] = 0.0
    out = np.zeros_like(xp)
    for t in range(B + 1):
        out[t * H + shift:t * H + shift + N] += y[t]
    return out[H:H + n], np.append(np.sqrt((fr ** 2).sum(axis=1)), 0.0)


def shares(got, ref, E, N, consts=None):
    """per output block b, ||got - ref||_2 / ((K eps + G u) (E[b] + E[b + 1])); a block whose bound is 0 must match exactly (0, else
    inf), a non-finite output is inf.  Every block is within the header's bound iff every share is <= 1"""
    c = header_constants() if consts is None else consts
    H, n = N // 2, len(ref)
    B = -(-n // H)
    d = np.zeros(B * H)
    d[:n] = np.asarray(got, dtype=np.float64) - ref
    with np.errstate(invalid="ignore"):
        err = np.sqrt((d.reshape(B, H) ** 2).sum(axis=1))
    b = (c["BN_DENOISE_K"] * c["BN_BAND_EPS_ULPS"] + c["BN_DENOISE_GAIN_ULPS"]) * U * (E[:B] + E[1:B + 1])
    return np.where(~np.isfinite(err), np.inf, np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf)))
