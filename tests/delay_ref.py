"""bn_recording_delay restated in float64 numpy (include/birdnet_hip.h, "bn_recording_delay"): windows and frames are
band_levels_ref's, cut from both recordings at the same start; G = sum_t A_t conj(B_t); Psi is G inside the band (PLAIN) or its unit
phasor (PHAT) and 0 outside; r = irfft(Psi) * N / Z read at tau mod N; the peak by the tie rule.  delay() also returns the header's
bound per window, from the header's constants, and the margin by which the rule's peak leads every lag further than one sample away.
Shared by test_gpu_delay.py and test_delay_cpu.py; not derived from the kernel."""
import os
import re

import numpy as np

import band_levels_ref as band
import levels_ref

NONFINITE, PADDED, FRAMES = band.NONFINITE, band.PADDED, band.FRAMES
PLAIN, PHAT = 0, 1
U = 2.0 ** -24
FRAME_COUNTS = (1, 4, 5, 9)  # a single frame, one frame per wave, uneven runs, runs of three


def header_constants() -> dict:
    """BN_DELAY_* and BN_BAND_* as include/birdnet_hip.h declares them"""
    text = open(os.path.join(band.ROOT, "include", "birdnet_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (BN_(?:DELAY|BAND)_\w+) (\d+)\b", text, flags=re.M)}


def delays(N):
    """the GPU test's delays; max_lag = N / 8"""
    return 0, 3, -7, N // 8, -(N // 8)


def bands(N):
    """the GPU test's bands: all bins (both edge bins, c_k = 1), an interior band of N/8 bins, one bin"""
    return (0, N // 2 + 1), (N // 8, N // 4), (N // 4 + 3, N // 4 + 4)


def pair(N, F, d, hop=None, windows=2):
    """(a, b, S, hop): int16 white noise x with b[n] = x[n] and a[n] = x[n - d] cut from one long sequence (a linear delay, not a
    circular one), independent noise 30 dB down added to each; `windows` windows of S = N + (F - 1) hop samples"""
    hop = N // 2 if hop is None else hop
    S = N + (F - 1) * hop
    n, off = windows * S, N // 8
    rng = np.random.RandomState(1000 * F + N + (d % 97))
    x = rng.standard_normal(n + 2 * off)
    own = 10.0 ** -1.5 * rng.standard_normal((2, n))
    a, b = x[off - d:off - d + n] + own[0], x[off:off + n] + own[1]
    return tuple(np.clip(np.round(6000 * v), -32768, 32767).astype(np.int16) for v in (a, b)) + (S, hop)


def f32(v):
    """the f32 samples the library reads from int16 (exact)"""
    return np.asarray(v).astype(np.float32) / np.float32(32768.0)


def frames(w, N, hop, nf):
    """X [nf, N/2 + 1] of one window's samples"""
    idx = np.arange(nf)[:, None] * hop + np.arange(N)[None, :]
    return np.fft.rfft(np.asarray(w, dtype=np.float64)[idx] * band.hann(N)[None, :], axis=1)


def pick(r, max_lag):
    """the peak of r (indexed by tau mod N) over -max_lag .. max_lag by the tie rule, and its margin over the lags further than one away"""
    taus = np.arange(-max_lag, max_lag + 1)
    v = r[taus]
    best = min(range(len(taus)), key=lambda i: (-v[i], abs(taus[i]), taus[i]))
    far = np.abs(taus - taus[best]) > 1
    return int(taus[best]), float(v[best] - v[far].max()) if far.any() else np.inf


def delay(a, b, S, step, N, hop, bins, max_lag, weighting, first=0, count=None, consts=None):
    """windows [first, first + count) of a against b: curve [count, 2 max_lag + 1], peak, before, after, bound, margin float64 [count];
    peak_lag int32, flags, n_frames uint32"""
    c = header_constants() if consts is None else consts
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    n = min(len(a), len(b))
    total = (n + step - 1) // step if n else 0
    count = total - first if count is None else count
    nf, lo, hi = band.n_frames(S, N, hop), bins[0], bins[1]
    ck = np.full(N // 2 + 1, 2.0)
    ck[0] = ck[-1] = 1.0
    inside = np.zeros(N // 2 + 1, dtype=bool)
    inside[lo:hi] = True
    eps, q = c["BN_BAND_EPS_ULPS"] * U, -(-nf // 4)
    Z = ck[inside].sum() if weighting == PHAT else nf * N * (band.hann(N) ** 2).sum()
    taus = np.arange(-max_lag, max_lag + 1)
    out = {k: np.zeros(count) for k in ("peak", "before", "after", "bound", "margin")}
    out.update(curve=np.zeros((count, len(taus))), peak_lag=np.zeros(count, dtype=np.int32), flags=np.zeros(count, dtype=np.uint32),
               n_frames=np.full(count, nf, dtype=np.uint32))
    for i, k in enumerate(range(first, first + count)):
        wa, wb = levels_ref.window(a, S, k * step), levels_ref.window(b, S, k * step)
        out["flags"][i] = PADDED if k * step + S > n else 0  # past either end is past the shorter one
        read = (nf - 1) * hop + N
        if not (np.isfinite(wa[:read]).all() and np.isfinite(wb[:read]).all()):
            out["flags"][i] |= NONFINITE
            for key in ("peak", "before", "after", "bound", "margin", "curve"):
                out[key][i] = np.nan
            continue
        A, B = frames(wa, N, hop, nf), frames(wb, N, hop, nf)
        G = (A * np.conj(B)).sum(axis=0)
        mag = np.abs(G)
        with np.errstate(divide="ignore", invalid="ignore"):
            psi = np.where(inside, np.where(mag > 0, G / mag, 0.0) if weighting == PHAT else G, 0.0)
        r = np.fft.irfft(psi, N) * N / Z
        r = np.where(r == 0, 0.0, r)  # -0 is stored as +0
        lag, out["margin"][i] = pick(r, max_lag)
        out["curve"][i], out["peak_lag"][i] = r[taus], lag
        out["peak"][i], out["before"][i], out["after"][i] = r[lag], r[lag - 1], r[lag + 1]
        # the header's bound
        Ea, Eb = (ck * np.abs(A) ** 2).sum(axis=1)[:, None], (ck * np.abs(B) ** 2).sum(axis=1)[:, None]
        delta = (eps * (np.abs(B) * np.sqrt(Ea) + np.abs(A) * np.sqrt(Eb)) + eps * eps * np.sqrt(Ea * Eb)).sum(axis=0) \
            + (c["BN_DELAY_ACC_DEPTH"] + 2 * q) * U * (np.abs(A) * np.abs(B)).sum(axis=0)
        tail = eps + c["BN_DELAY_OUT_ULPS"] * U
        if weighting == PHAT:
            with np.errstate(divide="ignore", invalid="ignore"):
                turn = np.where(mag > delta, np.minimum(2.0, delta / (mag - delta)), 2.0)
            per_bin = turn + c["BN_DELAY_PHAT_ULPS"] * U + tail
        else:
            per_bin = delta + tail * mag
        out["bound"][i] = (ck * per_bin)[inside].sum() / Z
    return out


def worst_share(rec, curve, r) -> float:
    """max |got - ref| / bound over peak, before, after and, if given, the curve; a window whose bound is 0 must match exactly; NaN
    must meet NaN"""
    got = np.stack([rec["peak"], rec["before"], rec["after"]], axis=1).astype(np.float64)
    want = np.stack([r["peak"], r["before"], r["after"]], axis=1)
    if curve is not None:
        got, want = np.concatenate([got, curve.astype(np.float64)], axis=1), np.concatenate([want, r["curve"]], axis=1)
    worst = 0.0
    for g, w, b in zip(got, want, r["bound"]):
        if np.isnan(w).any():
            worst = max(worst, 0.0 if np.isnan(g).all() else np.inf)
            continue
        err = np.abs(g - w).max() if np.isfinite(g).all() else np.inf
        worst = max(worst, err / b if b > 0 else (0.0 if err == 0 else np.inf))
    return float(worst)
