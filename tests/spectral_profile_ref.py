"""bn_recording_spectral_profile restated in float64 numpy (include/birdnet_hip.h, "bn_recording_spectral_profile"): windows, frames
and the one-sided power P[t, k] are band_levels_ref's; with A = sqrt(P) a window gives, per bin k of [lo, hi), the planes
M_k = mean_t P, S_k = sum_t A, D_k = sum_t |A[t+1] - A[t]|, and aci = sum_k D_k / S_k (0 where S_k == 0), total_mean = mean_t sum_k P.

bounds() is the header's promise as a function of the header's constants.  `wrong` names one of four wrong rules, for
test_spectral_profile_cpu.py's proof that the bounds are not vacuous.  Shared with test_gpu_spectral_profile.py."""
import os
import re

import numpy as np

import band_levels_ref as band
import levels_ref

NONFINITE, PADDED, FRAMES = band.NONFINITE, band.PADDED, band.FRAMES
WRONG = ("power in place of amplitude in plane 2", "last frame dropped", "run boundary differences dropped", "bin_lo moved by one")
U = 2.0 ** -24


def header_constants() -> dict:
    """BN_PROFILE_* and BN_BAND_* as include/birdnet_hip.h declares them"""
    text = open(os.path.join(band.ROOT, "include", "birdnet_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (BN_(?:PROFILE|BAND)_\w+) (\d+)\b", text, flags=re.M)}


def bin_ranges(N):
    """the GPU test's ranges: all bins (lane 0's extra bin, the full store loop), inside one lane's bins, bin N/2 alone"""
    return (0, N // 2 + 1), (3, 17), (N // 2, N // 2 + 1)


def random_case(N, hop, S=8192, windows=5):
    """the inputs of the GPU random-audio test: white int16 noise plus one off-centre tone (band_levels_ref's coloured noise leaves bin
    N/2 of the longest frame too little amplitude for an ACI bound below 1 %), exactly `windows` windows of S at step S // 3, the last
    three reaching past the end"""
    step = S // 3
    n = windows * step
    rng = np.random.RandomState(11 + N + hop)
    tone = 3000 * np.sin(2 * np.pi * np.arange(n) * (N // 8 + 0.37) / N)
    return np.clip(np.round(6000 * rng.standard_normal(n) + tone), -32768, 32767).astype(np.int16), S, step


def profile(x, S, step, N, hop, bins, first=0, count=None, wrong=None):
    """windows [first, first + count) of chunk_audio(x, S, step): planes [count, 3, n_bins], aci, total_mean, root_totals (sum_t
    sqrt(T_t), for the bounds) [count] in float64; flags, n_frames uint32"""
    x = np.asarray(x, dtype=np.float32)
    lo, hi = (bins[0] + 1, bins[1] + 1) if wrong == WRONG[3] else bins
    total = (len(x) + step - 1) // step if len(x) else 0
    count = total - first if count is None else count
    nf = band.n_frames(S, N, hop)
    out = {"planes": np.zeros((count, 3, hi - lo)), "aci": np.zeros(count), "total_mean": np.zeros(count), "root_totals": np.zeros(count),
           "flags": np.zeros(count, dtype=np.uint32), "n_frames": np.full(count, nf, dtype=np.uint32)}
    for i, k in enumerate(range(first, first + count)):
        w = levels_ref.window(x, S, k * step)
        out["flags"][i] = PADDED if k * step + S > len(x) else 0
        if not np.isfinite(w[:(nf - 1) * hop + N]).all():
            out["flags"][i] |= NONFINITE
            for key in ("planes", "aci", "total_mean", "root_totals"):
                out[key][i] = np.inf
            continue
        P = band.frame_powers(w.astype(np.float64), N, hop, frames=nf - 1 if wrong == WRONG[1] and nf > 1 else None)
        A = np.sqrt(P)
        dA = np.abs(np.diff(P if wrong == WRONG[0] else A, axis=0))
        if wrong == WRONG[2]:
            q = -(-nf // 4)
            dA[[t for t in (q - 1, 2 * q - 1, 3 * q - 1) if t < len(dA)]] = 0.0
        M, Sk, D = P.mean(axis=0)[lo:hi], A.sum(axis=0)[lo:hi], dA.sum(axis=0)[lo:hi]
        out["planes"][i] = M, Sk, D
        out["aci"][i] = (D[Sk > 0] / Sk[Sk > 0]).sum()
        out["total_mean"][i] = P.sum(axis=1).mean()
        out["root_totals"][i] = np.sqrt(P.sum(axis=1)).sum()
    return out


def bounds(r, consts=None) -> dict:
    """the header's bounds on planes, aci and total_mean of a profile() result; inf for the aci of a window with a bin whose S_k lies
    inside its own bound"""
    c = header_constants() if consts is None else consts
    eps, q = c["BN_BAND_EPS_ULPS"] * U, -(-r["n_frames"].astype(np.float64) // 4)[:, None]
    delta, delta_a = (c["BN_PROFILE_POW_DEPTH"] + q) * U, (c["BN_PROFILE_AMP_DEPTH"] + q) * U
    M, S, D = r["planes"][:, 0], r["planes"][:, 1], r["planes"][:, 2]
    T, R = r["total_mean"][:, None], eps * r["root_totals"][:, None]
    b0 = 2.0 * eps * np.sqrt(M * T) + eps * eps * T + delta * M
    b1 = R + delta_a * S
    b2 = 2.0 * b1 + delta_a * D
    with np.errstate(divide="ignore", invalid="ignore"):
        per_bin = np.where(S > b1, (b2 + D / S * b1) / (S - b1), np.where((S == 0) & (b1 == 0), 0.0, np.inf))
    return {"planes": np.stack([b0, b1, b2], axis=1), "aci": per_bin.sum(axis=1) + c["BN_PROFILE_ACI_DEPTH"] * U * r["aci"],
            "total_mean": band.bound(r["total_mean"], r["total_mean"], r["n_frames"], c)}


def worst_share(got, r, consts=None) -> dict:
    """per float field, max |got - ref| / bound; a field whose bound is 0 must match exactly (then 0, else inf).  Every float is
    within its bound iff every share is <= 1.  got: planes / aci / total_mean arrays (planes may be missing)"""
    shares = {}
    for k, b in bounds(r, consts).items():
        if k not in got:
            continue
        g, want, share = np.asarray(got[k], dtype=np.float64), r[k], np.zeros(r[k].shape)
        fin = np.isfinite(want)
        share[~fin] = np.where(g[~fin] == want[~fin], 0.0, np.inf)  # +Inf against +Inf
        with np.errstate(invalid="ignore"):
            err, bf = np.abs(g[fin] - want[fin]), b[fin]
            share[fin] = np.where(~np.isfinite(g[fin]), np.inf, np.where(bf > 0, err / np.where(bf > 0, bf, 1.0), np.where(err == 0, 0.0, np.inf)))
        shares[k] = float(share.max()) if share.size else 0.0
    return shares
