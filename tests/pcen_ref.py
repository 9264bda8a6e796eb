"""The rule of bn_recording_pcen (include/birdnet_hip.h, "PCEN") in numpy float64: a plain loop over frames on the float32 image and
the float32 parameters, with the skip of non-finite elements and the smoother's bound B[t] run beside M.  No float32 emulation
(only "is gain * E finite in float32" is asked in float32) and no chunking."""
import os
import re

import numpy as np

U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_constants() -> dict:
    """BN_PCEN_* as include/birdnet_hip.h declares them"""
    text = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define (BN_PCEN_\w+) (\d+)\b", text, flags=re.M)}


def pcen(E, smooth, gain, alpha, delta, r, eps, state=None, keep=None):
    """(V, M, B, bound) of the float32 image E [T, R], each [T, R] float64 (only the frames where `keep` is true, if given): the value
    (+Inf where gain * E is not finite), the smoother, its bound, and the value's bound; then M and B behind the last frame"""
    c = header_constants()
    s, g, alpha, delta, r, eps = (float(np.float32(v)) for v in (smooth, gain, alpha, delta, r, eps))
    a, (T, R) = 1.0 - s, E.shape
    keep = np.ones(T, bool) if keep is None else keep
    pos, out = np.cumsum(keep) - 1, np.zeros((4, int(keep.sum()), R))
    with np.errstate(over="ignore"):
        fin0 = np.isfinite(np.float32(g) * E[0])
    M = np.where(fin0, g * E[0].astype(np.float64), 0.0) if state is None else np.asarray(state, np.float32).astype(np.float64)
    B = np.zeros(R)
    for t in range(T):
        with np.errstate(over="ignore"):
            fin = np.isfinite(np.float32(g) * E[t])
        x = np.where(fin, g * E[t].astype(np.float64), 0.0)
        M = np.where(fin, a * M + s * x, M)
        B = np.where(fin, a * B + c["BN_PCEN_SMOOTH_DEPTH"] * U * M, B)
        if keep[t]:
            y = (x / (eps + M) ** alpha + delta) ** r
            bound = (alpha * r * B / (eps + M) + c["BN_PCEN_VALUE_DEPTH"] * U) * y
            out[:, pos[t]] = np.where(fin, y - delta ** r, np.inf), M, B, np.where(fin, bound, 0.0)
    return out[0], out[1], out[2], out[3], M, B
