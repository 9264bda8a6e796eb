"""bn_recording_levels restated in float64 numpy (include/birdnet_hip.h, "Window levels and list steps"): a window's S samples are
chunk_audio's -- the layout rule's f32 samples (tests/pcm_ref.py), zeros past the end -- and its levels are

    peak          max |s|                 exact in f32: a maximum rounds nothing
    mean          (sum s) / S             float64 here
    mean_square   (sum s*s) / S           float64 here; the divisor is S, padding included
    flags         PADDED iff the window reaches past the last sample; NONFINITE iff any sample is NaN or +-Inf, and then
                  peak = mean_square = +Inf, mean = 0

The device computes mean and mean_square in f32 in a fixed tree; bounds() gives what the header promises of them from
BN_LEVEL_SUM_DEPTH.  Shared by test_window_list_cpu.py (this file against hand-computed cases) and test_gpu_levels.py."""
import numpy as np

import pcm_ref

NONFINITE, PADDED = 1, 2


def window(x, S, start) -> np.ndarray:
    """the S samples of the window that starts at frame `start` of the f32 samples x: zeros past the end"""
    out = np.zeros(S, dtype=np.float32)
    seg = np.asarray(x, dtype=np.float32)[start:start + S]
    out[:len(seg)] = seg
    return out


def window_levels(w, padded):
    """(peak f32, mean f64, mean_square f64, flags, mean|s| f64) of one window's samples"""
    w = np.asarray(w, dtype=np.float32)
    flags = PADDED if padded else 0
    if not np.isfinite(w).all():
        return np.float32(np.inf), 0.0, np.inf, flags | NONFINITE, np.inf
    d = w.astype(np.float64)
    S = len(w)
    return np.float32(np.abs(w).max()) if S else np.float32(0), float(d.sum() / S), float((d * d).sum() / S), flags, float(np.abs(d).sum() / S)


def levels(x, S, step, first=0, count=None):
    """the levels of windows [first, first + count) of chunk_audio(x, S, step) as a dict of arrays: peak (float32), mean,
    mean_square, mean_abs (float64), flags (uint32)"""
    x = np.asarray(x, dtype=np.float32)
    total = (len(x) + step - 1) // step if len(x) else 0
    count = total - first if count is None else count
    assert 0 <= first and first + count <= total
    rows = [window_levels(window(x, S, k * step), k * step + S > len(x)) for k in range(first, first + count)]
    return {"peak": np.array([r[0] for r in rows], dtype=np.float32), "mean": np.array([r[1] for r in rows], dtype=np.float64),
            "mean_square": np.array([r[2] for r in rows], dtype=np.float64), "flags": np.array([r[3] for r in rows], dtype=np.uint32),
            "mean_abs": np.array([r[4] for r in rows], dtype=np.float64)}


def bounds(ref, depth):
    """(absolute bound on mean, relative bound on mean_square) per window, from the header's BN_LEVEL_SUM_DEPTH"""
    u = 2.0 ** -24
    return (depth + 1) * u * ref["mean_abs"], (depth + 2) * u


def tree_depth(S):
    """the longest chain of additions a term passes through in the device's tree at this S (csrc/levels.hip): ceil(S / 1024) in one
    of the 1024 accumulators, then 2 + 6 + 2; BN_LEVEL_SUM_DEPTH is its value at S = 2^20.  The header's derivation
    holds for any S with this depth in place of the constant, so bounds(ref, tree_depth(S)) is the same promise at the tree's own
    depth -- at S = 144000 (depth 151) tight enough to notice one dropped or doubled sample of ordinary audio"""
    return -(-S // 1024) + 10


def samples(raw, fmt, channels=1, channel=0) -> np.ndarray:
    """the f32 samples of a layout recording: pcm_ref's rule"""
    return pcm_ref.mono(raw, fmt, channels, channel)


def gate(peaks, threshold, hangover=1) -> np.ndarray:
    """the windows a host gate keeps: peak >= threshold, plus `hangover` windows either side; ascending window numbers"""
    loud = np.flatnonzero(np.asarray(peaks) >= np.float32(threshold))
    keep = np.zeros(len(peaks), dtype=bool)
    for k in loud:
        keep[max(0, k - hangover):k + hangover + 1] = True
    return np.flatnonzero(keep)
