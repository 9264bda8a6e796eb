"""The rule of bn_recording_template_match and bn_template_peaks (include/birdnet_hip.h, "Template matching") in numpy int64 and
float64: the Pearson correlation of each template with the uint8 code image at every frame offset, from exact integer sums."""
import numpy as np


def scores(image_u8, templates, dtype=np.float32):
    """[n_templates, n_offsets] over an image of n_offsets + max_frames - 1 frames; float32 is the rule, float64 its unrounded quotient"""
    s = image_u8.astype(np.int64) - 128
    n = s.shape[0] - max(t.shape[0] for t in templates) + 1
    out = np.zeros((len(templates), n), dtype=dtype)
    for q, t in enumerate(templates):
        tau, W = t.astype(np.int64) - 128, t.shape[0]
        K, T1 = tau.size, tau.sum()
        dT = K * (tau * tau).sum() - T1 * T1
        for o in range(n):
            p = s[o:o + W]
            S1 = p.sum()
            num, dS = K * (tau * p).sum() - T1 * S1, K * (p * p).sum() - S1 * S1
            out[q, o] = np.float64(num) / np.sqrt(np.float64(dT) * np.float64(dS)) if dS else 0.0
    return out


def peaks(sc, min_score, radius, cap=None):
    """[(offset, template, score)]: at least min_score, and every other offset within radius comes after in "score descending, ties
    by offset ascending"; a NaN is never a hit and never suppresses"""
    hits = []
    for q, row in enumerate(sc):
        for t, v in enumerate(row):
            near = [u for u in range(max(t - radius, 0), min(t + radius, len(row) - 1) + 1) if u != t and not np.isnan(row[u])]
            if v >= min_score and all(row[u] < v or (row[u] == v and u > t) for u in near):
                hits.append((t, q, v))
    return hits, hits[:cap]
