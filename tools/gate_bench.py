#!/usr/bin/env python3
"""Window levels and list steps, measured: three legs over a synthetic BirdNET-v2.4-style model.

  gating       a synthetic recording of --hours with a --loud share of loud windows: bn_step_windows over every window, against
               bn_recording_levels + a host gate (peak >= 0.01, one window of hangover) + bn_step_window_list over the kept windows
               only; and the level pass alone, in GB/s of stored bytes.
  band gate    the same hour with a 60 Hz rumble at -20 dBFS under everything and the calls at -50 dBFS: the windows the peak gate keeps
               (all of them), the windows a 2 - 10 kHz gate on bn_recording_band_levels' max keeps, the band pass alone in GB/s of
               stored bytes next to the level pass, and the band-gated run.
  short files  --files recordings of 4 windows each: one bn_step_windows per recording, against list steps of --batch rows.

Every figure is the median of --runs timed runs after one warm-up; the JSON line at the end carries all of them.  No rate is a
pass condition: the tool measures, tests/test_gpu_window_list.py checks.

    python tools/gate_bench.py --hours 1 --loud 0.05 --runs 5
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--loud", type=float, default=0.05, help="share of loud windows")
    ap.add_argument("--files", type=int, default=512)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--width", type=float, default=1.0)
    ap.add_argument("--depth", type=float, default=1.0)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
    with tempfile.NamedTemporaryFile(suffix=".onnx", delete=False) as f:
        f.write(synth.birdnet_v24(num_species=6522, width=a.width, depth=a.depth))
        path = f.name
    try:
        model = bn.Model(path)
    finally:
        os.unlink(path)
    S, B, K = int(model.config.sample_count), a.batch, 10
    ctx = bn.Context(model, B)
    rng = np.random.RandomState(1)
    res = {"S": S, "batch": B, "runs": a.runs}

    # ---- gating leg
    n_win = int(a.hours * 3600 * int(model.config.sample_rate)) // S
    x = np.zeros(n_win * S, dtype=np.int16)
    loud = np.sort(rng.choice(n_win, max(1, int(round(a.loud * n_win))), replace=False))
    for k in loud:
        x[k * S + S // 4:k * S + S // 2] = (6000 * np.sin(np.arange(S // 4) * 0.2)).astype(np.int16)
    rec = bn.Recording(x)

    def everything():
        for first in range(0, n_win, B):
            ctx.step_windows(rec, S, first, min(B, n_win - first), K, None, sync=False)
        ctx.synchronize()

    kept = []

    def gated():
        lv = rec.levels(S, S)
        hit = np.flatnonzero(lv["peak"] >= np.float32(0.01))
        keep = np.zeros(n_win, dtype=bool)
        for d in (-1, 0, 1):
            keep[np.clip(hit + d, 0, n_win - 1)] = True
        ks = np.flatnonzero(keep)
        kept[:] = [len(ks)]
        for i in range(0, len(ks), B):
            ctx.step_window_list([(rec, int(k) * S, 0, int(k)) for k in ks[i:i + B]], K, None, sync=False)
        ctx.synchronize()

    t_all, t_gate, t_lv = timed(everything, a.runs), timed(gated, a.runs), timed(lambda: rec.levels(S, S), a.runs)
    res["gating"] = {"windows": n_win, "loud": len(loud), "kept": kept[0], "all_s": t_all, "gated_s": t_gate, "levels_s": t_lv,
                     "levels_GBps": x.nbytes / t_lv[0] / 1e9}
    del rec

    # ---- band-gate leg: rumble under everything, the calls 30 dB below it
    rate, N, hop = int(model.config.sample_rate), 1024, 512
    band = bn.band_bins(rate, N, 2000.0, 10000.0)
    y = 3276.8 * np.sin(2 * np.pi * 60.0 * np.arange(n_win * S) / rate)
    for k in loud:
        y[k * S + S // 4:k * S + S // 2] += 103.6 * np.sin(2 * np.pi * 5000.0 * np.arange(S // 4) / rate)
    y = np.round(y).astype(np.int16)
    rec = bn.Recording(y)
    by_peak = int((rec.levels(S, S)["peak"] >= np.float32(0.01)).sum())
    quiet_max = np.delete(rec.band_levels(S, S, N, hop, [band])["max"][:, 0], loud)
    threshold = np.float32(10.0 * max(float(quiet_max.max()), 1e-12)) if len(quiet_max) else np.float32(1e-9)   # 10 dB over the loudest quiet window

    def band_gated():
        bl = rec.band_levels(S, S, N, hop, [band])
        hit = np.flatnonzero(bl["max"][:, 0] >= threshold)
        keep = np.zeros(n_win, dtype=bool)
        for d in (-1, 0, 1):
            keep[np.clip(hit + d, 0, n_win - 1)] = True
        ks = np.flatnonzero(keep)
        kept[:] = [len(ks), len(hit)]
        for i in range(0, len(ks), B):
            ctx.step_window_list([(rec, int(k) * S, 0, int(k)) for k in ks[i:i + B]], K, None, sync=False)
        ctx.synchronize()

    t_band_gate = timed(band_gated, a.runs)
    t_bl, t_lv = timed(lambda: rec.band_levels(S, S, N, hop, [band]), a.runs), timed(lambda: rec.levels(S, S), a.runs)
    res["band_gate"] = {"windows": n_win, "calls": len(loud), "kept_by_peak": by_peak, "hit_by_band": kept[1], "kept_by_band": kept[0], "frame": N, "hop": hop,
                        "bins": list(band), "threshold": float(threshold), "band_gated_s": t_band_gate, "band_levels_s": t_bl, "levels_s": t_lv,
                        "band_levels_GBps": y.nbytes / t_bl[0] / 1e9, "levels_GBps": y.nbytes / t_lv[0] / 1e9}
    del rec, x, y

    # ---- short-files leg
    clips = [bn.Recording((3000 * rng.standard_normal(4 * S)).astype(np.int16)) for _ in range(a.files)]

    def per_file():
        for r in clips:
            ctx.step_windows(r, S, 0, 4, K, None, sync=False)
        ctx.synchronize()

    refs = [(r, k * S, 0, i * 4 + k) for i, r in enumerate(clips) for k in range(4)]

    def listed():
        for i in range(0, len(refs), B):
            ctx.step_window_list(refs[i:i + B], K, None, sync=False)
        ctx.synchronize()

    res["short_files"] = {"files": a.files, "windows": len(refs), "per_file_s": timed(per_file, a.runs), "list_s": timed(listed, a.runs)}
    res["capture_fallbacks"] = ctx.stats()["capture_fallbacks"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
