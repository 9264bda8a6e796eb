#!/usr/bin/env python3
"""Window levels and list steps, measured: two legs over a synthetic BirdNET-v2.4-style model.

  gating       a synthetic recording of --hours with a --loud share of loud windows: bn_step_windows over every window, against
               bn_recording_levels + a host gate (peak >= 0.01, one window of hangover) + bn_step_window_list over the kept windows
               only; and the level pass alone, in GB/s of stored bytes.
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
    del rec, x

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
