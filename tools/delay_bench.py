#!/usr/bin/env python3
"""Cross-channel delay estimation, measured ("Cross-channel delay"): one hour of 48 kHz stereo int16 noise, the right
channel the left one delayed by 11 samples, uploaded once and read as two channel views; 3 s windows (S = 144000), frames of 1024 every
512, all 513 bins, max_lag 128.

  delay        bn_recording_delay over every window, both weightings, with and without the curve: windows per second, launch to
               results on the host.
  yardstick    bn_recording_spectral_profile (no planes) over the same windows of one channel view: that kernel does one transform per
               frame where the delay kernel does two, so it is what the delay rate is read against.

--reps calls back to back per timed run, the variants alternating; every figure is the median of --runs timed runs after one warm-up
round, and the JSON line at the end carries all of them.  No rate is a pass condition: the tool measures, tests/test_gpu_delay.py checks.

    python tools/delay_bench.py --runs 5 --reps 3
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    S, rate, N, hop, max_lag, d = 144000, 48000, 1024, 512, 128, 11
    n_win = int(args.hours * 3600 * rate) // S
    x = (6000 * np.random.RandomState(5).standard_normal(n_win * S + d)).astype(np.int16)
    stereo = bn.Recording.from_layout(np.stack([x[:-d], x[d:]], axis=1), bn.BN_PCM_I16, 2, 0)  # left[n] = right[n - d]
    left, right, bins = stereo.view_channel(0), stereo.view_channel(1), (0, N // 2 + 1)
    lags = left.delay(right, S, S, N, hop, bins, max_lag, bn.BN_DELAY_PHAT)[0]["peak_lag"]
    assert (lags == d).all(), lags
    calls = {"profile_s": lambda: left.spectral_profile(S, S, N, hop, bins, planes=False)}
    for name, weighting in (("plain", bn.BN_DELAY_PLAIN), ("phat", bn.BN_DELAY_PHAT)):
        calls[f"delay_{name}_s"] = lambda w=weighting: left.delay(right, S, S, N, hop, bins, max_lag, w)
        calls[f"delay_{name}_curve_s"] = lambda w=weighting: left.delay(right, S, S, N, hop, bins, max_lag, w, curve=True)
    times = {k: [] for k in calls}
    for r in range(args.runs + 1):  # round 0 warms up
        for k, fn in calls.items():
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            if r:
                times[k].append((time.perf_counter() - t0) / args.reps)
    out = {k: (statistics.median(t), min(t), max(t)) for k, t in times.items()}
    for k in list(calls):
        out[k.replace("_s", "_windows_per_s")] = n_win / out[k][0]
        print(f"{k:22s} median {out[k][0] * 1e3:8.2f} ms  (min {out[k][1] * 1e3:.2f}, max {out[k][2] * 1e3:.2f})  {n_win / out[k][0]:10.0f} windows/s")
    out.update(windows=n_win, frame=N, hop=hop, max_lag=max_lag, reps=args.reps, runs=args.runs, delay_phat_over_profile=out["delay_phat_s"][0] / out["profile_s"][0],
               delay_plain_over_profile=out["delay_plain_s"][0] / out["profile_s"][0])
    print(f"delay (phat, no curve) takes {out['delay_phat_over_profile']:.2f}x the spectral profile's time over the same windows")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
