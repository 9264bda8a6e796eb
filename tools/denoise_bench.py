#!/usr/bin/env python3
"""Noise reduction of a whole recording, measured ("Noise reduction"): bn_recording_create_denoised over a synthetic
int16 recording of --hours at --rate, for each frame length of --frames, next to a device-to-device copy of the output's bytes (the
memory floor) and bn_recording_create_filtered at --taps taps on the same recording.

Per leg: seconds per call (allocation of the result, upload of the thresholds, the kernel, the synchronisation) and samples per
second.  Every figure is the median of --runs timed calls after one warm-up; the JSON line at the end carries all of them.  No rate
is a pass condition: the tool measures, tests/test_gpu_denoise.py checks.

    python tools/denoise_bench.py --hours 1 --rate 48000 --frames 512,1024
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch  # before the library: two copies of the runtime in one process cannot both see the GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fir_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--frames", default="512,1024")
    ap.add_argument("--taps", type=int, default=255)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    n = int(a.hours * 3600 * a.rate)
    sigma = 3000.0
    rec = bn.Recording(np.resize((sigma * np.random.RandomState(1).standard_normal(1 << 20)).astype(np.int16), n))
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    floor = timed(copy, a.runs)
    del src, dst
    torch.cuda.empty_cache()
    taps = bn.fir_bandpass(a.rate, 150.0, a.rate / 2.0, a.taps)
    fir = timed(lambda: rec.filtered(taps), a.runs)
    res = {"hours": a.hours, "rate": a.rate, "samples": n, "runs": a.runs, "copy_s": floor, "fir_taps": a.taps, "fir_s": fir, "legs": []}
    print(f"copy {floor[0] * 1e3:9.2f} ms   fir {a.taps} taps {fir[0] * 1e3:9.2f} ms")
    for N in [int(f) for f in a.frames.split(",")]:
        noise = np.full(N // 2 + 1, 2.0 * (sigma / 32768.0) ** 2 / N, dtype=np.float32)
        t = timed(lambda: rec.denoised(N, noise, 2.0, 0.1), a.runs)
        res["legs"].append({"frame": N, "call_s": t, "samples_per_s": n / t[0], "over_copy": t[0] / floor[0], "over_fir": t[0] / fir[0]})
        print(f"frame {N:5d}  {t[0] * 1e3:9.2f} ms  {n / t[0] / 1e9:7.2f} Gsample/s  {t[0] / floor[0]:6.1f} x copy  {t[0] / fir[0]:6.2f} x fir")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
