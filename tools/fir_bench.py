#!/usr/bin/env python3
"""FIR filtering of a whole recording, measured ("FIR filtering"): bn_recording_create_filtered over a synthetic
recording of --hours at --rate, for each tap count of --taps, over two sources: int16 mono and 24-bit stereo mixed down.

Per leg: seconds per call (allocation of the result, upload of the packed taps, the kernel, the synchronisation), samples per second,
the multiply-adds per second that implies (n_taps per sample), and the call's time over the memory floor -- a device-to-device copy of
the output's bytes.  Every figure is the median of --runs timed calls after one warm-up; the JSON line at the end carries all of them.
No rate is a pass condition: the tool measures, tests/test_gpu_fir.py checks.

    python tools/fir_bench.py --hours 1 --rate 48000 --taps 63,255,1023
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library: two copies of the runtime in one process cannot both see the GPU

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
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--taps", default="63,255,1023")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    n = int(a.hours * 3600 * a.rate)
    rng = np.random.RandomState(1)
    block = (8000 * rng.standard_normal(1 << 20)).astype(np.int16)
    mono = np.resize(block, n)
    i24 = np.zeros((n, 2, 3), dtype=np.uint8)  # both channels: the int16 value in the upper two bytes of a packed 24-bit sample
    i24[:, :, 1], i24[:, :, 2] = (mono & 0xff).astype(np.uint8)[:, None], ((mono >> 8) & 0xff).astype(np.uint8)[:, None]
    sources = {"i16_mono": bn.Recording(mono), "i24_stereo_mix": bn.Recording.from_layout(i24, bn.BN_PCM_I24, 2, bn.BN_PCM_MIX)}
    del i24

    src, dst = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")

    def copy():
        dst.copy_(src)
        torch.cuda.synchronize()

    floor = timed(copy, a.runs)
    del src, dst
    torch.cuda.empty_cache()
    res = {"hours": a.hours, "rate": a.rate, "samples": n, "runs": a.runs, "copy_s": floor, "copy_GBps": 8.0 * n / floor[0] / 1e9, "legs": []}
    for n_taps in [int(t) for t in a.taps.split(",")]:
        taps = bn.fir_bandpass(a.rate, 150.0, a.rate / 2.0, n_taps)
        for name, rec in sources.items():
            t = timed(lambda: rec.filtered(taps), a.runs)
            res["legs"].append({"source": name, "n_taps": n_taps, "call_s": t, "samples_per_s": n / t[0], "GMACps": n * n_taps / t[0] / 1e9,
                                "over_copy": t[0] / floor[0]})
            print(f"{name:15s} {n_taps:5d} taps  {t[0] * 1e3:9.2f} ms  {n / t[0] / 1e9:7.2f} Gsample/s  {n * n_taps / t[0] / 1e12:6.2f} TMAC/s  {t[0] / floor[0]:6.1f} x copy")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
