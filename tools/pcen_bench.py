#!/usr/bin/env python3
"""PCEN of a whole recording, measured ("PCEN"): bn_recording_pcen over a synthetic int16 recording of --hours at
--rate with frames of --frame every --hop and --mels mel rows, as floats and as U8 codes, next to bn_recording_spectrogram of the
same image (stage 1 with its read-back: what a caller without PCEN on the device starts from).

Per leg: seconds per whole call (the device buffers, the launches, the read-back into pageable host memory) and frames per second.
Every figure is the median of --runs timed calls after one warm-up; the JSON line at the end carries all of them.  The kernels alone
are read from a kernel trace of this same command in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/pcen_bench.py --runs 1): pcen_chunk_kernel, pcen_carry_kernel, pcen_apply_kernel.  No rate is a pass condition: the tool
measures, tests/test_gpu_pcen.py checks.

    python tools/pcen_bench.py --hours 1 --rate 48000 --frame 1024 --hop 512 --mels 128
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch  # noqa: F401  before the library: two copies of the runtime in one process cannot both see the GPU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fir_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--frame", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--fmin", type=float, default=500.0)  # 128 triangles from 0 Hz are narrower than a bin of 1024 at 48 kHz
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    n, N, hop = int(a.hours * 3600 * a.rate), a.frame, a.hop
    rec = bn.Recording(np.resize((3000.0 * np.random.RandomState(1).standard_normal(1 << 20)).astype(np.int16), n))
    frames = (n - N) // hop + 1
    bank = bn.Filterbank(0, N, bn.mel_filterbank(a.rate, N, a.mels, a.fmin, a.rate / 2.0))
    res = {"hours": a.hours, "rate": a.rate, "frame": N, "hop": hop, "frames": frames, "rows": a.mels, "runs": a.runs, "legs": []}
    spec = timed(lambda: rec.spectrogram(0, frames, N, hop, bank=bank), a.runs)
    res["spectrogram_f32_s"] = spec
    print(f"spectrogram f32, {a.mels} mel rows: {spec[0] * 1e3:9.2f} ms")
    for name, kw, elem in (("pcen f32", {}, 4), ("pcen u8", {"u8": 4.0}, 1)):
        t = timed(lambda: rec.pcen(0, frames, N, hop, bank=bank, smooth=0.025, gain=1e5, **kw), a.runs)
        res["legs"].append({"leg": name, "bytes": frames * a.mels * elem, "call_s": t, "frames_per_s": frames / t[0], "over_spectrogram": t[0] / spec[0]})
        print(f"{name:10s} {frames * a.mels * elem / 1e6:8.1f} MB  call {t[0] * 1e3:9.2f} ms  {frames / t[0] / 1e6:7.2f} Mframe/s  {t[0] / spec[0]:7.2f} x spectrogram f32")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
