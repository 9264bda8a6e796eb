#!/usr/bin/env python3
"""Spectrograms of a whole recording, measured ("Spectrogram"): bn_recording_spectrogram over a synthetic int16
recording of --hours at --rate with frames of --frame every --hop, in four legs -- all bins as floats, all bins as U8 codes, --mels
mel rows as floats and as codes -- next to bn_recording_spectral_profile with planes over the same samples and a pinned
device-to-host copy of each leg's output bytes (what the read-back alone costs).

Per leg: seconds per whole call (the device buffer, the launches, the read-back into pageable host memory) and frames per second.
Every figure is the median of --runs timed calls after one warm-up; the JSON line at the end carries all of them.  The kernels alone
are read from a kernel trace of this same command in a run of its own (rocprofv3 --kernel-trace --stats -- python
tools/spectrogram_bench.py --runs 1).  No rate is a pass condition: the tool measures, tests/test_gpu_spectrogram.py checks.

    python tools/spectrogram_bench.py --hours 1 --rate 48000 --frame 1024 --hop 512 --mels 128
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
    ap.add_argument("--frame", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--fmin", type=float, default=500.0)  # 128 triangles from 0 Hz are narrower than a bin of 1024 at 48 kHz
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    n, N, hop = int(a.hours * 3600 * a.rate), a.frame, a.hop
    sigma = 3000.0
    rec = bn.Recording(np.resize((sigma * np.random.RandomState(1).standard_normal(1 << 20)).astype(np.int16), n))
    frames, K = (n - N) // hop + 1, N // 2 + 1
    bank = bn.Filterbank(0, N, bn.mel_filterbank(a.rate, N, a.mels, a.fmin, a.rate / 2.0))
    u8 = (float(2.0 * (sigma / 32768.0) ** 2 / N * 100.0), 80.0)  # 20 dB above the noise's mean power per bin
    res = {"hours": a.hours, "rate": a.rate, "frame": N, "hop": hop, "frames": frames, "runs": a.runs, "legs": []}
    # the profile with planes over the same samples: one window per frame pair would not be the same work; one window per second is
    S = a.rate // 4 * 4
    prof = timed(lambda: rec.spectral_profile(S, S, N, hop, (0, K)), a.runs)
    res["profile_planes_s"] = prof
    print(f"spectral profile with planes, windows of {S}: {prof[0] * 1e3:9.2f} ms")
    for name, kw, rows, elem in (("bins f32", {"bins": (0, K)}, K, 4), ("bins u8", {"bins": (0, K), "u8": u8}, K, 1),
                                 (f"{a.mels} mel f32", {"bank": bank}, a.mels, 4), (f"{a.mels} mel u8", {"bank": bank, "u8": u8}, a.mels, 1)):
        nbytes = frames * rows * elem
        dev, host = torch.empty(nbytes, dtype=torch.uint8, device="cuda"), torch.empty(nbytes, dtype=torch.uint8).pin_memory()

        def copy():
            host.copy_(dev)
            torch.cuda.synchronize()

        floor = timed(copy, a.runs)
        del dev, host
        torch.cuda.empty_cache()
        t = timed(lambda: rec.spectrogram(0, frames, N, hop, **kw), a.runs)
        res["legs"].append({"leg": name, "bytes": nbytes, "call_s": t, "pinned_copy_s": floor, "frames_per_s": frames / t[0], "over_profile": t[0] / prof[0]})
        print(f"{name:12s} {nbytes / 1e6:8.1f} MB  call {t[0] * 1e3:9.2f} ms  {frames / t[0] / 1e6:7.2f} Mframe/s  pinned copy {floor[0] * 1e3:9.2f} ms  "
              f"{t[0] / prof[0]:7.2f} x profile")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
