#!/usr/bin/env python3
"""Template matching over a whole recording, measured ("Template matching"): bn_recording_template_match of
--templates templates of --template-frames x --mels codes over a synthetic int16 recording of --hours at --rate, frames of --frame
every --hop through a mel bank.

Three times: the whole call (both stages and the read-back of the scores into pageable host memory; the median of --runs calls after
one warm-up), and the image stage and the match stage alone, which are the kernels' times from a kernel trace of one more call in a
child process of its own (rocprofv3 --kernel-trace --stats -- python tools/template_bench.py --child).  The match stage's i8
multiply-adds per second count the true elements, n_templates * frames * rows per offset; tools/sq8_bench.py's scan is the other
user of the instruction, for scale.  No rate is a pass condition: the tool measures, tests/test_gpu_template.py checks.

    python tools/template_bench.py --hours 1 --rate 48000 --frame 1024 --hop 512 --mels 128 --templates 16 --template-frames 64
"""
import argparse
import csv
import glob
import importlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fir_bench import timed  # noqa: E402


def kernel_times(argv):
    """{"image": s, "match": s} per call from a kernel trace of a child that makes two calls; {} with the reason printed if there is
    no profiler or no table"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "tm", "--", sys.executable, os.path.abspath(__file__), "--child"] + argv
        try:
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=600)
        except (OSError, subprocess.SubprocessError) as e:
            print("stages not measured:", e)
            return {}
        out = {"image": 0.0, "match": 0.0}
        for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key, word in (("image", "spectrogram_"), ("match", "template_match_kernel")):
                    if word in row["Name"]:
                        out[key] += float(row["TotalDurationNs"]) * 1e-9 / 2  # the child's warm-up and its one timed call
        return out if out["match"] else {}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=1.0)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--frame", type=int, default=1024)
    ap.add_argument("--hop", type=int, default=512)
    ap.add_argument("--mels", type=int, default=128)
    ap.add_argument("--fmin", type=float, default=500.0)
    ap.add_argument("--templates", type=int, default=16)
    ap.add_argument("--template-frames", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", action="store_true", help="one warm-up and one call and nothing else, for the kernel trace")
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    n, N, hop, W = int(a.hours * 3600 * a.rate), a.frame, a.hop, a.template_frames
    sigma = 3000.0
    rec = bn.Recording(np.resize((sigma * np.random.RandomState(1).standard_normal(1 << 20)).astype(np.int16), n))
    bank = bn.Filterbank(0, N, bn.mel_filterbank(a.rate, N, a.mels, a.fmin, a.rate / 2.0))
    u8 = (float(2.0 * (sigma / 32768.0) ** 2 / N * 100.0), 80.0)  # 20 dB above the noise's mean power per bin
    offsets = (n - N) // hop + 1 - (W - 1)
    image = rec.spectrogram(0, 4 * W * a.templates, N, hop, bank=bank, u8=u8)
    tpl = bn.Templates(0, [image[4 * W * q:4 * W * q + W] for q in range(a.templates)])
    t = timed(lambda: rec.template_match(0, offsets, N, hop, tpl, bank=bank, u8=u8), 1 if a.child else a.runs)
    if a.child:
        return
    macs = float(a.templates) * W * a.mels * offsets
    res = {"hours": a.hours, "rate": a.rate, "frame": N, "hop": hop, "rows": a.mels, "templates": a.templates, "template_frames": W, "offsets": offsets,
           "runs": a.runs, "call_s": t, "offsets_per_s": offsets / t[0], "i8_macs": macs}
    print(f"whole call, {offsets} offsets x {a.templates} templates of {W} x {a.mels}: {t[0] * 1e3:9.2f} ms ({offsets / t[0] / 1e6:.2f} Moffset/s)")
    k = kernel_times([x for x in sys.argv[1:] if x != "--child"])
    if k:
        res.update(image_stage_s=k["image"], match_stage_s=k["match"], match_i8_macs_per_s=macs / k["match"])
        print(f"image stage {k['image'] * 1e3:9.2f} ms   match stage {k['match'] * 1e3:9.2f} ms   {macs / k['match'] / 1e12:.2f} T i8 multiply-adds/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
