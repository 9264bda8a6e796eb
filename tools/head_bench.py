#!/usr/bin/env python3
"""What an attached classifier head costs per step, and how long a fit takes (the library only: no oracle, no reference).

    python tools/head_bench.py [--family perch|v30] [--batch 32] [--rounds 40]

Step time: one context, full-width model, the same device-resident batch; the cases (no head, C = 16, C = 1024) run interleaved in
one process, round by round, so clock and thermal drift hit all of them alike; median and minimum per case over the rounds.
Fit: bn_head_fit on n = 10 000 unit rows of dim 1536 with class offsets, C = 16; wall time and evaluations.  One JSON line."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", default="perch", choices=["perch", "v30"])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--inner", type=int, default=5)
    args = ap.parse_args()
    data = synth.perch_v2() if args.family == "perch" else synth.birdnet_v30()
    with tempfile.NamedTemporaryFile(suffix=".onnx", delete=False) as f:
        f.write(data)
    try:
        model = bn.Model(f.name)
    finally:
        os.unlink(f.name)
    cfg = model.config
    S, sr, dim, B = int(cfg.sample_count), int(cfg.sample_rate), int(cfg.embedding_dim), args.batch
    rec = bn.Recording(np.clip(synth.synthetic_segments(1, S * B, sr)[0], -1, 1).astype(np.float32))
    ctx = bn.Context(model, B)
    rng = np.random.default_rng(0)
    heads = {"none": None}
    for c in (16, 1024):
        heads[f"C{c}"] = bn.Head(0, rng.standard_normal((c, dim)).astype(np.float32), rng.standard_normal(c).astype(np.float32), l2norm=True)
    ctx.step_windows(rec, S, 0, B, 10, None, sync=True)
    d_in = ctx.input_device()[0]
    times = {k: [] for k in heads}
    for r in range(args.rounds + 3):
        for name, h in heads.items():
            ctx.attach_head(h, top_k=10)
            ctx.step_device(d_in, B, 10, None, sync=True)
            t0 = time.perf_counter()
            for _ in range(args.inner):
                ctx.step_device(d_in, B, 10, None, sync=True)
            if r >= 3:
                times[name].append((time.perf_counter() - t0) / args.inner * 1e6)
    out = {"family": args.family, "batch": B, "embedding_dim": dim, "rounds": args.rounds,
           "step_us": {k: {"median": float(np.median(v)), "min": float(np.min(v))} for k, v in times.items()},
           "capture_fallbacks": ctx.stats()["capture_fallbacks"]}
    base = out["step_us"]["none"]["median"]
    out["head_cost_us"] = {k: out["step_us"][k]["median"] - base for k in heads if k != "none"}
    n, C, d = 10000, 16, 1536
    centres = rng.standard_normal((C + 1, d))
    cls = rng.integers(0, C + 1, n)
    X = (rng.standard_normal((n, d)) + 0.5 * centres[cls]).astype(np.float32)
    Y = (cls[:, None] == np.arange(C)[None, :]).astype(np.uint8)
    fits = []
    for _ in range(3):
        t0 = time.perf_counter()
        h = bn.Head.fit(0, X, Y, l2norm=True)
        fits.append(time.perf_counter() - t0)
    out["fit"] = {"n": n, "dim": d, "classes": C, "seconds_median": float(np.median(fits)), "seconds_min": float(np.min(fits)), **h.report}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
