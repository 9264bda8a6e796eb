#!/usr/bin/env python3
"""What an attached species prior costs per step (the library only: no oracle, no reference).

    python tools/prior_bench.py [--batch 32] [--contexts 4] [--sources 1024] [--rounds 12] [--steps-only N]

Full-width BirdNET v2.4 synth.  Two measurements, each with the cases (no prior, SELECT, SELECT + rerank, AFTER_TOPK) interleaved
round by round in one process, so clock and thermal drift hit all of them alike; median and minimum per case over the rounds:

  pool    `contexts` contexts stepping ONE live pool of `sources` sources at `sources` sites (source s at site s, a table of
          sources x num_species): every round pushes one window per source and the contexts take the ready windows round robin,
          sync = 0, each context's previous step collected before it steps again; wall time per step of `batch` windows.
  single  one context, the same device-resident batch, synchronous steps: the difference to the no-prior case is what the prior's
          launches add to one step's latency.

--steps-only N runs N synchronous single-context steps with a SELECT prior attached and prints nothing else: the process to put
under `rocprofv3 --kernel-trace --stats`, which then lists prior_select_kernel next to the step's own top-K kernel.  One JSON line."""
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
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--steps-only", type=int, default=0)
    args = ap.parse_args()
    with tempfile.NamedTemporaryFile(suffix=".onnx", delete=False) as f:
        f.write(synth.birdnet_v24())
    try:
        model = bn.Model(f.name)
    finally:
        os.unlink(f.name)
    cfg = model.config
    S, sr, n, B = int(cfg.sample_count), int(cfg.sample_rate), int(cfg.num_species), args.batch
    rng = np.random.default_rng(0)
    table = rng.uniform(0, 1, (args.sources, n)).astype(np.float32)
    table[rng.uniform(size=table.shape) < 0.1] = bn.BN_PRIOR_UNKNOWN
    priors = {"none": None, "select": bn.Prior(0, table, 0.5), "select_rerank": bn.Prior(0, table, 0.5, rerank=True),
              "after_topk": bn.Prior(0, table, 0.5, after_topk=True, rerank=True)}
    site_map = np.arange(args.sources, dtype=np.int32)
    rec = bn.Recording(np.clip(synth.synthetic_segments(1, S * B, sr)[0], -1, 1).astype(np.float32))
    ctxs = [bn.Context(model, B) for _ in range(args.contexts)]
    for c in ctxs:  # capture the batch's graph outside the timings
        c.step_windows(rec, S, 0, B, args.top_k, None, sync=True)
    one = ctxs[0]
    d_in = one.input_device()[0]

    if args.steps_only:
        one.attach_prior(priors["select"], top_k=args.top_k)
        for _ in range(args.steps_only):
            one.step_device(d_in, B, args.top_k, None, sync=True)
        return

    # ---- single context, synchronous
    single = {k: [] for k in priors}
    for r in range(args.rounds + 3):
        for name, p in priors.items():
            one.attach_prior(p, top_k=args.top_k)
            one.step_device(d_in, B, args.top_k, None, sync=True)
            t0 = time.perf_counter()
            for _ in range(args.inner):
                one.step_device(d_in, B, args.top_k, None, sync=True)
            if r >= 3:
                single[name].append((time.perf_counter() - t0) / args.inner * 1e6)

    # ---- the pool
    live = bn.Live(0, args.sources, S, S, 2 * S + S, bn.BN_PCM_I16)
    block = rng.integers(-32768, 32768, size=2 * S).astype(np.int16)
    srcs = list(range(args.sources))
    pool = {k: [] for k in priors}
    for r in range(args.rounds + 2):
        for name, p in priors.items():
            for c in ctxs:
                c.attach_prior(p, source_sites=site_map, top_k=args.top_k)
            live.push_many(srcs, [block[(s * 997) % S:][:S] for s in srcs])
            pending = [False] * len(ctxs)
            steps, turn = 0, 0
            t0 = time.perf_counter()
            while live.ready(-1):
                i = turn % len(ctxs)
                turn += 1
                if pending[i]:
                    ctxs[i].synchronize()
                src, _ = ctxs[i].step_live(live, B, args.top_k, None, sync=False)
                pending[i] = len(src) > 0
                steps += 1 if len(src) else 0
            for c in ctxs:
                c.synchronize()
            if r >= 2 and steps:
                pool[name].append((time.perf_counter() - t0) / steps * 1e6)

    def summary(t):
        return {k: {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2)} for k, v in t.items()}

    out = {"model": "v24", "num_species": n, "batch": B, "contexts": args.contexts, "sources": args.sources, "sites": args.sources,
           "top_k": args.top_k, "rounds": args.rounds, "table_mb": round(table.nbytes / 1e6, 1),
           "single_step_us": summary(single), "pool_step_us": summary(pool),
           "capture_fallbacks": sum(c.stats()["capture_fallbacks"] for c in ctxs)}
    for key in ("single_step_us", "pool_step_us"):
        base = out[key]["none"]["median"]
        out[key.replace("step_us", "prior_cost_us")] = {k: round(v["median"] - base, 2) for k, v in out[key].items() if k != "none"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
