#!/usr/bin/env python3
"""Clustering an index: one JSON line per k with the median / min / max over interleaved rounds of

  (a) bn_index_assign (per call and per pass of 64 centroids),
  (b) one iteration of bn_index_cluster: the call with max_iters = 1 from given centroids is assign + update + assign, so an
      iteration (one assign + one update) is that call minus one assign call of the same round,
  (c) the yardstick: bn_head_rank_index with as many classes on the same index (the same bytes and flops per pass).

    python tools/cluster_bench.py --rows 1000000 --dim 1536 --k 64,256,1024

All legs run in one process; within a round they run back to back, so a drift of the machine hits them alike.  A call is host to
host: launches, the passes, the copy of the planes to the host.  --only scan runs legs (a) and (c) alone (for a kernel trace in a process
of its own)."""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KC = 128  # the scan's k-step: slab rows are padded to a multiple of it (csrc/cluster.hip)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}


def timed(fn):
    t = time.perf_counter()
    fn()
    return time.perf_counter() - t


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--k", default="64,256,1024")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chunk", type=int, default=50_000)
    ap.add_argument("--only", choices=["all", "scan"], default="all")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    if bn.device_count() < 1:
        raise SystemExit("cluster_bench needs a gfx950 device")
    rng = np.random.default_rng(0)
    idx = bn.Index(a.device, a.dim, a.rows)
    t0 = time.perf_counter()
    for r0 in range(0, a.rows, a.chunk):
        idx.add(rng.standard_normal((min(a.chunk, a.rows - r0), a.dim), dtype=np.float32))
    fill_s = time.perf_counter() - t0
    slab_bytes = a.rows * ((a.dim + KC - 1) // KC * KC) * 4
    for k in (int(v) for v in a.k.split(",")):
        cent = idx.read(0, k)  # stored rows as centroids
        head = bn.Head(a.device, cent, None, l2norm=True)
        legs = {"assign": lambda: idx.assign(cent)}
        if a.only == "all":
            legs["cluster_1"] = lambda: idx.cluster(k, max_iters=1, init_centroids=cent)
        legs["rank_top"] = lambda: head.rank_index(idx, 100, "top")
        ts = {name: [] for name in legs}
        for r in range(a.warmup + a.rounds):
            for name, fn in legs.items():
                dt = timed(fn)
                if r >= a.warmup:
                    ts[name].append(dt)
        passes = (k + 63) // 64
        out = {"rows": a.rows, "dim": a.dim, "k": k, "slab_bytes": slab_bytes, "passes": passes, "rounds": a.rounds, "fill_s": round(fill_s, 2)}
        for name, v in ts.items():
            out[name] = stats(v)
        for name in ("assign", "rank_top"):
            if name in ts:
                out[name]["ms_per_pass"] = round(float(np.median(ts[name])) * 1e3 / passes, 4)
                out[name]["streamed_GBps"] = round(slab_bytes * passes / float(np.median(ts[name])) / 1e9, 1)
        if "cluster_1" in ts:
            it = np.array(ts["cluster_1"]) - np.array(ts["assign"])
            out["iteration"] = stats(list(it))
            out["update"] = stats(list(it - np.array(ts["assign"])))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
