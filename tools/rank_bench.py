#!/usr/bin/env python3
"""Ranking an index by a head: one JSON line per class count with the median / min / max over interleaved rounds of

  (a) bn_head_rank_index in both modes,
  (b) bn_index_search with as many queries as classes on the same index (the same bytes and flops: the yardstick),
  (c) the route without it: bn_index_read + bn_head_apply_host + numpy.argpartition on --host-rows rows, reported per row.

    python tools/rank_bench.py --rows 1000000 --dim 1536 --classes 1,8,32,64 --top-m 100

All legs run in one process; within a round they run back to back, so a drift of the machine hits them alike.  A call is host to
host: launches, the scan + merge passes, the copy of the results into pinned memory.  --only rank runs leg (a) alone (for a kernel
trace in a process of its own)."""
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
HBM_TBS = 6.0
KC = 128  # the scan's k-step: slab rows are padded to a multiple of it (csrc/rank.hip)


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
    ap.add_argument("--classes", default="1,8,32,64")
    ap.add_argument("--top-m", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=50_000)
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--only", choices=["all", "rank"], default="all")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    if bn.device_count() < 1:
        raise SystemExit("rank_bench needs a gfx950 device")
    rng = np.random.default_rng(0)
    idx = bn.Index(a.device, a.dim, a.rows)
    t0 = time.perf_counter()
    for r0 in range(0, a.rows, a.chunk):
        idx.add(rng.standard_normal((min(a.chunk, a.rows - r0), a.dim), dtype=np.float32))
    fill_s = time.perf_counter() - t0
    dpad = (a.dim + KC - 1) // KC * KC
    slab_bytes = a.rows * dpad * 4
    m = a.top_m
    for c in (int(v) for v in a.classes.split(",")):
        W = rng.standard_normal((c, a.dim), dtype=np.float32)
        head = bn.Head(a.device, W, rng.standard_normal(c, dtype=np.float32), l2norm=True)
        twin = bn.Head(a.device, W, None, l2norm=False)
        host_rows = min(a.host_rows, a.rows)

        def host_route():
            z = twin.apply(idx.read(0, host_rows))
            return np.argpartition(-z, min(m, host_rows - 1), axis=0)[:m]

        legs = {"rank_top": lambda: head.rank_index(idx, m, "top"), "rank_uncertain": lambda: head.rank_index(idx, m, "uncertain")}
        if a.only == "all":
            legs["search"] = lambda: idx.search(W, m)
            legs["host_route"] = host_route
        ts = {k: [] for k in legs}
        for r in range(a.warmup + a.rounds):
            for k, fn in legs.items():
                if k == "host_route" and r not in (a.warmup, a.warmup + 1, a.warmup + 2):  # three rounds of the slow leg are enough
                    continue
                dt = timed(fn)
                if r >= a.warmup:
                    ts[k].append(dt)
        passes = (c + 63) // 64  # each pass of up to 64 classes streams the slab once
        out = {"rows": a.rows, "dim": a.dim, "classes": c, "top_m": m, "slab_bytes": slab_bytes, "passes": passes, "rounds": a.rounds, "fill_s": round(fill_s, 2)}
        for k, v in ts.items():
            out[k] = stats(v)
            if k == "host_route":
                out[k]["rows"] = host_rows
                out[k]["us_per_row"] = round(float(np.median(v)) * 1e6 / host_rows, 4)
            else:
                gbs = slab_bytes * passes / float(np.median(v)) / 1e9
                out[k]["streamed_GBps"] = round(gbs, 1)
                out[k]["fraction_of_6TBps"] = round(gbs / (HBM_TBS * 1e3), 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
