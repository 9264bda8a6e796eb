#!/usr/bin/env python3
"""Embedding index scan rate: one JSON line per (rows, dim, queries, top_m) with the median time of 20 timed bn_index_search
calls after warm-up, the slab bytes one call streams, the effective GB/s and the fraction of 6.0 TB/s.

    python tools/index_bench.py --rows 1000000 --dim 1536 --queries 1,8,32,128 --top-m 100

The slab is filled in chunks through bn_index_add_host (host memory stays at one chunk).  A call is host to host: query
upload + normalisation, the scan + merge passes, the copy of the results into pinned memory."""
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
KC = 128  # the scan's k-step: slab rows are padded to a multiple of it (csrc/index.hip)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--queries", default="1,8,32,128")
    ap.add_argument("--top-m", default="100")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=50_000)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    rng = np.random.default_rng(0)
    idx = bn.Index(a.device, a.dim, a.rows)
    t0 = time.perf_counter()
    for r0 in range(0, a.rows, a.chunk):
        idx.add(rng.standard_normal((min(a.chunk, a.rows - r0), a.dim), dtype=np.float32))
    fill_s = time.perf_counter() - t0
    dpad = (a.dim + KC - 1) // KC * KC
    slab_bytes = a.rows * dpad * 4
    for q in (int(v) for v in a.queries.split(",")):
        queries = rng.standard_normal((q, a.dim), dtype=np.float32)
        for m in (int(v) for v in a.top_m.split(",")):
            for _ in range(a.warmup):
                idx.search(queries, m)
            ts = []
            for _ in range(a.iters):
                t = time.perf_counter()
                idx.search(queries, m)
                ts.append(time.perf_counter() - t)
            ms = float(np.median(ts)) * 1e3
            passes = (q + 63) // 64  # each pass of up to 64 queries streams the slab once
            gbs = slab_bytes / (ms * 1e-3) / 1e9
            print(json.dumps({"rows": a.rows, "dim": a.dim, "queries": q, "top_m": m, "median_ms": round(ms, 4),
                              "min_ms": round(min(ts) * 1e3, 4), "slab_bytes": slab_bytes, "passes": passes, "streamed_GBps": round(gbs * passes, 1),
                              "effective_GBps": round(gbs, 1), "fraction_of_6TBps": round(gbs / (HBM_TBS * 1e3), 3),
                              "fill_s": round(fill_s, 2)}), flush=True)


if __name__ == "__main__":
    main()
