#!/usr/bin/env python3
"""Probed (IVF) search against the exact search on one index, in one process.

    python tools/ivf_bench.py [--rows 1000000] [--dim 1536] [--k 1024] [--iters 3] [--rounds 5] [--json out.json]
    python tools/ivf_bench.py --trace      # one pass over the cells and nothing else, for `rocprofv3 --kernel-trace -- python ...`

Random unit rows (the worst case for a partition: there is no cluster structure to find), centroids from bn_index_cluster with a few
iterations (timed), the view's build (timed), then for Q in {1, 8, 32, 128} and nprobe in {1, 8, 32, 128} at M = 100: host-to-host
milliseconds as median (min-max) over interleaved rounds (every round runs the exact search and every cell once, so drift hits all
legs alike), rows scanned, recall@100 against bn_index_search, the time ratio to bn_index_search of the same round, and the bandwidth
bound scanned rows x padded dim x 4 bytes / 6 TB/s.  The first round is a warm-up and is dropped."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")

QS, NPROBES, M = (1, 8, 32, 128), (1, 8, 32, 128), 100
HBM_BYTES_PER_S = 6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if bn.device_count() < 1:
        raise SystemExit("ivf_bench needs a gfx950 device")
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows)
    for r0 in range(0, a.rows, 32768):
        idx.add(rng.standard_normal((min(32768, a.rows - r0), a.dim), dtype=np.float32))
    dpad = (a.dim + 127) // 128 * 128
    t = time.perf_counter()
    cent, assign, score, counts, rep = idx.cluster(a.k, max_iters=a.iters)
    t_cluster = time.perf_counter() - t
    t = time.perf_counter()
    ivf = bn.Ivf(idx, cent)
    t_build = time.perf_counter() - t
    sizes = ivf.list_sizes()
    out = {"rows": a.rows, "dim": a.dim, "k": a.k, "cluster_s": t_cluster, "cluster_iters": rep["iters"], "build_s": t_build,
           "list_min": int(sizes.min()), "list_max": int(sizes.max()), "cells": []}
    print("cluster (%d updates) %.2f s, build %.3f s, lists %d..%d rows" % (rep["iters"], t_cluster, t_build, sizes.min(), sizes.max()), flush=True)
    Qall = rng.standard_normal((max(QS), a.dim), dtype=np.float32)
    nprobes = [p for p in NPROBES if p <= a.k]
    if a.trace:
        for nq in QS:
            idx.search(Qall[:nq], M)
            for p in nprobes:
                ivf.search(Qall[:nq], p, M)
        return
    times = {}
    exact, got = {}, {}
    for rnd in range(a.rounds + 1):
        for nq in QS:
            t = time.perf_counter()
            exact[nq] = idx.search(Qall[:nq], M)
            te = time.perf_counter() - t
            for p in nprobes:
                t = time.perf_counter()
                got[nq, p] = ivf.search(Qall[:nq], p, M)
                ti = time.perf_counter() - t
                if rnd:
                    times.setdefault((nq, p), []).append((ti, te))
    print("%4s %6s | %28s | %10s | %9s | %18s | %8s | %8s" % ("Q", "nprobe", "ivf ms median (min-max)", "rows/query", "recall", "exact ms", "ratio", "bound ms"))
    for nq in QS:
        for p in nprobes:
            ti = [1e3 * x[0] for x in times[nq, p]]
            te = [1e3 * x[1] for x in times[nq, p]]
            ratio = statistics.median(x[0] / x[1] for x in times[nq, p])
            ids, _, cnt, _, scanned = got[nq, p]
            eids = exact[nq][0]
            recall = float(np.mean([len(np.intersect1d(ids[q, :cnt[q]], eids[q])) / M for q in range(nq)]))
            bound = float(scanned.sum()) * dpad * 4 / HBM_BYTES_PER_S * 1e3
            cell = {"Q": nq, "nprobe": p, "ivf_ms": [statistics.median(ti), min(ti), max(ti)], "exact_ms": [statistics.median(te), min(te), max(te)],
                    "rows_per_query": float(scanned.mean()), "recall": recall, "ratio": ratio, "bound_ms": bound}
            out["cells"].append(cell)
            print("%4d %6d | %10.3f (%7.3f-%7.3f) | %10.0f | %9.4f | %8.3f (%7.3f) | %8.4f | %8.4f" %
                  (nq, p, cell["ivf_ms"][0], min(ti), max(ti), cell["rows_per_query"], recall, cell["exact_ms"][0], min(te), ratio, bound), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
