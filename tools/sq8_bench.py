#!/usr/bin/env python3
"""Coarse int8 search with exact re-rank (bn_sq8_*) against the exact search on one index, in one process.

    python tools/sq8_bench.py [--rows 1000000] [--dim 1536] [--rounds 5] [--json out.json]
    python tools/sq8_bench.py --trace      # per-kernel times from a `rocprofv3 --kernel-trace --stats` run in a process of its own

Random unit rows; queries are a stored row plus noise.  The view's build and an extend over 4 096 appended rows are timed; then for Q in
{1, 8, 32, 128} and refine in {128, 256} at M = 100: host-to-host milliseconds as median (min-max) over interleaved rounds (every round
runs the exact search and every cell once, so drift hits all legs alike), recall@100 against bn_index_search, the time ratio to
bn_index_search of the same round, and the bandwidth bound rows x (padded dim + 5) bytes / 6 TB/s.  The first round is a warm-up and is
dropped.  Recall on random rows says little about real embeddings."""
import argparse
import csv
import glob
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")

QS, REFINES, M, EXTEND_ROWS = (1, 8, 32, 128), (128, 256), 100, 4096
HBM_BYTES_PER_S = 6e12
KERNELS = ("sq8_encode", "sq8_scan", "sq8_members", "ivf_scan", "ivf_merge", "index_scan", "index_merge", "index_normalise", "index_gather")


def trace(argv):
    """runs this tool's --trace-pass under rocprofv3 in a child process and prints the kernels' totals"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace-pass"] + argv
        subprocess.run(cmd, check=True)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        print("%-24s %8s %12s %12s" % ("kernel", "calls", "total ms", "mean us"))
        for row in csv.DictReader(open(files[0])):
            name = row["Name"]
            short = next((k for k in KERNELS if k in name), None)
            if short:
                print("%-24s %8s %12.3f %12.1f" % (short + ("<%s>" % name.split("<")[1].split(">")[0] if "<" in name else ""), row["Calls"],
                                                 float(row["TotalDurationNs"]) / 1e6, float(row["AverageNs"]) / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-pass", action="store_true", help="one pass over the cells and nothing else (what --trace profiles)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.trace:
        return trace(["--rows", str(a.rows), "--dim", str(a.dim)])
    if bn.device_count() < 1:
        raise SystemExit("sq8_bench needs a gfx950 device")
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows + EXTEND_ROWS)
    block = rng.standard_normal((32768, a.dim), dtype=np.float32)
    for c, r0 in enumerate(range(0, a.rows, 32768)):     # one Gaussian block, rotated along k by the chunk number: every row stays Gaussian
        idx.add(np.roll(block, c, axis=1)[:min(32768, a.rows - r0)])
    dpad = (a.dim + 127) // 128 * 128
    t = time.perf_counter()
    view = bn.Sq8(idx)
    t_build = time.perf_counter() - t
    idx.add(rng.standard_normal((EXTEND_ROWS, a.dim), dtype=np.float32))
    t = time.perf_counter()
    view.extend()
    t_extend = time.perf_counter() - t
    rows = view.rows
    bound = rows * (dpad + 5) / HBM_BYTES_PER_S * 1e3
    out = {"rows": rows, "dim": a.dim, "build_s": t_build, "extend_s": t_extend, "extend_rows": EXTEND_ROWS, "bound_ms": bound, "cells": []}
    print("build %.4f s (%d rows), extend %.4f s (%d rows), bound %.3f ms" % (t_build, a.rows, t_extend, EXTEND_ROWS, bound), flush=True)
    base = idx.read(0, max(QS))
    Qall = (base + (0.5 / np.sqrt(a.dim)) * rng.standard_normal((max(QS), a.dim))).astype(np.float32)
    if a.trace_pass:
        for nq in QS:
            idx.search(Qall[:nq], M)
            for r in REFINES:
                view.search(Qall[:nq], r, M)
        return
    times, exact, got = {}, {}, {}
    for rnd in range(a.rounds + 1):
        for nq in QS:
            t = time.perf_counter()
            exact[nq] = idx.search(Qall[:nq], M)
            te = time.perf_counter() - t
            for r in REFINES:
                t = time.perf_counter()
                got[nq, r] = view.search(Qall[:nq], r, M)
                ti = time.perf_counter() - t
                if rnd:
                    times.setdefault((nq, r), []).append((ti, te))
    print("%4s %6s | %28s | %9s | %18s | %8s | %8s" % ("Q", "refine", "sq8 ms median (min-max)", "recall", "exact ms", "ratio", "bound ms"))
    for nq in QS:
        for r in REFINES:
            ti = [1e3 * x[0] for x in times[nq, r]]
            te = [1e3 * x[1] for x in times[nq, r]]
            ratio = statistics.median(x[0] / x[1] for x in times[nq, r])
            ids, _, cnt, _, _ = got[nq, r]
            eids = exact[nq][0]
            recall = float(np.mean([len(np.intersect1d(ids[q, :cnt[q]], eids[q])) / M for q in range(nq)]))
            cell = {"Q": nq, "refine": r, "sq8_ms": [statistics.median(ti), min(ti), max(ti)], "exact_ms": [statistics.median(te), min(te), max(te)],
                    "recall": recall, "ratio": ratio}
            out["cells"].append(cell)
            print("%4d %6d | %10.3f (%7.3f-%7.3f) | %9.4f | %8.3f (%7.3f) | %8.4f | %8.4f" %
                  (nq, r, cell["sq8_ms"][0], min(ti), max(ti), recall, cell["exact_ms"][0], min(te), ratio, bound), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
