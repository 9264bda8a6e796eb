#!/usr/bin/env python3
"""Sequence search (bn_index_search_seq) against the exact search with the same number of query rows, on one index, in one process.

    python tools/seq_bench.py [--rows 1000000] [--dim 1536] [--rounds 5] [--json out.json]

The rows are Gaussian (one block, rotated along k per chunk, so the fill is cheap); a sequence is seq_len consecutive stored rows plus
noise, so every sequence has its match.  Times, host to host in milliseconds as median (min-max) over interleaved rounds (every round
runs every leg once, so drift hits all legs alike; the first round is a warm-up and is dropped):

  * for seq_len L in {1, 2, 8, 16, 33, 64} and n_seq in {1, what fills 64 query rows, what one pass holds}: bn_index_search with
    L * n_seq queries, then bn_index_search_seq at peak_radius 0 and 8, each with its ratio to bn_index_search of the same round.

A pass holds min(64 // L, 28) sequences, so the legs with n_seq = 64 // L > 28 (L = 1, 2) take more passes than bn_index_search does, and
L = 33 leaves 31 of the 64 query rows idle; the `rows_per_pass` column says how full the passes are.  Before anything is timed, L = 1 at
radius 0 is checked against bn_index_search's bytes and every sequence must find its own start first."""
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

LS, M, RADII = (1, 2, 8, 16, 33, 64), 100, (0, 8)
CAP = 28         # sequences per pass at most (csrc/seq_plan.h)
NOISE = 0.3
CHUNK = 8192


def med(ts):
    ms = [1e3 * t for t in ts]
    return [statistics.median(ms), min(ms), max(ms)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if bn.device_count() < 1:
        raise SystemExit("seq_bench needs a gfx950 device")
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows)
    block = rng.standard_normal((CHUNK, a.dim), dtype=np.float32)
    for c, r0 in enumerate(range(0, a.rows, CHUNK)):
        idx.add(np.roll(block, c, axis=1)[:min(CHUNK, a.rows - r0)])
    legs = []
    for L in LS:
        for n_seq in sorted({1, 64 // L, min(64 // L, CAP)}):
            starts = np.sort(rng.choice(a.rows - L, n_seq, replace=False))
            Q = np.concatenate([idx.read(int(s), L) for s in starts])
            Q = (Q + NOISE / np.sqrt(a.dim) * rng.standard_normal(Q.shape, dtype=np.float32)).astype(np.float32)
            ids, _, cnt = idx.search_seq(Q, L, M)
            assert (cnt > 0).all() and ids[:, 0].tolist() == starts.tolist(), ("a sequence did not find its own start", L, n_seq)
            legs.append((L, n_seq, Q))
    Q1 = legs[0][2]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(idx.search(Q1, M), idx.search_seq(Q1, 1, M))), "L = 1, radius 0 differs from bn_index_search"
    t_exact, t_seq = {}, {}
    for rnd in range(a.rounds + 1):
        for L, n_seq, Q in legs:
            t = time.perf_counter()
            idx.search(Q, M)
            te = time.perf_counter() - t
            if rnd:
                t_exact.setdefault((L, n_seq), []).append(te)
            for r in RADII:
                t = time.perf_counter()
                idx.search_seq(Q, L, M, r)
                ts = time.perf_counter() - t
                if rnd:
                    t_seq.setdefault((L, n_seq, r), []).append((ts, te))
    out = {"rows": a.rows, "dim": a.dim, "M": M, "cells": []}
    print("%3s %5s %6s %6s %13s | %28s | %18s | %8s" % ("L", "n_seq", "qrows", "passes", "rows_per_pass", "seq ms median (min-max)", "exact ms", "ratio"))
    for L, n_seq, Q in legs:
        me = med(t_exact[L, n_seq])
        P = min(64 // L, CAP)
        passes = (n_seq + P - 1) // P
        for r in RADII:
            ms = med([x[0] for x in t_seq[L, n_seq, r]])
            ratio = statistics.median(x[0] / x[1] for x in t_seq[L, n_seq, r])
            out["cells"].append({"seq_len": L, "n_seq": n_seq, "query_rows": L * n_seq, "passes": passes, "peak_radius": r, "seq_ms": ms, "exact_ms": me,
                                 "ratio": ratio})
            print("%3d %5d %6d %6d %13.1f | r=%-2d %8.3f (%7.3f-%7.3f) | %8.3f (%7.3f) | %8.4f" % (L, n_seq, L * n_seq, passes, L * n_seq / passes, r, ms[0], ms[1],
                                                                                              ms[2], me[0], me[1], ratio), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
