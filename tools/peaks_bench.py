#!/usr/bin/env python3
"""Event-level search (bn_index_search_peaks) against the exact search on one index, in one process.

    python tools/peaks_bench.py [--rows 1000000] [--dim 1536] [--rounds 5] [--json out.json]

The rows are built as overlapping windows would be: row i is a blend of a slowly changing base (anchors every 8 rows, interpolated
linearly) and noise of its own, so neighbouring rows correlate and a match fills several consecutive ranks of bn_index_search.  The
queries are noisy copies of stored rows.  Times, host to host in milliseconds as median (min-max) over interleaved rounds (every round
runs every leg once, so drift hits all legs alike; the first round is a warm-up and is dropped):

  * for Q in {1, 8, 32, 128} at M = 100: bn_index_search, then bn_index_search_peaks at radius 0, 2, 8 and 64, each with its ratio to
    bn_index_search of the same round;
  * the number of distinct moments per query (median over the queries): ids more than the radius apart, counted along the sorted ids, among
    bn_index_search's top 100, against the count bn_index_search_peaks returns (every one of them a moment of its own).

Radius 0 is checked against bn_index_search's bytes before anything is timed."""
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

QS, M, RADII = (1, 8, 32, 128), 100, (0, 2, 8, 64)
HOP = 8          # rows between two anchors of the base
NOISE = 0.5      # weight of a row's own noise against the base
CHUNK = 32768


def med(ts):
    ms = [1e3 * t for t in ts]
    return [statistics.median(ms), min(ms), max(ms)]


def window_rows(rng, n, dim):
    """chunks (first id, rows) of the correlated rows; the anchor between two chunks is carried over"""
    carry = rng.standard_normal((1, dim), dtype=np.float32)
    for r0 in range(0, n, CHUNK):
        k = min(CHUNK, n - r0)
        anchors = np.concatenate([carry, rng.standard_normal(((k + HOP - 1) // HOP, dim), dtype=np.float32)])
        i = np.arange(k)
        f = ((i % HOP) / HOP).astype(np.float32)[:, None]
        rows = (1 - f) * anchors[i // HOP] + f * anchors[i // HOP + 1] + NOISE * rng.standard_normal((k, dim), dtype=np.float32)
        carry = anchors[-1:]                                # CHUNK is a multiple of HOP: the next chunk starts on this anchor
        yield r0, rows


def moments(ids, radius):
    """ids more than `radius` apart, counted along the sorted ids"""
    n, last = 0, None
    for i in np.sort(ids.astype(np.int64)):
        if last is None or i - last > radius:
            n, last = n + 1, i
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if bn.device_count() < 1:
        raise SystemExit("peaks_bench needs a gfx950 device")
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows)
    picks = np.sort(rng.choice(a.rows, max(QS), replace=False))
    Qall = np.zeros((max(QS), a.dim), dtype=np.float32)
    for r0, rows in window_rows(rng, a.rows, a.dim):
        idx.add(rows)
        mine = picks[(picks >= r0) & (picks < r0 + len(rows))]
        Qall[np.searchsorted(picks, mine)] = rows[mine - r0]
    Qall += NOISE * rng.standard_normal(Qall.shape, dtype=np.float32)
    rng.shuffle(Qall)
    want, got = idx.search(Qall, M), idx.search_peaks(Qall, M, 0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got)), "radius 0 differs from bn_index_search"
    found = {r: idx.search_peaks(Qall, M, r) for r in RADII}
    t_exact, t_peaks = {}, {}
    for rnd in range(a.rounds + 1):
        for nq in QS:
            t = time.perf_counter()
            idx.search(Qall[:nq], M)
            te = time.perf_counter() - t
            if rnd:
                t_exact.setdefault(nq, []).append(te)
            for r in RADII:
                t = time.perf_counter()
                idx.search_peaks(Qall[:nq], M, r)
                tp = time.perf_counter() - t
                if rnd:
                    t_peaks.setdefault((nq, r), []).append((tp, te))
    out = {"rows": a.rows, "dim": a.dim, "M": M, "cells": []}
    print("%4s %6s | %28s | %18s | %8s | %14s | %14s" % ("Q", "radius", "peaks ms median (min-max)", "exact ms", "ratio", "moments, exact", "moments, peaks"))
    for nq in QS:
        me = med(t_exact[nq])
        for r in RADII:
            mp = med([x[0] for x in t_peaks[nq, r]])
            ratio = statistics.median(x[0] / x[1] for x in t_peaks[nq, r])
            m_exact = statistics.median(moments(want[0][q, :want[2][q]], r) for q in range(nq))
            m_peaks = statistics.median(int(found[r][2][q]) for q in range(nq))
            out["cells"].append({"Q": nq, "radius": r, "peaks_ms": mp, "exact_ms": me, "ratio": ratio, "moments_exact": m_exact, "moments_peaks": m_peaks})
            print("%4d %6d | %10.3f (%7.3f-%7.3f) | %8.3f (%7.3f) | %8.4f | %14.1f | %14.1f" % (nq, r, mp[0], mp[1], mp[2], me[0], me[1], ratio, m_exact, m_peaks),
                  flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
