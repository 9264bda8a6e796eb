#!/usr/bin/env python3
"""Grouped threshold search (bn_index_group_above) against the count alone (bn_index_search_above, max_hits = 0) on one index, in one
process.

    python tools/group_bench.py [--rows 1000000] [--dim 1536] [--rounds 7] [--json out.json]

Gaussian rows and Gaussian queries.  For Q in {1, 8, 64, 128}, n_groups in {1, 256, 65536}, two tag planes -- contiguous runs (row i has
tag i * n_groups // rows: one recorder after the other) and random tags below n_groups -- and three thresholds per query set: +inf (no
hit), one scalar found by bisection on the count so that the mean hit rate is 1e-3, and -inf (every valid row is a hit).  With
n_groups = 1 the two planes are the same, so that cell is run once ("one group").  Each leg alternates with the count for the same
queries and thresholds: every round runs every leg once, count then group, so drift hits both alike; the first round is a warm-up and is
dropped.  Times are host to host around the C call alone (outputs allocated once, outside the timed region; all seven outputs asked
for), in milliseconds as median (min-max); `ratio` is the median over the rounds of group / count of the same round, `count spread` is
(max - min) / median of the count's own times in that cell: a ratio within 1 +- that spread says nothing either way.  `per pass` is the
number of queries group_plan.h leaves a pass (the count always takes 64).

Before anything is timed the grouped totals are checked against the count, and the records of a few queries against the lists of
bn_index_search_above where they fit."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # noqa: F401  before the library: it bundles its own HIP runtime, and two copies in one process cannot both see the GPU

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")

QS, GROUPS = (1, 8, 64, 128), (1, 256, 65536)
CHUNK = 32768
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def med(ts):
    ms = [1e3 * t for t in ts]
    return [statistics.median(ms), min(ms), max(ms)]


def per_pass(n_groups):
    """csrc/group_plan.h, plan(): queries per pass"""
    return next(w for w in (64, 48, 32, 16, 8, 4, 2, 1) if w * n_groups * 20 <= 64 << 20)


def check(idx, Q, thr, n_groups, tags):
    """totals against the count; the records of the first queries against the threshold search's lists"""
    got = idx.group_above(Q, thr, n_groups)
    assert np.array_equal(got[6], idx.count_above(Q, thr)) and np.array_equal(got[0].sum(axis=1, dtype=np.uint64) + got[5], got[6])
    ids, sc, tg, cnt = idx.search_above(Q[:4], thr[:4], 65536)
    for q in range(min(4, len(Q))):
        if cnt[q] > 65536:
            continue
        i, s = ids[q, :cnt[q]].astype(np.int64), sc[q, :cnt[q]]
        t = tags[i].astype(np.int64)
        assert np.array_equal(t, tg[q, :cnt[q]]) and np.array_equal(np.bincount(t, minlength=n_groups), got[0][q])
        for g in np.unique(t)[:50]:
            m = t == g
            best = i[m][np.lexsort((i[m], -s[m].astype(np.float64)))[0]]
            assert got[1][q, g] == best and got[3][q, g] == i[m][0] and got[4][q, g] == i[m][-1] and got[2][q, g] == s[m].max(), (q, g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if bn.device_count() < 1:
        raise SystemExit("group_bench needs a gfx950 device")
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows)
    block = rng.standard_normal((min(CHUNK, a.rows), a.dim), dtype=np.float32)
    for c, r0 in enumerate(range(0, a.rows, CHUNK)):        # one Gaussian block rotated along k by the chunk number: every row stays Gaussian
        idx.add(np.roll(block, c, axis=1)[:min(CHUNK, a.rows - r0)])
    qmax = max(QS)
    Qall = rng.standard_normal((qmax, a.dim), dtype=np.float32)
    lo, hi = 0.0, 1.0
    for _ in range(20):                                      # the scalar threshold of a mean hit rate of 1e-3
        mid = 0.5 * (lo + hi)
        if idx.count_above(Qall, mid).mean() > 1e-3 * a.rows:
            lo = mid
        else:
            hi = mid
    thresholds = [("no hit", np.full(qmax, np.inf, dtype=np.float32)), ("rate 1e-3", np.full(qmax, hi, dtype=np.float32)),
                  ("every row", np.full(qmax, -np.inf, dtype=np.float32))]
    rates = {name: float(idx.count_above(Qall, thr).mean()) / a.rows for name, thr in thresholds}

    qp = Qall.ctypes.data_as(f32p)
    c_cnt = np.zeros(qmax, dtype=np.uint32)

    def count(nq, thr):
        t = time.perf_counter()
        st = bn.lib.bn_index_search_above(idx._h, qp, nq, thr.ctypes.data_as(f32p), 0, 0, 0, 0, None, None, None, c_cnt.ctypes.data_as(u32p))
        dt = time.perf_counter() - t
        assert st == 0
        return dt

    out = {"rows": a.rows, "dim": a.dim, "rounds": a.rounds, "rates": rates, "cells": []}
    print("%4s %8s %-10s %-10s | %9s | %8s | %28s | %28s | %7s | %12s" % ("Q", "n_groups", "tags", "leg", "hit rate", "per pass", "group ms median (min-max)",
                                                                         "count ms median (min-max)", "ratio", "count spread"))
    for n_groups in GROUPS:
        o = [np.zeros((qmax, n_groups), dtype=np.uint32), np.zeros((qmax, n_groups), dtype=np.uint64), np.zeros((qmax, n_groups), dtype=np.float32),
             np.zeros((qmax, n_groups), dtype=np.uint64), np.zeros((qmax, n_groups), dtype=np.uint64), np.zeros(qmax, dtype=np.uint32),
             np.zeros(qmax, dtype=np.uint32)]
        ptrs = [x.ctypes.data_as(t) for x, t in zip(o, (u32p, u64p, f32p, u64p, u64p, u32p, u32p))]

        def group(nq, thr):
            t = time.perf_counter()
            st = bn.lib.bn_index_group_above(idx._h, qp, nq, thr.ctypes.data_as(f32p), 0, 0, n_groups, n_groups, *ptrs)
            dt = time.perf_counter() - t
            assert st == 0
            return dt

        planes = [("one group", np.zeros(a.rows, dtype=np.uint32))] if n_groups == 1 else \
            [("runs", (np.arange(a.rows, dtype=np.int64) * n_groups // a.rows).astype(np.uint32)), ("random", rng.integers(0, n_groups, a.rows).astype(np.uint32))]
        for plane, tags in planes:
            idx.set_tags(0, tags)
            check(idx, Qall[:8], thresholds[1][1][:8], n_groups, tags)
            times = {}
            for rnd in range(a.rounds + 1):
                for nq in QS:
                    for name, thr in thresholds:
                        tc = count(nq, thr)
                        tg = group(nq, thr)
                        if rnd:
                            times.setdefault((nq, name), []).append((tg, tc))
            for nq in QS:
                for name, thr in thresholds:
                    ts = times[nq, name]
                    mg, mc = med([x[0] for x in ts]), med([x[1] for x in ts])
                    ratio = statistics.median(x[0] / x[1] for x in ts)
                    spread = (mc[2] - mc[1]) / mc[0]
                    out["cells"].append({"Q": nq, "n_groups": n_groups, "tags": plane, "leg": name, "hit_rate": rates[name], "per_pass": per_pass(n_groups),
                                         "group_ms": mg, "count_ms": mc, "ratio": ratio, "count_spread": spread})
                    print("%4d %8d %-10s %-10s | %9.2e | %8d | %10.3f (%7.3f-%7.3f) | %10.3f (%7.3f-%7.3f) | %7.3f | %12.3f" %
                          (nq, n_groups, plane, name, rates[name], per_pass(n_groups), mg[0], mg[1], mg[2], mc[0], mc[1], mc[2], ratio, spread), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
