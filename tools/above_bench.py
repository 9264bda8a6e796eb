#!/usr/bin/env python3
"""Threshold search (bn_index_search_above) against the exact search on one index, in one process.

    python tools/above_bench.py [--rows 1000000] [--dim 1536] [--rounds 7] [--json out.json]

Gaussian rows and Gaussian queries.  For Q in {1, 8, 64, 128}, at max_hits = 4096, three thresholds per query set: +inf (no hit), the
query's own rank-10 score of bn_index_search (a hit rate of 1e-5 on a million rows), and one scalar found by bisection on
bn_index_search_above's count so that the mean hit rate is 1e-3; then the count alone (max_hits = 0) at -inf, where every valid row is a
hit.  Each is timed against bn_index_search at top_m = 100 with the same Q: every round runs every leg once, alternating, so drift hits
all legs alike; the first round is a warm-up and is dropped.  Times are host to host around the C call alone (outputs allocated once,
outside the timed region), in milliseconds as median (min-max); `ratio` is the median over the rounds of above / exact of the same round,
`exact spread` is (max - min) / median of the exact search's own times: a ratio within 1 +- that spread says nothing either way.
`per pass` is the number of queries the budget of above_plan.h leaves a pass at this range and max_hits, `passes` how many passes over the
slab the call therefore makes (the exact search always takes 64 queries per pass).

The lists are checked against bn_index_search's before anything is timed: at the rank-10 threshold the hits are exactly the ten best rows."""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library: it bundles its own HIP runtime, and two copies in one process cannot both see the GPU

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")

QS, M, MAX_HITS = (1, 8, 64, 128), 100, 4096
CHUNK = 32768
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def med(ts):
    ms = [1e3 * t for t in ts]
    return [statistics.median(ms), min(ms), max(ms)]


def per_pass(rows, cus, max_hits):
    """csrc/above_plan.h, plan(): queries per pass"""
    tiles = (rows + 63) // 64
    tpw = (tiles + cus - 1) // cus
    n_wg = (tiles + tpw - 1) // tpw
    per_query = n_wg * min(tpw * 64, max_hits) * 8 + max_hits * 12
    return next((w for w in (64, 48, 32, 16, 8, 4, 2, 1) if w * per_query <= 64 << 20), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if bn.device_count() < 1:
        raise SystemExit("above_bench needs a gfx950 device")
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows)
    block = rng.standard_normal((min(CHUNK, a.rows), a.dim), dtype=np.float32)
    for c, r0 in enumerate(range(0, a.rows, CHUNK)):        # one Gaussian block rotated along k by the chunk number: every row stays Gaussian
        idx.add(np.roll(block, c, axis=1)[:min(CHUNK, a.rows - r0)])
    Qall = rng.standard_normal((max(QS), a.dim), dtype=np.float32)

    # thresholds, and the check against the exact search
    top = idx.search(Qall, 256)
    thr10 = top[1][:, 9].copy()
    ids, sc, _, cnt = idx.search_above(Qall, thr10, 256)
    for q in range(len(Qall)):
        k = int(cnt[q])
        best = np.flatnonzero(top[1][q] >= thr10[q])
        order = best[np.argsort(top[0][q, best], kind="stable")]
        assert 10 <= k < 256 and np.array_equal(ids[q, :k], top[0][q, order]) and sc[q, :k].tobytes() == top[1][q, order].tobytes(), q
    lo, hi = 0.0, float(thr10.min())
    for _ in range(14):                                      # the scalar threshold of a mean hit rate of 1e-3
        mid = 0.5 * (lo + hi)
        if idx.count_above(Qall, mid).mean() > 1e-3 * a.rows:
            lo = mid
        else:
            hi = mid
    thr3 = np.full(len(Qall), hi, dtype=np.float32)
    legs = [("no hit", np.full(len(Qall), np.inf, dtype=np.float32), MAX_HITS), ("rate 1e-5", thr10, MAX_HITS), ("rate 1e-3", thr3, MAX_HITS),
            ("count, -inf", np.full(len(Qall), -np.inf, dtype=np.float32), 0)]
    rates = {name: float(idx.count_above(Qall, thr).mean()) / a.rows for name, thr, _ in legs}

    qmax = max(QS)
    e_ids, e_sc, e_cnt = np.zeros((qmax, M), dtype=np.uint64), np.zeros((qmax, M), dtype=np.float32), np.zeros(qmax, dtype=np.uint32)
    a_ids, a_sc = np.zeros((qmax, MAX_HITS), dtype=np.uint64), np.zeros((qmax, MAX_HITS), dtype=np.float32)
    a_tag, a_cnt = np.zeros((qmax, MAX_HITS), dtype=np.uint32), np.zeros(qmax, dtype=np.uint32)
    qp = Qall.ctypes.data_as(f32p)

    def exact(nq):
        t = time.perf_counter()
        st = bn.lib.bn_index_search(idx._h, qp, nq, M, M, e_ids.ctypes.data_as(u64p), e_sc.ctypes.data_as(f32p), e_cnt.ctypes.data_as(u32p))
        dt = time.perf_counter() - t
        assert st == 0
        return dt

    def above(nq, thr, max_hits):
        t = time.perf_counter()
        st = bn.lib.bn_index_search_above(idx._h, qp, nq, thr.ctypes.data_as(f32p), 0, 0, max_hits, max_hits, a_ids.ctypes.data_as(u64p),
                                          a_sc.ctypes.data_as(f32p), a_tag.ctypes.data_as(u32p), a_cnt.ctypes.data_as(u32p))
        dt = time.perf_counter() - t
        assert st == 0
        return dt

    t_exact, t_above = {}, {}
    for rnd in range(a.rounds + 1):
        for nq in QS:
            for name, thr, max_hits in legs:                 # exact, above, exact, above, ...: each leg next to an exact run of its own
                te = exact(nq)
                ta = above(nq, thr, max_hits)
                if rnd:
                    t_exact.setdefault(nq, []).append(te)
                    t_above.setdefault((nq, name), []).append((ta, te))
    out = {"rows": a.rows, "dim": a.dim, "M": M, "max_hits": MAX_HITS, "cus": cus, "rounds": a.rounds, "rates": rates, "cells": []}
    print("%4s %-12s | %9s | %8s %6s | %28s | %28s | %7s | %12s" % ("Q", "leg", "hit rate", "per pass", "passes", "above ms median (min-max)", "exact ms median (min-max)",
                                                                  "ratio", "exact spread"))
    for nq in QS:
        me = med(t_exact[nq])
        spread = (me[2] - me[1]) / me[0]
        for name, thr, max_hits in legs:
            ma = med([x[0] for x in t_above[nq, name]])
            ratio = statistics.median(x[0] / x[1] for x in t_above[nq, name])
            w = per_pass(a.rows, cus, max_hits)
            passes = (nq + w - 1) // w
            out["cells"].append({"Q": nq, "leg": name, "hit_rate": rates[name], "per_pass": w, "passes": passes, "exact_passes": (nq + 63) // 64, "above_ms": ma,
                                 "exact_ms": me, "ratio": ratio, "exact_spread": spread})
            print("%4d %-12s | %9.2e | %8d %6d | %10.3f (%7.3f-%7.3f) | %10.3f (%7.3f-%7.3f) | %7.3f | %12.3f" %
                  (nq, name, rates[name], w, passes, ma[0], ma[1], ma[2], me[0], me[1], me[2], ratio, spread), flush=True)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
