#!/usr/bin/env python3
"""Filtered search (bn_subset_*) against the exact search on one index, in one process.

    python tools/subset_bench.py [--rows 1000000] [--dim 1536] [--rounds 5] [--json out.json]

Random unit rows with a tag drawn per row so that tag 1 marks 10 % and tag 2 marks 1 % of them (spread evenly through the ids: the
gathered scan's worst case, no two members adjacent).  Times, host to host in milliseconds as median (min-max) over interleaved rounds
(every round runs every leg once, so drift hits all legs alike; the first round is a warm-up and is dropped):

  * selection over all rows without a tag list, and with one (10 % and 1 % admitted);
  * for Q in {1, 8, 32, 128} at M = 100: bn_index_search, then bn_subset_search over the subsets of 100 %, 10 % and 1 % of the rows,
    each with its ratio to bn_index_search of the same round and the bandwidth bound subset rows x padded dim x 4 bytes / 6 TB/s.

The 100 % subset's results are checked against bn_index_search's bytes before anything is timed."""
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

QS, M = (1, 8, 32, 128), 100
HBM_BYTES_PER_S = 6e12


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
        raise SystemExit("subset_bench needs a gfx950 device")
    rng = np.random.default_rng(1)
    idx = bn.Index(0, a.dim, a.rows)
    for r0 in range(0, a.rows, 32768):
        idx.add(rng.standard_normal((min(32768, a.rows - r0), a.dim), dtype=np.float32))
    dpad = (a.dim + 127) // 128 * 128
    u = rng.random(a.rows)
    idx.set_tags(0, np.where(u < 0.01, 2, np.where(u < 0.11, 1, 0)).astype(np.uint32))
    selections = {"all rows, no tag list": dict(), "tag list, 10 % admitted": dict(tags=[1]), "tag list, 1 % admitted": dict(tags=[2]),
                  "tag list, 100 % admitted": dict(tags=[0, 1, 2])}
    subsets = {"100 %": bn.Subset.select(idx), "10 %": bn.Subset.select(idx, tags=[1]), "1 %": bn.Subset.select(idx, tags=[2])}
    Qall = rng.standard_normal((max(QS), a.dim), dtype=np.float32)
    want, got = idx.search(Qall, M), subsets["100 %"].search(Qall, M)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(want, got)), "the subset of all rows differs from bn_index_search"
    t_sel, t_exact, t_sub = {}, {}, {}
    for rnd in range(a.rounds + 1):
        for name, kw in selections.items():
            t = time.perf_counter()
            s = bn.Subset.select(idx, **kw)
            dt = time.perf_counter() - t
            s.close()
            if rnd:
                t_sel.setdefault(name, []).append(dt)
        for nq in QS:
            t = time.perf_counter()
            idx.search(Qall[:nq], M)
            te = time.perf_counter() - t
            if rnd:
                t_exact.setdefault(nq, []).append(te)
            for name, s in subsets.items():
                t = time.perf_counter()
                s.search(Qall[:nq], M)
                ts = time.perf_counter() - t
                if rnd:
                    t_sub.setdefault((nq, name), []).append((ts, te))
    out = {"rows": a.rows, "dim": a.dim, "M": M, "selection": [], "cells": []}
    print("%-26s | %28s" % ("selection", "ms median (min-max)"))
    for name in selections:
        m = med(t_sel[name])
        out["selection"].append({"filter": name, "ms": m})
        print("%-26s | %10.3f (%7.3f-%7.3f)" % (name, m[0], m[1], m[2]), flush=True)
    print("%4s %6s %9s | %28s | %18s | %8s | %8s" % ("Q", "subset", "rows", "subset ms median (min-max)", "exact ms", "ratio", "bound ms"))
    for nq in QS:
        me = med(t_exact[nq])
        for name, s in subsets.items():
            ms = med([x[0] for x in t_sub[nq, name]])
            ratio = statistics.median(x[0] / x[1] for x in t_sub[nq, name])
            passes = (nq + 63) // 64                        # every pass of 64 queries reads the subset's rows once
            bound = passes * len(s) * dpad * 4 / HBM_BYTES_PER_S * 1e3
            out["cells"].append({"Q": nq, "subset": name, "rows": len(s), "subset_ms": ms, "exact_ms": me, "ratio": ratio, "bound_ms": bound})
            print("%4d %6s %9d | %10.3f (%7.3f-%7.3f) | %8.3f (%7.3f) | %8.4f | %8.4f" % (nq, name, len(s), ms[0], ms[1], ms[2], me[0], me[1], ratio, bound),
                  flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
