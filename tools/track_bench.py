#!/usr/bin/env python3
"""What an attached detection-event tracker costs per step (the library only: no oracle, no reference).

    python tools/track_bench.py [--batch 32] [--contexts 4] [--sources 1024] [--rounds 12] [--steps-only N]

Full-width BirdNET v2.4 synth.  Two measurements, each with the cases (nothing attached, tracker, SELECT prior, prior + tracker under
BN_TRACK_PRIOR) interleaved round by round in one process, so clock and thermal drift hit all of them alike; median and minimum per
case over the rounds:

  pool    `contexts` contexts stepping a live pool of `sources` sources, one tracker of sources x num_species records shared by all
          of them: every round pushes one window per source and the contexts take the ready windows round robin, sync = 0, each
          context's previous step collected (its events read) before it steps again; wall time per step of `batch` windows.  Every
          case has a pool of its own, so that its tracker sees consecutive windows, and the pushed audio changes kind every three
          rounds (noise / tones), so that events open, span windows, close and are emitted inside the timed rounds: the emission
          path (ballot, atomic, pinned event store, host sort) is part of the figure, and events_read_pool says how much of it.
  single  one context, synchronous bn_step_windows over a recording at a step of one sample (so that the window numbers can go on
          increasing): the difference to the bare case is what the tracker's two launches add to one step's latency.

enter_conf is the (1 - hit_fraction) quantile of the confidences of one batch: by default about 13 of the 6522 species hit per
window, a station's load rather than the tests' fifth.  The baseline `none` is this build with nothing attached.

--steps-only N runs N tracked steps and prints nothing else: the process to put under `rocprofv3 --kernel-trace --stats`, which then
lists track_update_kernel (the update alone, `batch` rows x num_species) next to the step's own top-K kernel.  Without --pool the
steps are one context's bn_step_windows (all `batch` rows of ONE source: one group, every lane walks `batch` rows); with --pool they
are bn_step_live steps of a pool (`batch` sources, one row each).  One JSON line."""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--pool", action="store_true", help="with --steps-only: steps of a live pool instead of one recording")
    ap.add_argument("--hit-fraction", type=float, default=0.002)
    args = ap.parse_args()
    with tempfile.NamedTemporaryFile(suffix=".onnx", delete=False) as f:
        f.write(synth.birdnet_v24())
    try:
        model = bn.Model(f.name)
    finally:
        os.unlink(f.name)
    cfg = model.config
    S, sr, n, B = int(cfg.sample_count), int(cfg.sample_rate), int(cfg.num_species), args.batch
    rng = np.random.default_rng(0)
    cases = ("none", "track", "prior", "prior_track")
    n_single = (args.rounds + 3) * (args.inner + 1) * B * 2 + max(args.steps_only, 1) * B   # windows a tracked case of `single` walks through
    rec = bn.Recording(np.clip(synth.synthetic_segments(1, S + n_single, sr)[0], -1, 1).astype(np.float32))
    ctxs = [bn.Context(model, B) for _ in range(args.contexts)]
    for c in ctxs:  # capture the batch's graph outside the timings
        c.step_windows(rec, 1, 0, B, args.top_k, None, sync=True)
    one = ctxs[0]
    conf = 1.0 / (1.0 + np.exp(-one.step_results(B)[0].astype(np.float64)))
    enter = float(np.quantile(conf, 1.0 - args.hit_fraction))
    table = rng.uniform(0, 1, (args.sources, n)).astype(np.float32)
    table[rng.uniform(size=table.shape) < 0.1] = bn.BN_PRIOR_UNKNOWN
    prior = bn.Prior(0, table, 0.5)
    site_map = np.arange(args.sources, dtype=np.int32)

    def trackers(n_sources):
        return {"none": None, "track": bn.Tracker(0, n_sources, n, enter, 2, 1), "prior": None,
                "prior_track": bn.Tracker(0, n_sources, n, enter, 2, 1, use_prior=True)}

    def attach(c, name, trk, with_map):
        c.attach_prior(prior if name.startswith("prior") else None, source_sites=site_map if with_map else None, top_k=args.top_k)
        c.attach_track(trk[name])

    trk = trackers(1)
    first = {k: 0 for k in cases}

    def single_step(name):
        one.step_windows(rec, 1, first[name], B, args.top_k, None, sync=True)
        first[name] += B

    # the pool's audio: one block per kind, every source reads it at an offset of its own
    noise = rng.integers(-32768, 32768, size=2 * S).astype(np.int16)
    tones = (np.clip(synth.synthetic_segments(1, 2 * S, sr)[0], -1, 1) * 32767).astype(np.int16)
    srcs = list(range(args.sources))

    def push_round(live, r):
        block = (noise, tones)[(r // 3) % 2]
        live.push_many(srcs, [block[(s * 997 + r * 131) % S:][:S] for s in srcs])

    def new_pool():
        return bn.Live(0, args.sources, S, S, 2 * S + S, bn.BN_PCM_I16)

    if args.steps_only and not args.pool:
        attach(one, "track", trk, False)
        for _ in range(args.steps_only):
            single_step("track")
        return
    if args.steps_only:
        trk, live, r, done = trackers(args.sources), new_pool(), 0, 0
        attach(one, "track", trk, True)
        while done < args.steps_only:
            push_round(live, r)
            r += 1
            while live.ready(-1) and done < args.steps_only:
                one.step_live(live, B, args.top_k, None, sync=True)
                done += 1
        return

    # ---- single context, synchronous
    single = {k: [] for k in cases}
    for r in range(args.rounds + 3):
        for name in cases:
            attach(one, name, trk, False)
            single_step(name)
            t0 = time.perf_counter()
            for _ in range(args.inner):
                single_step(name)
            if r >= 3:
                single[name].append((time.perf_counter() - t0) / args.inner * 1e6)
    open_single = {k: v.open_events() for k, v in trk.items() if v is not None}

    # ---- the pool
    trk = trackers(args.sources)
    lives = {k: new_pool() for k in cases}
    pool = {k: [] for k in cases}
    events = {k: 0 for k in cases}
    dropped = {k: 0 for k in cases}
    for r in range(args.rounds + 2):
        for name in cases:
            for c in ctxs:
                attach(c, name, trk, True)
            live = lives[name]
            push_round(live, r)
            pending = [False] * len(ctxs)
            steps, turn = 0, 0
            t0 = time.perf_counter()
            while live.ready(-1):
                i = turn % len(ctxs)
                turn += 1
                if pending[i]:
                    ctxs[i].synchronize()
                    if trk[name] is not None:
                        ev, lost, _ = ctxs[i].step_track_results()
                        events[name] += len(ev)
                        dropped[name] += lost
                src, _ = ctxs[i].step_live(live, B, args.top_k, None, sync=False)
                pending[i] = len(src) > 0
                steps += 1 if len(src) else 0
            for i, c in enumerate(ctxs):
                c.synchronize()
                if pending[i] and trk[name] is not None:
                    ev, lost, _ = c.step_track_results()
                    events[name] += len(ev)
                    dropped[name] += lost
            if r >= 2 and steps:
                pool[name].append((time.perf_counter() - t0) / steps * 1e6)

    def summary(t):
        return {k: {"median": round(float(np.median(v)), 2), "min": round(float(np.min(v)), 2), "max": round(float(np.max(v)), 2)} for k, v in t.items()}

    out = {"model": "v24", "num_species": n, "batch": B, "contexts": args.contexts, "sources": args.sources, "top_k": args.top_k,
           "rounds": args.rounds, "enter_conf": round(enter, 6), "state_mb": round(6 * 4 * args.sources * n / 1e6, 1),
           "single_step_us": summary(single), "pool_step_us": summary(pool), "open_events_single": open_single,
           "open_events_pool": {k: v.open_events() for k, v in trk.items() if v is not None}, "events_read_pool": events, "events_dropped_pool": dropped, "hit_fraction": args.hit_fraction,
           "capture_fallbacks": sum(c.stats()["capture_fallbacks"] for c in ctxs)}
    for key in ("single_step_us", "pool_step_us"):
        m = {k: v["median"] for k, v in out[key].items()}
        out[key.replace("step_us", "added_us")] = {"track": round(m["track"] - m["none"], 2), "prior": round(m["prior"] - m["none"], 2),
                                                   "track_behind_prior": round(m["prior_track"] - m["prior"], 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
