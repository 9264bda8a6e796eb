"""Live ingest measurement (bn_live_*, bn_step_live): N i16 sources at the model's rate, each tick one push_many of `chunk_s`
seconds per source, four contexts of batch B stepping the shared pool round robin (sync = 0, each context's previous step
collected before it steps again).  Reports segments/s, the time from the push that made a window ready to its results being
collected (mean, p99: an upper bound on "readable", since a context is synchronised only when the round robin comes back to
it), and host time per push_many; then, in the same process, four contexts running bn_step_windows over one
recording of the same number of windows.  One JSON line per run.

With --src-rate R[,R...] the pool is a resampling one (bn_live_create_rates): source s delivers i16 at the (s mod n)-th rate and
every tick pushes `chunk_s` seconds at that rate; the same process then also runs a plain pool at the model's rate through the
same loop ("plain_*" in the JSON line), so that the two are compared under one clock state.

    python tools/live_bench.py [--sources 1024] [--ticks 12] [--batch 32] [--contexts 4] [--scatter direct|copy]
                               [--model v24|v30] [--src-rate 48000[,44100...]]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=1024)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--chunk-s", type=float, default=1.0)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--top-k", type=int, default=5)
    ap.add_argument("--scatter", choices=["direct", "copy"], default="direct")
    ap.add_argument("--width", type=float, default=1.0)
    ap.add_argument("--model", choices=["v24", "v30"], default="v24")
    ap.add_argument("--src-rate", default="", help="comma-separated source rates, assigned round robin: a resampling pool")
    a = ap.parse_args()
    os.environ["BN_LIVE_SCATTER"] = a.scatter  # read when the pool is created
    bn = importlib.import_module("rust-birdnet-onnx_amd")
    synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
    with tempfile.NamedTemporaryFile(suffix=".onnx", delete=False) as f:
        f.write(synth.birdnet_v24(width=a.width) if a.model == "v24" else synth.birdnet_v30(width=a.width))
        path = f.name
    model = bn.Model(path)
    os.unlink(path)
    S, rate = model.config.sample_count, model.config.sample_rate
    step = S
    src_rates = [int(r) for r in a.src_rate.split(",") if r]
    ctxs = [bn.Context(model, a.batch) for _ in range(a.contexts)]
    rng = np.random.RandomState(0)
    max_chunk = int(a.chunk_s * max(src_rates + [rate]))
    block = rng.randint(-32768, 32768, size=max_chunk * 4).astype(np.int16)  # each source's tick reads a rotating slice of it

    # warm-up: capture the graphs of every batch size a step may take
    zeros = bn.Recording(np.zeros(a.batch * S, dtype=np.int16))
    for c in ctxs:
        for b in range(1, a.batch + 1):
            c.step_windows(zeros, S, 0, b, a.top_k, None, sync=True)

    srcs = list(range(a.sources))

    def run(live, chunk_of):
        """the tick loop over one pool; chunk_of[s]: samples source s pushes per tick"""
        ready_t = []  # time each window (by sequence number) became ready
        seq_taken = 0
        lat = []
        pending = [None] * a.contexts
        push_t = []
        done = 0
        turn = 0

        def collect(i):
            nonlocal done
            if pending[i] is None:
                return
            ctxs[i].synchronize()
            now = time.perf_counter()
            first, n = pending[i]
            lat.extend(now - ready_t[first + j] for j in range(n))
            done += n
            pending[i] = None

        t0 = time.perf_counter()
        for t in range(a.ticks):
            chunks = [block[(s * 997 + t * chunk_of[s]) % (3 * max_chunk):][:chunk_of[s]] for s in srcs]
            before = live.ready(-1)
            p0 = time.perf_counter()
            live.push_many(srcs, chunks)
            p1 = time.perf_counter()
            push_t.append(p1 - p0)
            ready_t.extend([p1] * (live.ready(-1) - before))
            while live.ready(-1):
                i = turn % a.contexts
                turn += 1
                collect(i)
                src, _ = ctxs[i].step_live(live, a.batch, a.top_k, None, sync=False)
                pending[i] = (seq_taken, len(src))
                seq_taken += len(src)
        for i in range(a.contexts):
            collect(i)
        elapsed = time.perf_counter() - t0
        lat_ms = np.array(lat) * 1e3
        return {"windows": done, "segments_per_s": done / elapsed, "latency_ms_mean": round(float(lat_ms.mean()), 3),
                "latency_ms_p99": round(float(np.percentile(lat_ms, 99)), 3), "push_many_ms_mean": round(float(np.mean(push_t)) * 1e3, 3),
                "push_many_ms_max": round(float(np.max(push_t)) * 1e3, 3)}

    plain = None
    if src_rates:
        rates = [src_rates[s % len(src_rates)] for s in srcs]
        live = bn.Live(0, a.sources, S, step, 2 * S + step + 4096, bn.BN_PCM_I16, dst_rate=rate, src_rates=rates)
        res = run(live, [int(a.chunk_s * r) for r in rates])
        live.free()
        plain = run(bn.Live(0, a.sources, S, step, 2 * S + step, bn.BN_PCM_I16), [int(a.chunk_s * rate)] * a.sources)
    else:
        res = run(bn.Live(0, a.sources, S, step, 2 * S + step, bn.BN_PCM_I16), [int(a.chunk_s * rate)] * a.sources)
    done, live_rate = res["windows"], res["segments_per_s"]

    # the recording path on the same number of windows
    n_win = done
    rec = bn.Recording(rng.randint(-32768, 32768, size=n_win * S).astype(np.int16))
    for c in ctxs:
        c.synchronize()
    t0 = time.perf_counter()
    issued = [0] * a.contexts
    f = 0
    turn = 0
    while f < n_win:
        i = turn % a.contexts
        turn += 1
        if issued[i]:
            ctxs[i].synchronize()
        m = min(a.batch, n_win - f)
        ctxs[i].step_windows(rec, step, f, m, a.top_k, None, sync=False)
        issued[i] = m
        f += m
    for c in ctxs:
        c.synchronize()
    rec_rate = n_win / (time.perf_counter() - t0)
    out = {
        "model": a.model, "src_rates": src_rates, "sources": a.sources, "ticks": a.ticks, "chunk_s": a.chunk_s, "batch": a.batch,
        "contexts": a.contexts, "scatter": a.scatter,
        "windows": done, "live_segments_per_s": round(live_rate, 1), "recording_segments_per_s": round(rec_rate, 1),
        "live_vs_recording": round(live_rate / rec_rate, 4),
        "latency_ms_mean": res["latency_ms_mean"], "latency_ms_p99": res["latency_ms_p99"],
        "push_many_ms_mean": res["push_many_ms_mean"], "push_many_ms_max": res["push_many_ms_max"],
    }
    if plain:
        out.update({"plain_windows": plain["windows"], "plain_live_segments_per_s": round(plain["segments_per_s"], 1),
                    "plain_push_many_ms_mean": plain["push_many_ms_mean"], "plain_push_many_ms_max": plain["push_many_ms_max"],
                    "resampled_vs_plain": round(live_rate / plain["segments_per_s"], 4)})
    out["capture_fallbacks"] = sum(c.stats()["capture_fallbacks"] for c in ctxs)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
