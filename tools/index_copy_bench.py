#!/usr/bin/env python3
"""bn_index_append_rows / bn_index_append_subset against a plain device-to-device copy and against the routes they replace, in one process.

    python tools/index_copy_bench.py [--rows 1000000] [--dim 1536] [--rounds 5] [--dir /tmp] [--no-old] [--json out.json]
    python tools/index_copy_bench.py --trace     # one range copy and one 50 % subset copy and nothing else, for `rocprofv3 --kernel-trace -- python ...`

Every round runs, in this order: (a) bn_index_append_rows of everything into a fresh index, (b) bn_index_append_subset of 100 %, 50 %
(every other row), 10 % and 1 % of the rows, (c) hipMemcpyAsync device to device of the same slab bytes (rows x dim padded to a multiple
of 128, x 4) on a non-blocking stream of its own, as the index's is, and (d) the old routes: bn_index_read + bn_index_add_host, and
bn_index_save + bn_index_load into a fresh index.  The first round is a warm-up and is dropped; the rest give median (min-max) GB/s of
row bytes MOVED, read plus write: 2 x rows copied x padded row bytes (the valid bytes, tags and ids are under 1 % and not counted; the
old routes move the same rows, so they are counted the same way).  Times are host clocks around calls that end in a stream wait.  Every
destination index is created outside the timer, except that of bn_index_load, which creates (and zeroes) its own: that leg pays for it."""
import argparse
import ctypes as C
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

import torch  # noqa: F401  (before the library: two HIP runtimes in one process, torch's must come first)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
bn = importlib.import_module("rust-birdnet-onnx_amd")

D2D, NON_BLOCKING = 3, 1  # hipMemcpyDeviceToDevice, hipStreamNonBlocking


def hip_runtime():
    """the HIP runtime the library itself calls: a lookup through the library's handle searches the library and what it links against,
    so the yardstick's stream and copy live in the runtime instance that owns the indexes' streams, whatever else the process has loaded"""
    return C.CDLL(bn.LIB_PATH)


class PlainCopy:
    """two device buffers of n bytes and a stream: hipMemcpyAsync + hipStreamSynchronize"""

    def __init__(self, nbytes):
        self.hip, self.n = hip_runtime(), nbytes
        self.src, self.dst, self.stream = C.c_void_p(), C.c_void_p(), C.c_void_p()
        for p in (self.src, self.dst):
            self.ok(self.hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
            self.ok(self.hip.hipMemset(p, 1, C.c_size_t(nbytes)))
        self.ok(self.hip.hipStreamCreateWithFlags(C.byref(self.stream), NON_BLOCKING))
        self.ok(self.hip.hipDeviceSynchronize())

    @staticmethod
    def ok(e):
        if e:
            raise SystemExit(f"HIP runtime call failed with {e}")

    def run(self):
        self.ok(self.hip.hipMemcpyAsync(self.dst, self.src, C.c_size_t(self.n), D2D, self.stream))
        self.ok(self.hip.hipStreamSynchronize(self.stream))

    def close(self):
        self.hip.hipFree(self.src)
        self.hip.hipFree(self.dst)
        self.hip.hipStreamDestroy(self.stream)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--no-old", action="store_true", help="leave the old routes out")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if bn.device_count() < 1:
        raise SystemExit("index_copy_bench needs a gfx950 device")
    rows, dim = a.rows, a.dim
    dpad = (dim + 127) // 128 * 128
    row_bytes = dpad * 4
    rng = np.random.default_rng(1)
    block = rng.standard_normal((min(rows, 32768), dim), dtype=np.float32)   # the copy does not look at the values: one block, repeated
    src = bn.Index(0, dim, rows)
    for r0 in range(0, rows, len(block)):
        src.add(block[:min(len(block), rows - r0)])
    src.set_tags(0, (np.arange(rows) % 1000).astype(np.uint32))
    shares = {"100%": 1, "50%": 2, "10%": 10, "1%": 100}
    subsets = {k: bn.Subset.from_ids(src, np.arange(0, rows, s)) for k, s in shares.items()}

    def copy_range():
        dst = bn.Index(0, dim, rows)
        t, _ = timed(lambda: dst.append_rows(src))
        return t, dst

    def copy_subset(k):
        dst = bn.Index(0, dim, len(subsets[k]))
        t, _ = timed(lambda: dst.append_subset(subsets[k]))
        return t, dst

    if a.trace:
        copy_range()[1].close()
        copy_subset("50%")[1].close()
        return
    print(f"{rows} x {dim} f32, padded rows of {row_bytes} bytes: {rows * row_bytes / 1e9:.2f} GB of slab")
    plain = PlainCopy(rows * row_bytes)
    work = tempfile.mkdtemp(prefix="bn_index_copy_", dir=a.dir)
    legs = ["rows", *("subset " + k for k in shares), "memcpy"]
    old_file = os.path.join(work, "old.bnindex")
    with_file = not a.no_old and shutil.disk_usage(work).free > 1.2 * rows * dim * 4
    if not a.no_old:
        legs += ["read+add_host"] + (["save+load"] if with_file else [])
    times = {k: [] for k in legs}
    moved = {k: 2 * rows * row_bytes for k in legs}
    for k in shares:
        moved["subset " + k] = 2 * len(subsets[k]) * row_bytes
    try:
        for rnd in range(a.rounds + 1):
            got = {}
            got["rows"], dst = copy_range()
            if rnd == 0:
                assert len(dst) == rows and dst.read(rows - 3, 3).tobytes() == src.read(rows - 3, 3).tobytes() and dst.tags(rows - 3, 3).tolist() == src.tags(rows - 3, 3).tolist()
            dst.close()
            for k in shares:
                got["subset " + k], dst = copy_subset(k)
                if rnd == 0:
                    last = int(subsets[k].ids[-1])
                    assert len(dst) == len(subsets[k]), (k, len(dst))
                    assert dst.read(len(dst) - 1, 1).tobytes() == src.read(last, 1).tobytes() and dst.read(0, 1).tobytes() == src.read(0, 1).tobytes(), (k, "rows")
                    assert dst.tags(len(dst) - 1, 1)[0] == last % 1000, (k, "tags", dst.tags(len(dst) - 1, 1))
                dst.close()
            got["memcpy"], _ = timed(plain.run)
            if not a.no_old:
                y = bn.Index(0, dim, rows)                # created outside the timer, as the new calls' destinations are
                got["read+add_host"], _ = timed(lambda: y.add(src.read()))
                y.close()
                if with_file:
                    def through_file():
                        src.save(old_file)
                        return bn.Index.load(old_file, capacity_rows=rows)

                    got["save+load"], y = timed(through_file)
                    y.close()
            if rnd:
                for k in legs:
                    times[k].append(got[k])
    finally:
        plain.close()
        shutil.rmtree(work, ignore_errors=True)
    rate = {k: sorted(moved[k] / t / 1e9 for t in v) for k, v in times.items()}
    med = {k: statistics.median(v) for k, v in rate.items()}
    for k in legs:
        print(f"  {k:14s} {med[k]:9.1f} GB/s  ({rate[k][0]:.1f}-{rate[k][-1]:.1f})   {statistics.median(times[k]) * 1e3:10.2f} ms")
    print(f"  append_rows is {med['rows'] / med['memcpy']:.2f} of the plain copy, append_subset of every row {med['subset 100%'] / med['memcpy']:.2f}")
    if not a.no_old and not with_file:
        print(f"  save+load: not measured (no room for the file in {a.dir})")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"rows": rows, "dim": dim, "row_bytes": row_bytes, "rounds": a.rounds, "gbps": rate, "median_gbps": med,
                       "median_ms": {k: statistics.median(v) * 1e3 for k, v in times.items()}}, f, indent=1)


if __name__ == "__main__":
    main()
