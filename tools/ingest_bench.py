#!/usr/bin/env python3
"""Ingest of a layout recording against host-side conversion: bn_step_windows over every window of a long recording whose
bytes are interleaved multi-channel PCM (include/birdnet_hip.h, "PCM layouts"), uploaded asynchronously in their storage
format and converted on the device -- against the same analysis after deinterleaving, converting and mixing in numpy on the
host and uploading mono f32.  The mono int16 rate of the same build is reported beside them.

    python tools/ingest_bench.py --hours 24 --layout i24x2:mix
    python tools/ingest_bench.py --hours 1 --layout u8x4:2 --contexts 4 --batch 32

Layout: <format>x<channels>:<channel | mix>, format one of i16 f32 i24 i32 u8.  The recording is one minute of noise repeated
(the network's time does not depend on the samples), built in host memory: 24 h of i24x2 are 24.9 GB.  Prints one JSON line."""
from __future__ import annotations

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

FORMATS = {"i16": bn.BN_PCM_I16, "f32": bn.BN_PCM_F32, "i24": bn.BN_PCM_I24, "i32": bn.BN_PCM_I32, "u8": bn.BN_PCM_U8}
RATE, SEG = 48000, 144000


def parse_layout(text):
    fmt, rest = text.split("x", 1)  # "mix" has an x of its own
    ch, op = rest.split(":", 1)
    return FORMATS[fmt], int(ch), (bn.BN_PCM_MIX if op == "mix" else int(op))


def minute_of(fmt, channels, rng):
    """one minute of interleaved frames as storage bytes (uint8 array)"""
    n = 60 * RATE * channels
    if fmt == bn.BN_PCM_F32:
        return rng.uniform(-1, 1, n).astype("<f4").view(np.uint8)
    if fmt == bn.BN_PCM_I16:
        return rng.randint(-32768, 32768, n).astype("<i2").view(np.uint8)
    if fmt == bn.BN_PCM_I32:
        return rng.randint(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype("<i4").view(np.uint8)
    if fmt == bn.BN_PCM_U8:
        return rng.randint(0, 256, n).astype(np.uint8)
    return rng.randint(0, 256, 3 * n).astype(np.uint8)  # any three bytes are a 24-bit sample


def host_convert(raw, fmt, channels, channel):
    """what a caller does today in front of the mono f32 path: the layout rule in numpy, f32 [n_frames]"""
    if fmt == bn.BN_PCM_F32:
        s = raw.view("<f4")
    elif fmt == bn.BN_PCM_I16:
        s = raw.view("<i2").astype(np.float32) / np.float32(32768)
    elif fmt == bn.BN_PCM_I32:
        s = raw.view("<i4").astype(np.float32) * np.float32(2.0 ** -31)
    elif fmt == bn.BN_PCM_U8:
        s = (raw.astype(np.int16) - 128).astype(np.float32) / np.float32(128)
    else:
        t = raw.reshape(-1, 3)
        v = t[:, 0].astype(np.int32) | (t[:, 1].astype(np.int32) << 8) | (t[:, 2].astype(np.int8).astype(np.int32) << 16)
        s = v.astype(np.float32) / np.float32(8388608)
    s = s.reshape(-1, channels)
    if channels == 1 or channel >= 0:
        return np.ascontiguousarray(s[:, max(channel, 0)])
    acc = s[:, 0].copy()
    for c in range(1, channels):
        acc += s[:, c]
    return acc * (np.float32(1) / np.float32(channels))


def analyse(ctxs, rec, batch, top_k):
    """every window of rec through the contexts in rotation; returns the windows stepped"""
    g, i = rec.n_windows(SEG), 0
    for first in range(0, g, batch):
        c = ctxs[i % len(ctxs)]
        i += 1
        c.synchronize()
        c.step_windows(rec, SEG, first, min(batch, g - first), top_k, None, sync=False)
    for c in ctxs:
        c.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hours", type=float, default=24.0)
    ap.add_argument("--layout", default="i24x2:mix")
    ap.add_argument("--contexts", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=10)
    a = ap.parse_args()
    fmt, channels, channel = parse_layout(a.layout)
    rng = np.random.RandomState(0)
    minutes = max(1, int(round(a.hours * 60)))
    raw = np.tile(minute_of(fmt, channels, rng), minutes)
    mono16 = np.tile(rng.randint(-32768, 32768, 60 * RATE).astype(np.int16), minutes)
    with tempfile.NamedTemporaryFile(suffix=".onnx", delete=False) as f:
        f.write(synth.birdnet_v24())
        path = f.name
    try:
        model = bn.Model(path)
        ctxs = [bn.Context(model, a.batch) for _ in range(a.contexts)]
        warm = bn.Recording(mono16[:SEG * a.batch * a.contexts])
        analyse(ctxs, warm, a.batch, a.top_k)  # graph captures are not what is measured
        out = {"tool": "ingest_bench", "layout": a.layout, "hours": minutes / 60.0, "contexts": a.contexts, "batch": a.batch, "bytes": int(raw.nbytes)}

        t0 = time.perf_counter()
        rec = bn.Recording.from_layout(raw, fmt, channels, channel, async_upload=True)
        g = analyse(ctxs, rec, a.batch, a.top_k)
        out["device_layout_s"] = time.perf_counter() - t0
        del rec

        t0 = time.perf_counter()
        x = host_convert(raw, fmt, channels, channel)
        out["host_convert_s"] = time.perf_counter() - t0
        rec = bn.Recording(x, async_upload=True)
        analyse(ctxs, rec, a.batch, a.top_k)
        out["host_convert_then_mono_f32_s"] = time.perf_counter() - t0
        del rec, x

        t0 = time.perf_counter()
        rec = bn.Recording(mono16, async_upload=True)
        analyse(ctxs, rec, a.batch, a.top_k)
        out["mono_i16_s"] = time.perf_counter() - t0
        out["windows"] = g
        out["device_layout_windows_per_s"] = g / out["device_layout_s"]
        out["mono_i16_windows_per_s"] = g / out["mono_i16_s"]
        print(json.dumps(out))
    finally:
        os.unlink(path)


if __name__ == "__main__":
    main()
