#!/usr/bin/env python3
"""Plans of the synthetic models under every planner switch setting, one line each -- the GPU-free proof that a change to the planner's
host code left its plans alone ("Plans are the parent's").

Builds tools/plan_digest.cpp (unsanitized, the line in that file's header), writes the synthetic models with synth.py, runs the digest
under each setting and prints, per (model, setting):  model  setting  bytes  sha256-of-the-digest-text.

  tools/plan_sweep.py                      14 models: the sizes of tests/test_planner_sanitizers.py (both), of tests/test_gpu_models.py,
                                           the v24 model with the `dft` and `stft` front ends, and smoke()'s
  tools/plan_sweep.py --small              the 8 of tests/test_planner_sanitizers.py only
  tools/plan_sweep.py --full-text DIR      also keeps every digest text as DIR/<model>@<setting>.txt (compare two trees with diff -r)
  tools/plan_sweep.py --strip-fnv          hashes the text without the constants' fnv= values (their bytes come from numpy and libm and may
                                           differ in the last bit between machines; len= and off= stay) -- tests/golden/plan_sweep_small.txt
To compare with another commit, copy this script onto a checkout of it and run it there: it reads the tree it lies in.
"""
import argparse
import concurrent.futures
import hashlib
import importlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc")

# One-at-a-time values.  Which switches: the rows of BN_SWITCH_TABLE (switches.h, the source of kSwitchTable) in the sections the planner
# and plan_rules.h read.  By kind: `present` is set, `on_unless_0` gets 0, an `integer` gets 0 (1 where 0 is its default); every other
# documented non-default value, and one other value of each real and size, is listed here.
VALUES = {
    "BN_CONVMERGE": ["0", "1"], "BN_CONVFOLD": ["0"], "BN_CONVFOLD_TOL": ["1e-3"], "BN_STFT": ["0", "1"], "BN_STFT_MINBINS": ["64"],
    "BN_STFT_TOL": ["1e-5"], "BN_STFT_MEL": ["0", "force"], "BN_SEFUSE": ["dw", "mb", "1"], "BN_MBFUSE": ["0", "force"],
    "BN_MBFUSE_MAXK": ["24"], "BN_MBFUSE_HALO": ["1.5"], "BN_MBMAP": ["1"], "BN_MBMAP_MAXHW": ["128"], "BN_MBROW": ["0", "force"],
    "BN_MBROW_TR": ["0", "1"], "BN_MBROW_TOH": ["4"], "BN_GEMM3": ["0", "1"], "BN_GEMM3_KS": ["1", "2"], "BN_GEMMDMA": ["0", "2"],
    "BN_GEMMDMA_KS": ["1", "2"], "BN_SPLITK_MINK": ["128"], "BN_SPLITK_MAXROWS": ["64"],
}
SKIP = {"BN_STFT_DEBUG"}  # makes the planner print what its recognition found: not a plan
# tests/test_planner_sanitizers.py, RULE_SETS (the first is the defaults)
RULE_SETS = [
    {"BN_SEGEMM": "1", "BN_STFT": "1", "BN_STFT_MEL": "force", "BN_MBMAP3": "1"},
    {"BN_STFT": "0", "BN_MBMAP2": "0", "BN_GEMMDMA": "0", "BN_MBROW": "0", "BN_CONVFOLD": "0", "BN_GEMMPOST": "0"},
    {"BN_GEMMDMA": "2", "BN_MBFUSE": "force", "BN_MBMAP": "1", "BN_STFT_MELMFMA": "0", "BN_STFT_POWER": "0", "BN_REDUCE_SPLIT": "0"},
    {"BN_CONVFOLD2": "0", "BN_CONVMERGE": "0", "BN_FRAME_PRE": "0", "BN_GEMMGAP": "0"},
    {"BN_CONVMERGE": "1", "BN_STFT": "0"},
]
# opt-ins that act together
COMBINATIONS = [
    {"BN_SEGEMM": "1", "BN_SEGEMM_MAXC": "64"},
    {"BN_SEFUSE": "1", "BN_MBROW": "0"},
    {"BN_SEFUSE": "1", "BN_MBFUSE": "force"},
    {"BN_SEFUSE": "1", "BN_SEGEMM": "1"},
    {"BN_MBMAP3": "1", "BN_MBMAP_BANDS": "0"},
    {"BN_MBMAP3": "1", "BN_MBFUSE": "force"},
]


def planner_switches():
    """(kind, name, default) of every row in the planner's and the shape rules' sections of BN_SWITCH_TABLE."""
    rows, on = [], False
    for line in open(os.path.join(CSRC, "switches.h")):
        m = re.match(r"\s*/\* ---- (.*?) \*/", line)
        if m:
            on = m.group(1).startswith(("planner", "shape rules"))
        m = re.match(r"\s*X\((\w+),\s*(\w+),\s*([^,]+),", line)
        if m and on and m.group(2) not in SKIP:
            rows.append((m.group(1), m.group(2), m.group(3).strip()))
    return rows


def settings():
    out = [{}]
    for kind, name, dflt in planner_switches():
        values = VALUES.get(name) or (["1"] if kind == "present" or (kind == "integer" and dflt == "0") else ["0"])
        out += [{name: v} for v in values]
    return out + RULE_SETS + COMBINATIONS


def label(s):
    return ",".join(f"{k}={v}" for k, v in s.items()) or "defaults"


def models(small):
    synth = importlib.import_module("rust-birdnet-onnx_amd.synth")
    out = [("v24_tiny", synth.birdnet_v24(num_species=50, width=0.25, depth=0.25, head=64)),
           ("v30_tiny", synth.birdnet_v30(num_species=40, width=0.25, depth=0.25)),
           ("perch_tiny", synth.perch_v2(num_species=60, width=0.25, depth=0.25, emb=96)),
           ("meta_tiny", synth.meta_model(num_species=30, hidden=8)),
           ("v24", synth.birdnet_v24()), ("v30", synth.birdnet_v30()), ("perch", synth.perch_v2()), ("meta", synth.meta_model())]
    if not small:
        out += [("v24_small", synth.birdnet_v24(num_species=500, width=0.5, depth=0.5, head=256)),
                ("v30_small", synth.birdnet_v30(num_species=300, width=0.5, depth=0.34, emb=1024)),
                ("perch_small", synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)),
                ("v24_small_dft", synth.birdnet_v24(num_species=500, width=0.5, depth=0.5, head=256, front_end="dft")),
                ("v24_small_stft", synth.birdnet_v24(num_species=500, width=0.5, depth=0.5, head=256, front_end="stft")),
                ("v24_smoke", synth.birdnet_v24(num_species=6522, width=0.5, depth=0.5, head=256))]
    return out


def build_digest(out):
    cmd = ["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           os.path.join(ROOT, "tools", "plan_digest.cpp")]
    # the planner's files as the header of plan_digest.cpp lists them
    head = open(os.path.join(ROOT, "tools", "plan_digest.cpp")).read(2000)
    names = re.search(r"csrc/\{([\w,]+)\}\.cpp", head).group(1).split(",")
    subprocess.run(cmd + [os.path.join(CSRC, f + ".cpp") for f in names] + ["-o", out], check=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--strip-fnv", action="store_true")
    ap.add_argument("--full-text", metavar="DIR")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.full_text:
        os.makedirs(args.full_text, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "plan_digest")
        build_digest(exe)
        files = []
        for name, data in models(args.small):
            files.append(os.path.join(tmp, name + ".onnx"))
            with open(files[-1], "wb") as f:
                f.write(data)
        base_env = {k: v for k, v in os.environ.items() if not k.startswith("BN_")}

        def run(s):
            r = subprocess.run([exe] + files, env=dict(base_env, **s), capture_output=True, check=True)
            return re.split(rb"(?m)^(?=== )", r.stdout)[1:]  # one text per model, in order

        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            sets = settings()
            for s, texts in zip(sets, pool.map(run, sets)):
                assert len(texts) == len(files), (label(s), len(texts))
                for path, text in zip(files, texts):
                    model = os.path.basename(path)[:-5]
                    if args.full_text:
                        with open(os.path.join(args.full_text, f"{model}@{label(s)}.txt"), "wb") as f:
                            f.write(text)
                    hashed = re.sub(rb"(?m)^(const \d+: .*) fnv=[0-9a-f]+$", rb"\1", text) if args.strip_fnv else text
                    print(model, label(s), len(text), hashlib.sha256(hashed).hexdigest())


if __name__ == "__main__":
    main()
