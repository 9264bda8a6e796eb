"""The operands of finished plans, without a GPU: every launch names its buffers through PlanOp::Operands and for_each_ref (csrc/engine.h)
is the one list of them.  tools/asan_plan_operands.cpp, under ASan / UBSan, plans small models of the three families with the opt-in
fusions on -- an MBConv that finishes its squeeze-excite, a GEMM that computes one in its prologue, an FFT launch that absorbed its mel
bank -- and checks that the liveness of every storage follows from for_each_ref alone, that every ref names something the plan has and
that no weight, bias or table lives in the arena."""
import importlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")


def test_plan_operands_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path / "asan_plan_operands"
    src = os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + src, os.path.join(ROOT, "tools", "asan_plan_operands.cpp")]
    cmd += [os.path.join(src, f + ".cpp") for f in ("onnx_proto", "engine", "onnx_rewrite", "dft_bank", "mbconv_fuse", "plan_passes", "detect")] + ["-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the plan operand check failed:\n" + r.stderr[-3000:])
    files = []
    for name, data in (("v24", synth.birdnet_v24(num_species=50, width=0.25, depth=0.25, head=64)),
                       ("v30", synth.birdnet_v30(num_species=40, width=0.25, depth=0.25)),
                       ("perch", synth.perch_v2(num_species=60, width=0.25, depth=0.25, emb=96))):
        p = tmp_path / f"{name}.onnx"
        p.write_bytes(data)
        files.append(str(p))
    # the fusions that put a squeeze-excite into another launch are opt-in: the MBConv blocks finish their own (BN_MBROW=0 leaves them on the
    # kernel that has a last block), the blocks with a separate depthwise conv leave theirs to the project GEMM
    env = dict({k: v for k, v in os.environ.items() if not k.startswith("BN_")}, ASAN_OPTIONS="detect_leaks=0",
               BN_SEFUSE="mb", BN_MBROW="0", BN_SEGEMM="1", BN_STFT="1", BN_STFT_MEL="force")
    r = subprocess.run([str(out)] + files, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"3 plans, (\d+) operands, (\d+) tails, (\d+) inline, (\d+) mel banks, 0 failures", r.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), r.stdout
