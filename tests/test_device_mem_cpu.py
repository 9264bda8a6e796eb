"""The resource owners of csrc/device_mem.h over a runtime that only counts (tools/owner_check.cpp), compiled for the host with
-fsanitize=address,undefined: no device, nothing preloaded.  Empty owners release nothing, a scope exit releases once, moves hand
over, a failed acquisition leaves the owner empty, a creation shaped like bn_ctx_create balances at every failure position, and
members go in reverse order of declaration."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def owner_check(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("owner") / "owner_check"
    src = os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), "-I" + src, os.path.join(ROOT, "tools", "owner_check.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the owner check failed:\n" + r.stderr[-3000:])
    return str(out)


def test_owners_under_asan_ubsan(owner_check):
    r = subprocess.run([owner_check], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert "owner_check ok:" in r.stdout and "check failed" not in r.stderr, (r.stdout, r.stderr[-3000:])
