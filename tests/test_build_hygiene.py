"""Build hygiene (CPU): no kernel of the library may use scratch memory.

Round 3 found that the 5 x 5 row-streaming MBConv instances had been spilling 160-590 bytes per lane to scratch memory since round 2
(BirdNET v3.0 lost 7 % to it) -- nothing in the test suite could see that.  This test reads the AMDGPU metadata notes of every HIP
object file of the in-tree build (`.private_segment_fixed_size` per kernel) and fails if any kernel has a
non-zero scratch size.  It needs the objects `make` leaves next to the sources and the LLVM binutils of the ROCm image; it is skipped
where either is missing (the GPU box runs the prebuilt .so only)."""
import glob
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rust-birdnet-onnx_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"


def kernels_with_scratch(obj, tmp):
    fat, hsaco, scratch_copy = os.path.join(tmp, "x.fatbin"), os.path.join(tmp, "x.hsaco"), os.path.join(tmp, "x.o")
    for f in (fat, hsaco, scratch_copy):
        if os.path.exists(f):
            os.unlink(f)
    # an explicit OUTPUT operand: without one llvm-objcopy rewrites its input in place, i.e. this test re-stamped the build's own
    # object files and the next `make` relinked the library from them -- a test must not mutate the build
    r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, scratch_copy], capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(fat):
        return None  # no device code in this object
    r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}",
                        f"--output={hsaco}"], capture_output=True, text=True)
    assert r.returncode == 0 and os.path.exists(hsaco), r.stderr
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", hsaco], capture_output=True, text=True).stdout
    out, name = [], None
    for line in notes.splitlines():
        m = re.match(r"\s+\.name:\s+(\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.private_segment_fixed_size:\s+(\d+)", line)
        if m and name is not None:
            out.append((name, int(m.group(1))))
            name = None
    return out


def test_no_kernel_uses_scratch_memory(tmp_path):
    objs = sorted(glob.glob(os.path.join(CSRC, "*.o")))
    if not objs or not all(os.path.exists(f"{LLVM}/{t}") for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")):
        pytest.skip("needs the in-tree build's object files and the ROCm LLVM binutils")
    before = {o: (os.stat(o).st_mtime_ns, os.stat(o).st_size) for o in objs}
    seen, offenders = 0, []
    for obj in objs:
        ks = kernels_with_scratch(obj, str(tmp_path))
        if ks is None:
            continue
        seen += len(ks)
        offenders += [(os.path.basename(obj), n, b) for n, b in ks if b > 0]
    assert before == {o: (os.stat(o).st_mtime_ns, os.stat(o).st_size) for o in objs}, "the test touched the build's object files"
    assert seen > 200, f"only {seen} kernels found: the objects are not the HIP build"
    assert not offenders, "kernels with scratch memory (register spills): " + "; ".join(f"{o}:{n} {b} B" for o, n, b in offenders[:8])
