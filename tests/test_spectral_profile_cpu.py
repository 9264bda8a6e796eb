"""The spectral profile without a GPU: the refusals bn_recording_spectral_profile reaches before it needs a device, through the
library; the host arithmetic of csrc/profile_plan.h under ASan / UBSan (tools/asan_profile_plan.cpp); and the reference itself
(tests/spectral_profile_ref.py) on the exact inputs of the GPU random-audio test: four wrong rules leave the header's bounds for
every (N, hop), and the propagated ACI bound stays below 1 % of the ACI, so the ACI check is not vacuous.

The tests that take the `bn` fixture and the sanitizer build fail where the library lacks the entry point."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import band_levels_ref as band
import pcm_ref
import spectral_profile_ref as ref

ROOT = band.ROOT


def test_refusals_before_a_device_is_needed(bn):
    L, size = bn.lib, C.sizeof(bn.BnWindowProfile)
    assert size == 16 == bn.PROFILE_DTYPE.itemsize and C.sizeof(bn.BnProfileSpec) == 16 and bn.lib.bn_abi_version() == 2
    out, bins, spec = (bn.BnWindowProfile * 2)(), (C.c_float * 64)(), bn.BnProfileSpec(256, 128, 0, 10)
    for args, message in (((None, 1024, 100, 0, 1, C.byref(spec), 16, out, size, bins), "null recording"),
                          ((None, 6, 0, 0, 1, None, 0, None, size + 8, None), "null recording"),  # ... before the segment and the spec
                          ((None, 1024, 100, 0, 1, C.byref(spec), 16, out, size - 1, bins), "struct_size is below sizeof(bn_window_profile)"),
                          ((None, 1024, 100, 0, 0, None, 0, None, 0, None), "struct_size is below sizeof(bn_window_profile)")):
        assert L.bn_recording_spectral_profile(*args) == 1 and bn.last_error() == message, (args, bn.last_error())
    c = ref.header_constants()
    assert (c["BN_PROFILE_PLANES"], c["BN_PROFILE_POW_DEPTH"], c["BN_PROFILE_AMP_DEPTH"], c["BN_PROFILE_ACI_DEPTH"]) == \
        (bn.BN_PROFILE_PLANES, bn.BN_PROFILE_POW_DEPTH, bn.BN_PROFILE_AMP_DEPTH, bn.BN_PROFILE_ACI_DEPTH)


def test_plan_under_asan_ubsan(tmp_path):
    out = tmp_path / "asan_profile_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_profile_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout and "asan_profile_plan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_reference_known_answers():
    """a bin-centred sine whose amplitude alternates a, b from frame to frame (hop = N): D = (F - 1) |a - b| / sqrt 2 in all its bins
    together -- the centre bin holds 2/3 of the power -- and M = (a^2 + b^2) / 4 in all"""
    N, S, k0, a, b = 256, 4096, 20, 0.5, 0.2
    amp = np.repeat(np.where(np.arange(S // N) % 2 == 0, a, b), N)
    x = (amp * np.sin(2 * np.pi * k0 * np.arange(S) / N)).astype(np.float32)
    r = ref.profile(x, S, S, N, N, (k0, k0 + 1))
    assert r["n_frames"].tolist() == [16] and r["flags"].tolist() == [0]
    third = np.sqrt(2.0 / 3.0)  # the centre bin's share of the amplitude
    assert np.allclose(r["planes"][0, :, 0], [(a * a + b * b) / 4 * 2 / 3, 8 * (a + b) / np.sqrt(2) * third, 15 * (a - b) / np.sqrt(2) * third], rtol=1e-6)
    assert abs(r["aci"][0] - 15 * (a - b) / (8 * (a + b))) < 1e-6 and abs(r["total_mean"][0] - (a * a + b * b) / 4) < 1e-7


@pytest.mark.parametrize("N", ref.FRAMES)
def test_bounds_reject_wrong_rules_and_the_aci_bound_is_tight(N):
    for hop in (N, N // 2, 100):
        v, S, step = ref.random_case(N, hop)
        x = pcm_ref.mono(pcm_ref.pack(v, pcm_ref.I16), pcm_ref.I16, 1, 0)
        for bins in ref.bin_ranges(N):
            true = ref.profile(x, S, step, N, hop, bins)
            b = ref.bounds(true)
            assert set(ref.worst_share(true, true).values()) == {0.0}
            rel = float((b["aci"] / true["aci"]).max())
            print("frame", N, "hop", hop, "bins", bins, "aci bound / aci", rel)
            assert rel < 0.01, (N, hop, bins, rel)
        true = ref.profile(x, S, step, N, hop, (3, 17))
        for wrong in ref.WRONG:
            shares = ref.worst_share(ref.profile(x, S, step, N, hop, (3, 17), wrong=wrong), true)
            assert max(shares.values()) > 1.0, (wrong, N, hop, shares)
