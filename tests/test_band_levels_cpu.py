"""Band-limited window levels without a GPU: the float64 restatement of tests/band_levels_ref.py against cases worked by hand; the
header's bound against four wrong references on the exact inputs of the GPU random-audio test (a bound that let them pass would
check nothing); bn_band_bins through the library (host only); the host arithmetic of csrc/band_plan.h under ASan / UBSan
(tools/asan_band_plan.cpp); the header, the library, the harness and the Rust bindings agree on the new names, structs and constants.

The band_levels_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the
entry points and fail where the library lacks them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import band_levels_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against hand-computed cases --------------------------------------------------------------------------------
def test_reference_frames_and_unread_tail():
    assert (ref.n_frames(144000, 1024, 512), ref.unread(144000, 1024, 512)) == (280, 128)
    assert (ref.n_frames(4096, 256, 100), ref.unread(4096, 256, 100)) == (39, 40)
    assert (ref.n_frames(256, 256, 256), ref.unread(256, 256, 256)) == (1, 0)


def test_reference_bin_centred_sine_reads_half_a_squared():
    S, N, hop, A, k0 = 4096, 256, 128, 0.25, 20
    x = (A * np.sin(2 * np.pi * k0 * np.arange(S) / N + 0.3)).astype(np.float32)
    r = ref.band_levels(x, S, S, N, hop, [(k0 - 1, k0 + 2), (0, k0 - 4), (k0 + 5, N // 2 + 1), (k0, k0 + 1)])
    assert r["n_frames"].tolist() == [31] and r["flags"].tolist() == [0]
    for kind in ("mean", "max"):
        assert abs(r[kind][0, 0] - A * A / 2) < 1e-6 * A * A        # the tone with the window's two side bins
        assert r[kind][0, 1] < 1e-10 * A * A and r[kind][0, 2] < 1e-10 * A * A
        assert abs(r[kind][0, 3] - A * A / 3) < 1e-6 * A * A        # the centre bin alone holds 2/3 of it: (N/4)^2 * 2 / (3 N^2 / 8) = 1/3 of A^2
    assert abs(r["total_mean"][0] - A * A / 2) < 1e-6 * A * A and abs(r["total_max"][0] - A * A / 2) < 1e-6 * A * A


def test_reference_dc_and_nyquist():
    S, N, hop, c = 1024, 256, 256, 0.5
    half = N // 2
    dc = ref.band_levels(np.full(S, c, dtype=np.float32), S, S, N, hop, [(0, 1), (1, 2), (2, half + 1)])
    # X_0 = c N / 2, X_1 = -c N / 4, sum w^2 = 3 N / 8: P_0 = 2 c^2 / 3, P_1 = c^2 / 3, nothing else, c^2 in all
    assert np.allclose(dc["mean"][0], [2 * c * c / 3, c * c / 3, 0], rtol=0, atol=1e-15) and np.allclose(dc["max"][0], dc["mean"][0], rtol=0, atol=1e-15)
    assert abs(dc["total_mean"][0] - c * c) < 1e-15 and dc["n_frames"].tolist() == [4]
    ny = ref.band_levels((c * (-1.0) ** np.arange(S)).astype(np.float32), S, S, N, hop, [(half, half + 1), (half - 1, half), (0, half - 1)])
    assert np.allclose(ny["mean"][0], [2 * c * c / 3, c * c / 3, 0], rtol=0, atol=1e-15) and abs(ny["total_max"][0] - c * c) < 1e-15


def test_reference_impulse_in_one_frame():
    N = 256
    S = 4 * N
    x = np.zeros(S, dtype=np.float32)
    x[N + N // 2] = 1.0     # the centre of frame 1, where the window is 1: |X_k| = 1 for every k
    r = ref.band_levels(x, S, S, N, N, [(0, N // 2 + 1), (10, 20)])
    full = 8.0 / (3.0 * N)  # sum c_k / (N * 3 N / 8) = N / (3 N^2 / 8)
    assert abs(r["total_max"][0] - full) < 1e-15 and abs(r["total_mean"][0] - full / 4) < 1e-15
    assert abs(r["max"][0, 0] - full) < 1e-15 and abs(r["mean"][0, 0] - full / 4) < 1e-15
    assert abs(r["max"][0, 1] - 10 * 2 / (N * 3 * N / 8)) < 1e-15 and abs(r["mean"][0, 1] * 4 - r["max"][0, 1]) < 1e-15


def test_reference_padding_and_nonfinite():
    N, hop, S = 256, 64, 512
    x = np.random.RandomState(3).uniform(-1, 1, 700).astype(np.float32)
    r = ref.band_levels(x, S, S, N, hop, [(0, 129)])
    assert r["flags"].tolist() == [0, ref.PADDED]
    padded = ref.band_levels(np.concatenate([x, np.zeros(2 * S - 700, dtype=np.float32)]), S, S, N, hop, [(0, 129)])
    assert padded["mean"].tolist() == r["mean"].tolist() and padded["flags"].tolist() == [0, 0]
    # hop 100: n_frames 3, 56 positions unread -- a NaN there changes nothing, one inside a frame marks the window alone
    clean = ref.band_levels(x[:2 * S], S, S, N, 100, [(0, 129)])
    y = x[:2 * S].copy()
    y[S - 1] = np.nan
    assert all(ref.band_levels(y, S, S, N, 100, [(0, 129)])[k].tolist() == clean[k].tolist() for k in clean)
    y[S - 57] = np.inf
    bad = ref.band_levels(y, S, S, N, 100, [(0, 129)])
    assert bad["flags"].tolist() == [ref.NONFINITE, ref.PADDED] and bad["mean"][0, 0] == np.inf and bad["total_max"][0] == np.inf and bad["mean"][1].tolist() == clean["mean"][1].tolist()


def test_bound_follows_from_the_header_constants():
    c = ref.header_constants()
    assert set(c) == {"BN_BAND_MAX", "BN_BAND_EPS_ULPS", "BN_BAND_SUM_DEPTH"} and c["BN_BAND_MAX"] == 8
    u = 2.0 ** -24
    eps, delta = c["BN_BAND_EPS_ULPS"] * u, (c["BN_BAND_SUM_DEPTH"] + 3) * u     # 9 frames: ceil(9 / 4) = 3
    assert ref.bound(0.25, 1.0, 9) == 2 * eps * 0.5 + eps * eps + delta * 0.25
    assert ref.bound(0.0, 0.0, 9) == 0.0


# ---- the bound is not vacuous -------------------------------------------------------------------------------------------------
PERTURBED = {"last frame dropped": lambda N, hop, S, bands: dict(frames=ref.n_frames(S, N, hop) - 1),
             "band edge moved by one bin": lambda N, hop, S, bands: dict(bands=[bands[0], (bands[1][0], bands[1][1] + 1), bands[2]]),
             "one-sided factor 2 forgotten": lambda N, hop, S, bands: dict(one_sided=1.0),
             "rectangular window": lambda N, hop, S, bands: dict(window=np.ones(N))}


@pytest.mark.parametrize("N", ref.FRAMES)
def test_bound_rejects_perturbed_references(N):
    """on the exact inputs of test_gpu_band_levels.py's random-audio test, each wrong rule must leave the declared bound for at least one
    (window, band) -- here it does so for every (N, hop)"""
    import pcm_ref
    for hop in (N, N // 2, 100):
        v, S, step, bands = ref.random_case(N, hop)
        x = pcm_ref.mono(pcm_ref.pack(v, pcm_ref.I16), pcm_ref.I16, 1, 0)
        true = ref.band_levels(x, S, step, N, hop, bands)
        assert len(true["flags"]) == 5 and ref.worst_share(true, true) == 0.0
        for what, make in PERTURBED.items():
            kw = make(N, hop, S, bands)
            wrong = ref.band_levels(x, S, step, N, hop, kw.pop("bands", bands), **kw)
            b = ref.bounds(true)
            outside = sum(int((np.abs(wrong[k] - true[k]) > b[k]).sum()) for k in ("mean", "max"))
            assert outside >= 1, (what, N, hop)


# ---- bn_band_bins: host only ------------------------------------------------------------------------------------------------------
def test_band_bins_through_the_library(bn):
    assert bn.band_bins(48000, 1024, 2000.0, 10000.0) == (43, 214) == ref.bins(48000, 1024, 2000.0, 10000.0)
    # exactly the bins whose centres k * 46.875 Hz lie inside
    assert 42 * 46.875 < 2000.0 <= 43 * 46.875 and 213 * 46.875 < 10000.0 <= 214 * 46.875
    for rate, N, lo, hi in ((48000, 256, 0.0, 24000.0), (22050, 2048, 60.0, 61.0 + 22050 / 2048), (44100, 512, 1000.0, 1e12), (48000, 1024, 46.875, 93.75)):
        assert bn.band_bins(rate, N, lo, hi) == ref.bins(rate, N, lo, hi), (rate, N, lo, hi)
    lo, hi = C.c_uint32(7), C.c_uint32(7)
    for args, word in (((0, 1024, 1.0, 2000.0), "sample_rate"), ((48000, 1000, 1.0, 2000.0), "frame"), ((48000, 1024, 2000.0, 2000.0), "lo_hz"),
                       ((48000, 1024, 3000.0, 2000.0), "lo_hz"), ((48000, 1024, float("nan"), 2000.0), "lo_hz"), ((48000, 1024, 10.0, 20.0), "no bin centre"),
                       ((48000, 1024, 24001.0, 30000.0), "no bin centre")):
        assert bn.lib.bn_band_bins(*args, C.byref(lo), C.byref(hi)) == 1 and word in bn.last_error(), (args, bn.last_error())
        assert (lo.value, hi.value) == (7, 7)
        with pytest.raises(bn.EngineError):
            bn.band_bins(*args)
    assert bn.lib.bn_band_bins(48000, 1024, 1.0, 2000.0, None, C.byref(hi)) == 1 and "null" in bn.last_error()


# ---- the plan arithmetic under the sanitizers -------------------------------------------------------------------------------------
def test_plan_and_refusals_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path / "asan_band_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_band_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the plan check failed:\n" + r.stderr[-3000:])
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"\d+ plans, 0 failures", r.stdout) and "asan_band_plan: ok" in r.stdout, r.stdout


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "birdnet_host.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("bn_recording_band_levels", "bn_band_bins"):
        assert re.search(r"^bn_status " + name + r"\(", header, flags=re.M), name
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS and ("pub fn " + name + "(") in ffi, name
    assert re.search(r"\bbnh_recording_band_levels\(", host) and hasattr(L, "bnh_recording_band_levels") and "bnh_recording_band_levels" in bn.HOST_SYMBOLS
    assert "band_levels(size_t segment_samples" in host
    for struct in ("bn_band_spec", "bn_window_bands"):
        assert ("pub struct " + struct) in ffi, struct
    consts = ref.header_constants()
    assert consts == {"BN_BAND_MAX": bn.BN_BAND_MAX, "BN_BAND_EPS_ULPS": bn.BN_BAND_EPS_ULPS, "BN_BAND_SUM_DEPTH": bn.BN_BAND_SUM_DEPTH}
    for name, value in consts.items():
        assert re.search(r"pub const " + name + r": \w+ = " + str(value) + ";", ffi), name
    # the structs as the header lays them out: 3 + 8 + 8 and 8 + 8 + 4 32-bit fields
    assert C.sizeof(bn.BnBandSpec) == 76 and C.sizeof(bn.BnWindowBands) == 80 == bn.BAND_DTYPE.itemsize
    assert [f[0] for f in bn.BnWindowBands._fields_] == list(bn.BAND_DTYPE.names) == ["mean", "max", "total_mean", "total_max", "flags", "n_frames"]
    assert [getattr(bn.BnWindowBands, f).offset for f in ("mean", "max", "total_mean", "total_max", "flags", "n_frames")] == [0, 32, 64, 68, 72, 76]
    assert [getattr(bn.BnBandSpec, f).offset for f in ("frame", "hop", "n_bands", "bin_lo", "bin_hi")] == [0, 4, 8, 12, 44]
    assert bn.lib.bn_abi_version() == 2


def test_refusals_that_need_no_device(bn):
    out = (bn.BnWindowBands * 1)()
    sp = bn.band_spec(256, 128, [(0, 129)])
    args = (C.byref(sp), C.sizeof(bn.BnBandSpec), out)
    assert bn.lib.bn_recording_band_levels(None, 4096, 4096, 0, 1, *args, C.sizeof(bn.BnWindowBands)) == 1 and "null recording" in bn.last_error()
    assert bn.lib.bn_recording_band_levels(None, 4096, 4096, 0, 1, *args, C.sizeof(bn.BnWindowBands) - 1) == 1 and "struct_size" in bn.last_error()
    err, n = bn.BnhError(), C.c_size_t(7)
    assert bn.lib.bnh_recording_band_levels(None, 4096, 4096, C.byref(sp), 0, 1, out, 1, C.byref(n), C.byref(err)) != 0
    assert n.value == 0 and b"null recording" in err.message
    assert bytes(out) == bytes(80)
