"""Window levels and list steps without a GPU: the float64 restatement of tests/levels_ref.py against hand-computed cases; the host
arithmetic of csrc/window_list_plan.h under ASan / UBSan (tools/asan_window_list_plan.cpp); the header, the library, the harness and
the Rust bindings agree on the new names, structs and constants; arguments that need no device are refused before one is asked for.

The levels_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import levels_ref
import pcm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against hand-computed cases --------------------------------------------------------------------------------
def test_reference_levels_by_hand():
    x = np.array([0.5, -1.0, 0.25, 0.0, 0.5, 0.5], dtype=np.float32)
    r = levels_ref.levels(x, 4, 2)
    # windows [0.5 -1 0.25 0] [0.25 0 0.5 0.5] [0.5 0.5 0 0]: the last reaches past the end and is padded; the divisor stays 4
    assert r["peak"].tolist() == [1.0, 0.5, 0.5]
    assert r["mean"].tolist() == [-0.0625, 0.3125, 0.25]
    assert r["mean_square"].tolist() == [(0.25 + 1 + 0.0625) / 4, (0.0625 + 0.25 + 0.25) / 4, 0.125]
    assert r["mean_abs"].tolist() == [0.4375, 0.3125, 0.25]
    assert r["flags"].tolist() == [0, 0, levels_ref.PADDED]
    one = levels_ref.levels(x, 4, 2, 1, 1)
    assert all(one[k].tolist() == r[k][1:2].tolist() for k in r)


def test_reference_short_recording_and_full_scale():
    r = levels_ref.levels(pcm_ref.mono(pcm_ref.pack([-32768, 16384, 0], pcm_ref.I16), pcm_ref.I16, 1, 0), 4, 4)
    assert r["peak"].tolist() == [1.0] and r["flags"].tolist() == [levels_ref.PADDED]
    assert r["mean"].tolist() == [-0.125] and r["mean_square"].tolist() == [(1 + 0.25) / 4]
    z = levels_ref.levels(np.zeros(9, dtype=np.float32), 4, 4)
    assert all(not z[k][:2].any() for k in ("peak", "mean", "mean_square", "flags")) and z["flags"].tolist() == [0, 0, levels_ref.PADDED]


def test_reference_nonfinite_marks_only_its_windows():
    x = np.linspace(-1, 1, 12).astype(np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[5] = bad
        r = levels_ref.levels(y, 4, 4)
        assert r["flags"].tolist() == [0, levels_ref.NONFINITE, 0]
        assert r["peak"][1] == np.inf and r["mean_square"][1] == np.inf and r["mean"][1] == 0
        clean = levels_ref.levels(x, 4, 4)
        assert all(r[k][[0, 2]].tolist() == clean[k][[0, 2]].tolist() for k in ("peak", "mean", "mean_square"))


def test_reference_gate_with_hangover():
    peaks = np.array([0, 0, 0.5, 0, 0, 0, 0, 0.01, 0.02, 0], dtype=np.float32)
    assert levels_ref.gate(peaks, 0.01).tolist() == [1, 2, 3, 6, 7, 8, 9]
    assert levels_ref.gate(peaks, 0.01, 0).tolist() == [2, 7, 8]
    assert levels_ref.gate(peaks[:3], 0.01).tolist() == [1, 2] and levels_ref.gate(peaks[:2], 0.01).tolist() == []


def test_header_bounds_follow_from_the_depth():
    ref = levels_ref.levels(np.array([0.5, -0.5, 0.25, 0.25], dtype=np.float32), 4, 4)
    a, r = levels_ref.bounds(ref, 1034)
    assert a.tolist() == [1035 * 2.0 ** -24 * 0.375] and r == 1036 * 2.0 ** -24


# ---- the plan arithmetic under the sanitizers -------------------------------------------------------------------------------------
def test_plan_and_refusals_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path / "asan_window_list_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_window_list_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the plan check failed:\n" + r.stderr[-3000:])
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"\d+ plans, 0 failures", r.stdout) and "asan_window_list_plan: ok" in r.stdout, r.stdout


# ---- the library without a device ---------------------------------------------------------------------------------------------
NAMES = ("bn_recording_levels", "bn_step_window_list", "bn_recording_window_list")


def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"^bn_status " + name + r"\(", header, flags=re.M), name
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS and ("pub fn " + name + "(") in ffi, name
    for struct in ("bn_window_level", "bn_window_ref"):
        assert ("pub struct " + struct) in ffi, struct
    defines = dict(re.findall(r"^#define (BN_LEVEL_\w+) (\d+)u?\b", header, flags=re.M))
    assert defines == {"BN_LEVEL_NONFINITE": "1", "BN_LEVEL_PADDED": "2", "BN_LEVEL_SUM_DEPTH": str(bn.BN_LEVEL_SUM_DEPTH)}
    assert (bn.BN_LEVEL_NONFINITE, bn.BN_LEVEL_PADDED) == (levels_ref.NONFINITE, levels_ref.PADDED) == (1, 2)
    for name, value in defines.items():
        assert re.search(r"pub const " + name + r": \w+ = " + value + ";", ffi), name
    # the structs as the header lays them out: 16 bytes of four 32-bit fields; pointer, u64, i32 (+ padding), u64
    assert C.sizeof(bn.BnWindowLevel) == 16 == bn.LEVEL_DTYPE.itemsize
    assert [f[0] for f in bn.BnWindowLevel._fields_] == list(bn.LEVEL_DTYPE.names) == ["peak", "mean", "mean_square", "flags"]
    assert C.sizeof(bn.BnWindowRef) == 32 and [getattr(bn.BnWindowRef, f).offset for f in ("recording", "start", "source", "window")] == [0, 8, 16, 24]


def test_refusals_that_need_no_device(bn):
    lv = (bn.BnWindowLevel * 1)()
    assert bn.lib.bn_recording_levels(None, 4, 4, 0, 1, lv, C.sizeof(bn.BnWindowLevel)) == 1 and "null recording" in bn.last_error()
    assert bn.lib.bn_recording_levels(None, 4, 4, 0, 1, lv, 15) == 1 and "struct_size" in bn.last_error()
    refs = (bn.BnWindowRef * 1)()
    out = np.zeros(4, dtype=np.float32)
    f32p = out.ctypes.data_as(C.POINTER(C.c_float))
    assert bn.lib.bn_recording_window_list(refs, 0, C.sizeof(bn.BnWindowRef), 4, f32p) == 0
    assert bn.lib.bn_recording_window_list(None, 1, C.sizeof(bn.BnWindowRef), 4, f32p) == 1 and "null window list" in bn.last_error()
    assert bn.lib.bn_recording_window_list(refs, 1, 31, 4, f32p) == 1 and "struct_size" in bn.last_error()
    assert bn.lib.bn_recording_window_list(refs, 1, C.sizeof(bn.BnWindowRef), 6, f32p) == 1 and "multiple of 4" in bn.last_error()
    assert bn.lib.bn_recording_window_list(refs, 1, C.sizeof(bn.BnWindowRef), 4, f32p) == 1 and "row 0: null recording" in bn.last_error()
    assert bn.lib.bn_step_window_list(None, refs, 1, C.sizeof(bn.BnWindowRef), 5, 0, 0.0, 1) == 1 and "null context" in bn.last_error()
    # counts that no list can have, before anything is sized by them
    assert bn.lib.bn_recording_window_list(refs, 2 ** 32, C.sizeof(bn.BnWindowRef), 4, f32p) == 1 and "2^32" in bn.last_error()
    assert bn.lib.bn_recording_window_list(refs, 2 ** 32 - 1, C.sizeof(bn.BnWindowRef), 2 ** 32 - 4, f32p) == 1 and "address space" in bn.last_error()
    assert not out.any()


def test_host_mirror_refusals_that_need_no_device(bn):
    header = open(os.path.join(ROOT, "include", "birdnet_host.h")).read()
    for name in ("bnh_recording_create", "bnh_recording_free", "bnh_recording_samples", "bnh_recording_levels", "bnh_predict_window_list"):
        assert re.search(r"\b" + name + r"\(", header) and name in bn.HOST_SYMBOLS, name
    assert "levels(size_t segment_samples" in header and "predict_window_list(BatchInferenceContext &ctx, const WindowRef *refs" in header
    err, n = bn.BnhError(), C.c_size_t(7)
    lv = (bn.BnWindowLevel * 1)()
    assert bn.lib.bnh_recording_levels(None, 4, 4, 0, 1, lv, 1, C.byref(n), C.byref(err)) != 0
    assert n.value == 0 and b"null recording" in err.message
    res = C.c_void_p(1)
    assert bn.lib.bnh_predict_window_list(None, None, None, None, None, None, 1, -1, None, C.byref(res), C.byref(err)) != 0
    assert res.value is None and b"null argument" in err.message
    assert bn.lib.bnh_recording_samples(None) == 0
    bn.lib.bnh_recording_free(None)
    if bn.device_count() == 0:     # without a device the upload fails as an inference error with the library's message, not a crash
        with pytest.raises(bn.Error) as e:
            bn.HostRecording(np.zeros(8, dtype=np.int16))
        assert e.value.kind == bn.ErrorKind.Inference
