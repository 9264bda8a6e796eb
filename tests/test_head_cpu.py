"""Classifier heads without a GPU: the float64 reference of tests/head_ref.py solves the fit fixtures to a certificate below 1e-20,
its gradient is the derivative of its loss, the ABI declares and exports the head entry points, the Rust binding carries the
options struct, and without a device create / fit / apply refuse with the no-device status instead of computing on the CPU.

The first three tests (test_newton_reference_*, test_reference_*) are self-checks of tests/head_ref.py: they make the reference
trustworthy before the GPU tests lean on it, touch no library code and therefore pass with or without the feature.  The tests that
take the `bn` fixture need the head entry points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import head_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 9
HEAD_SYMBOLS = ["bn_head_create", "bn_head_free", "bn_head_dim", "bn_head_classes", "bn_head_flags", "bn_head_read", "bn_head_apply_host",
                "bn_head_fit", "bn_head_fit_index", "bn_ctx_attach_head", "bn_step_head_results"]


@pytest.mark.parametrize("name", sorted(head_ref.FIXTURES))
def test_newton_reference_reaches_the_optimum(name):
    X, Y, l2, pw = head_ref.fixture(name)
    W, b = head_ref.newton(X, Y, l2, pw)
    loss, gW, gb, cert = head_ref.objective(W, b, X, Y, l2, pw)
    print(f"{name}: L* = {loss:.12f}, certificate {cert:.3e}")
    assert cert < 1e-20
    # every class has positives and negatives here, and the optimum is no trivial point
    assert 0 < Y.mean() < 1 and np.abs(W).max() > 0.1
    # strong convexity: any other point lies above L* by at most its own certificate
    rng = np.random.default_rng(3)
    W2, b2 = W + 1e-3 * rng.standard_normal(W.shape), b + 1e-3 * rng.standard_normal(b.shape)
    l2_, _, _, c2 = head_ref.objective(W2, b2, X, Y, l2, pw)
    assert 0 < l2_ - loss <= c2


def test_reference_gradient_is_the_derivative_of_the_reference_loss():
    X, Y, l2, _ = head_ref.fixture("n2000_d256_c3")
    pw = np.array([1.0, 4.0, 0.5])
    rng = np.random.default_rng(5)
    W, b = 0.3 * rng.standard_normal((3, 256)), 0.3 * rng.standard_normal(3)
    _, gW, gb, _ = head_ref.objective(W, b, X, Y, l2, pw)
    dW, db = rng.standard_normal(W.shape), rng.standard_normal(b.shape)
    h = 1e-6
    fp = head_ref.objective(W + h * dW, b + h * db, X, Y, l2, pw)[0]
    fm = head_ref.objective(W - h * dW, b - h * db, X, Y, l2, pw)[0]
    want = (gW * dW).sum() + (gb * db).sum()
    assert abs((fp - fm) / (2 * h) - want) <= 1e-8 * max(1.0, abs(want))


def test_reference_logits_follow_the_normalisation_rule():
    W = np.array([[1.0, 2.0, 3.0], [0.5, -1.0, 0.0]])
    b = np.array([0.25, -0.5])
    rows = np.array([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0], [1.0, np.inf, 0.0], [1e30, 1e30, 0.0]])
    z, bound = head_ref.logits64(W, b, rows, True)
    assert np.allclose(z[0], [0.25 + 0.6 + 2.4, -0.5 + 0.3])
    assert np.array_equal(z[1], b) and np.array_equal(z[2], b) and np.array_equal(z[3], b)  # zero norm, non-finite, f32 overflow
    assert np.all(bound >= 2 * 11 * 2.0 ** -24 * np.abs(b))


def test_header_library_and_harness_agree_on_the_head_entry_points(bn):
    L = C.CDLL(bn.LIB_PATH)
    for s in HEAD_SYMBOLS:
        assert hasattr(L, s), s
        assert s in bn.ENGINE_SYMBOLS, s
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    assert re.search(r"#define\s+BN_HEAD_L2NORM\s+1u", header) and bn.BN_HEAD_L2NORM == 1
    assert bn.lib.bn_abi_version() == 2
    # the options struct of the harness has the header's fields in the header's order
    body = re.search(r"typedef struct bn_head_fit_opts \{(.*?)\} bn_head_fit_opts;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in bn.BnHeadFitOpts._fields_]
    body = re.search(r"typedef struct bn_head_fit_report \{(.*?)\} bn_head_fit_report;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", body) == [f for f, _ in bn.BnHeadFitReport._fields_]
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub struct bn_head { _p: [u8; 0] }" in ffi
    body = re.search(r"pub struct bn_head_fit_opts \{(.*?)\}", ffi, flags=re.S).group(1)
    assert [m for m in re.findall(r"pub (\w+): ([^,]+),", body)] == [("l2", "f32"), ("tol", "f32"), ("max_iters", "u32"), ("flags", "u32"),
                                                                       ("pos_weight", "*const f32")]


def test_rust_binding_names_only_types_it_declares():
    """every type an extern item or struct field of ffi.rs names is a Rust primitive, a std alias the file imports, or declared in the file"""
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = set(re.findall(r"pub (?:struct|type) (\w+)", ffi)) | {"c_void", "c_char"}
    prim = {"i8", "u8", "i16", "u16", "i32", "u32", "i64", "u64", "usize", "isize", "f32", "f64"}
    body = re.search(r'extern "C" \{(.*?)\n\}', ffi, flags=re.S).group(1)
    used = set()
    for m in re.finditer(r":\s*([^,;)]+)|->\s*([^;]+);", body):
        used |= set(re.findall(r"[A-Za-z_]\w*", m.group(1) or m.group(2)))
    for sbody in re.findall(r"pub struct \w+ \{(.*?)\}", ffi, flags=re.S):
        for ty in re.findall(r"pub (?:r#)?\w+: ([^,]+),", sbody):
            used |= set(re.findall(r"[A-Za-z_]\w*", ty))
    used -= {"const", "mut"}
    consts = set(re.findall(r"pub const (\w+)", ffi))
    assert "uint8_t" in used, "the label arrays of bn_head_fit are the header's first uint8_t"
    unknown = sorted(t for t in used if t not in declared and t not in prim and t not in consts)
    assert not unknown, unknown
    gen_src = open(os.path.join(ROOT, "tools", "gen_rust_ffi.py")).read()
    assert "no Rust type for C type" in gen_src  # the generator refuses a C type it cannot map instead of passing the name through


def test_null_handles_answer_without_a_device(bn):
    assert bn.lib.bn_head_dim(None) == 0 and bn.lib.bn_head_classes(None) == 0 and bn.lib.bn_head_flags(None) == 0
    bn.lib.bn_head_free(None)
    assert bn.lib.bn_ctx_attach_head(None, None, 1, 0, C.c_float(0)) == 1
    assert bn.lib.bn_step_head_results(None, None, None, None, None, None, None) == 1


def test_no_device_means_refusal_not_a_cpu_fallback(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    X, Y, _, _ = head_ref.fixture("n2000_d256_c3")
    with pytest.raises(bn.EngineError) as e:
        bn.Head(0, np.ones((3, 256), dtype=np.float32), np.zeros(3, dtype=np.float32))
    assert e.value.status == NO_DEVICE
    with pytest.raises(bn.EngineError) as e:
        bn.Head.fit(0, X, Y, l2norm=True)
    assert e.value.status == NO_DEVICE
    f32p = C.POINTER(C.c_float)
    out = np.zeros((4, 3), dtype=np.float32)
    assert bn.lib.bn_head_apply_host(None, X.ctypes.data_as(f32p), 4, out.ctypes.data_as(f32p)) == NO_DEVICE
    h, rep = C.c_void_p(), bn.BnHeadFitReport()
    ids = np.arange(4, dtype=np.uint64)
    assert bn.lib.bn_head_fit_index(None, ids.ctypes.data_as(C.POINTER(C.c_uint64)), Y.ctypes.data_as(C.POINTER(C.c_uint8)), 4, 3, None, 0, C.byref(h),
                                    C.byref(rep), C.sizeof(rep)) == NO_DEVICE
    assert "gfx950" in bn.last_error() and not h.value
