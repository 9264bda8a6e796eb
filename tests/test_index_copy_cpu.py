"""bn_index_append_rows / bn_index_append_subset without a GPU: the numpy rules of tests/index_copy_ref.py against a literal per-row loop
over the header's sentences; the header, the library, the harness and the Rust bindings agree on the new names; NULL handles are refused
before the device is asked for; without a device the calls refuse with the no-device status and leave *first_new_id alone; the argument
and plan arithmetic runs clean under ASan / UBSan (tools/asan_index_copy_plan.cpp).

The index_copy_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the
entry points and fail where the library lacks them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import index_copy_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NAMES = ("bn_index_append_rows", "bn_index_append_subset")
SENTINEL = 0xABCDEF0123
u64p = C.POINTER(C.c_uint64)


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def stored(rng, n, dim):
    """n stored rows: unit length, one all-zero row, one pair of identical rows (n >= 5)"""
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True).astype(np.float32)
    X[2] = 0.0
    X[4] = X[1]
    return X


def cases(n, dim=5):
    """(dst, src) with and without tag planes on either side; dst already holds 3 rows"""
    rng = np.random.default_rng(11)
    X, D = stored(rng, n, dim), stored(rng, 5, dim)[:3]
    for src_tagged in (False, True):
        for dst_tagged in (False, True):
            src = cr.state(X, (np.arange(n) * 7 + 1) % 65536 if src_tagged else None)
            dst = cr.state(D, [9, 0, 65535] if dst_tagged else None, capacity=3 + n)
            yield dst, src
            yield cr.empty(dim, n, dst_tagged), src


def test_reference_equals_a_literal_loop_over_ranges_and_lists():
    n = 12
    ranges = ((0, 0), (0, n), (3, 3), (n, 0), (n - 1, 1))
    lists = ([], [5], list(range(n)), list(range(0, n, 2)), [n - 1])
    calls = 0
    for dst, src in cases(n):
        before = (dst.rows.tobytes(), dst.valid.tobytes(), None if dst.tags is None else dst.tags.tobytes(), dst.size)
        for kw in [dict(first_id=f, n_ids=c) for f, c in ranges] + [dict(ids=l) for l in lists]:
            got, first_new = cr.append(dst, src, **kw)
            loop = cr.append_loop(dst, src, **kw)
            assert cr.same_state(got, loop) and first_new == loop[4] == dst.size, kw
            old = cr.source_ids(src, **kw)
            assert got.size == dst.size + len(old) and got.rows[dst.size:].tobytes() == src.rows[old].tobytes()
            assert got.rows[:dst.size].tobytes() == dst.rows.tobytes() and np.array_equal(got.read_tags()[:dst.size], dst.read_tags())
            assert np.array_equal(got.read_tags()[dst.size:], src.read_tags()[old]) and np.array_equal(got.valid[dst.size:], src.valid[old])
            calls += 1
        assert before == (dst.rows.tobytes(), dst.valid.tobytes(), None if dst.tags is None else dst.tags.tobytes(), dst.size), "append() copies"
    assert calls == 8 * 10


def test_reference_tag_planes():
    rng = np.random.default_rng(12)
    X = stored(rng, 6, 4)
    tagged, plain = cr.state(X, [1, 2, 3, 4, 5, 6]), cr.state(X)
    a, _ = cr.append(cr.empty(4, 6), tagged, 1, 2)
    assert a.tags.tolist() == [2, 3], "src with a plane, dst without: the plane appears"
    b, _ = cr.append(cr.state(X[:2], [7, 8], capacity=9), plain)
    assert b.tags.tolist() == [7, 8] + [0] * 6, "src without, dst with: zeros are written"
    c, _ = cr.append(cr.empty(4, 6), plain)
    assert c.tags is None and not c.read_tags().any(), "neither has a plane"
    d, _ = cr.append(cr.empty(4, 6), tagged, 6, 0)
    assert d.tags is None and d.size == 0, "an empty copy creates nothing"
    assert c.valid.tolist() == [True, True, False, True, True, True] and c.rows[1].tobytes() == c.rows[4].tobytes()


def test_reference_refusals_leave_the_state_and_agree_with_the_loop():
    rng = np.random.default_rng(13)
    src = cr.state(stored(rng, 8, 4), np.arange(8))
    dst = cr.state(stored(rng, 5, 4)[:2], capacity=9)
    for kw, word in ((dict(first_id=0, n_ids=8), "capacity"),     # 2 + 8 rows into 9: overflow by one row
                     (dict(ids=list(range(8))), "capacity"),
                     (dict(first_id=9), "range"), (dict(first_id=0, n_ids=9), "range"), (dict(first_id=7, n_ids=2), "range"),
                     (dict(same=True), "same index"), (dict(ids=[1], same=True), "borrows")):
        for f in (cr.append, cr.append_loop):
            with pytest.raises(cr.Refused, match=word):
                f(dst, src, **kw)
    other = cr.state(stored(rng, 8, 5))
    for f in (cr.append, cr.append_loop):
        with pytest.raises(cr.Refused, match="dim"):
            f(dst, other)
    got, first = cr.append(dst, src, 1, 7)
    assert got.size == 9 == got.capacity and first == 2, "exactly full is legal"
    assert dst.size == 2 and dst.tags is None


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = dict(re.findall(r"^bn_status (bn_index_append_\w+)\(([^;]*)\);", header, flags=re.M))
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        bound = re.search(r"pub fn %s\(([^;]*)\)" % name, ffi)
        assert bound and len(bound.group(1).split(",")) == len(declared[name].split(",")), name
        assert len(getattr(bn.lib, name).argtypes) == len(declared[name].split(","))
    assert header.index("bn_subset_search_ids(") < header.index("bn_index_append_rows(") < header.index("bn_index_search_peaks("), "after the subset block"
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert all(hasattr(bn.Index, m) for m in ("append_rows", "append_subset"))


def test_null_handles_are_refused_before_any_device_call(bn):
    """these refusals need no device: they are the same with and without a GPU"""
    first = C.c_uint64(SENTINEL)
    fake = C.c_void_p(0x1000)                                 # never dereferenced: the NULL is found first
    calls = ((lambda: bn.lib.bn_index_append_rows(None, fake, 0, 0, C.byref(first)), "null destination"),
             (lambda: bn.lib.bn_index_append_rows(fake, None, 0, 0, C.byref(first)), "null source index"),
             (lambda: bn.lib.bn_index_append_rows(None, None, 5, 5, None), "null destination"),
             (lambda: bn.lib.bn_index_append_subset(None, fake, C.byref(first)), "null destination"),
             (lambda: bn.lib.bn_index_append_subset(fake, None, C.byref(first)), "null source subset"),
             (lambda: bn.lib.bn_index_append_subset(None, None, None), "null destination"))
    for call, word in calls:
        assert call() == INVALID_ARG and word in bn.last_error(), word
    assert first.value == SENTINEL


def test_no_device_means_refusal_and_an_untouched_first_new_id(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    first = C.c_uint64(SENTINEL)
    a, b = C.c_void_p(0x1000), C.c_void_p(0x2000)             # never dereferenced: the device is asked for first
    for first_id, n_ids in ((0, 0), (3, 3), (1 << 40, 1)):
        assert bn.lib.bn_index_append_rows(a, b, first_id, n_ids, C.byref(first)) == NO_DEVICE and "gfx950" in bn.last_error()
    assert bn.lib.bn_index_append_rows(a, a, 0, 0, C.byref(first)) == NO_DEVICE, "dst == src is refused after the device"
    assert bn.lib.bn_index_append_subset(a, b, C.byref(first)) == NO_DEVICE and "gfx950" in bn.last_error()
    assert bn.lib.bn_index_append_subset(a, b, None) == NO_DEVICE
    assert first.value == SENTINEL
    with pytest.raises(bn.EngineError):
        bn.Index(0, 8, 4)


# ---- the argument and plan arithmetic under the sanitizers ------------------------------------------------------------------------
def test_plan_and_refusals_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path / "asan_index_copy_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_index_copy_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the plan check failed:\n" + r.stderr[-3000:])
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"\d+ plans, \d+ walks, 0 failures", r.stdout), r.stdout
