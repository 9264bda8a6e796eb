"""bn_sq8_* without a GPU: the numpy rules of tests/sq8_ref.py on hand-made cases; the header, the library, the harness and the Rust
bindings agree on every entry point; arguments that need no view are refused before the device is asked for; without a device the
calls refuse with the no-device status and leave the caller's outputs alone.

The sq8_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sq8_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NAMES = ("bn_sq8_build", "bn_sq8_free", "bn_sq8_rows", "bn_sq8_extend", "bn_sq8_read", "bn_sq8_search", "bn_sq8_search_ids")
f32p, u32p, u64p, i8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int8)


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def test_reference_codes():
    rng = np.random.default_rng(1)
    X = rng.standard_normal((50, 37)).astype(np.float32)
    X /= np.sqrt((X * X).sum(axis=1, keepdims=True))
    X[7] = 0.0
    X[9] = -np.abs(X[9])                           # the maximum is negative
    c, s = sq8_ref.codes(X)
    assert c.dtype == np.int8 and s.dtype == np.float32
    assert not c[7].any() and s[7].tobytes() == np.float32(0.0).tobytes(), "an all-zero row: codes 0, scale +0.0"
    assert np.abs(c.astype(np.int32)).max() <= 127
    top = np.abs(X).argmax(axis=1)
    good = np.arange(50) != 7
    assert (np.abs(c[good, top[good]].astype(np.int32)) == 127).all() and c[9, top[9]] == -127
    assert np.array_equal(s[good], np.abs(X).max(axis=1)[good] / np.float32(127.0))
    # ties: with a = 127 the inverse is exactly 1 and r * inv = r, so x.5 elements round to even
    r = np.array([[127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 126.5, -126.5, 63.5]], dtype=np.float32)
    c, s = sq8_ref.codes(r)
    assert c[0].tolist() == [127, 0, 2, 2, 0, -2, -2, 126, -126, 64] and s[0] == np.float32(1.0)
    # scaled by a power of two the codes stay
    c2, s2 = sq8_ref.codes(r * np.float32(2.0 ** -9))
    assert np.array_equal(c2, c) and s2[0] == np.float32(2.0 ** -9)


def test_reference_keys_stay_in_int32():
    dim = 131072
    q = np.full((2, dim), 127, dtype=np.int8)
    q[1] = -127
    c = np.full((3, dim), 127, dtype=np.int8)
    c[1] = -127
    c[2] = 0
    K = sq8_ref.keys(q, c, np.array([1.0, 1.0, 0.0], dtype=np.float32))
    D = 127 * 127 * dim
    assert D < 2 ** 31 and K.dtype == np.float32
    assert K.tolist() == [[float(np.float32(D)), float(np.float32(-D)), 0.0], [float(np.float32(-D)), float(np.float32(D)), 0.0]]
    D = 127 * 127 * 2001                                       # odd and above 2^24: the int -> f32 conversion rounds
    K = sq8_ref.keys(q[:1, :2001], c[:1, :2001], np.ones(1, dtype=np.float32))
    assert int(np.float32(D)) != D and K[0, 0] == np.float32(D) and K[0, 0].tobytes() == np.array(D, dtype=np.int32).astype(np.float32).tobytes()
    K = sq8_ref.keys(q[:, :3], c[:, :3], np.array([0.5, 0.25, 7.0], dtype=np.float32))
    assert K.tolist() == [[3 * 16129 * 0.5, -3 * 16129 * 0.25, 0.0], [-3 * 16129 * 0.5, 3 * 16129 * 0.25, 0.0]]
    assert not np.signbit(K[:, 2]).any(), "D == 0 gives +0.0"
    rng = np.random.default_rng(7)                             # against a plain int32 product
    qq, cc = rng.integers(-127, 128, (5, 300)).astype(np.int8), rng.integers(-127, 128, (40, 300)).astype(np.int8)
    sc = rng.random(40).astype(np.float32)
    D = qq.astype(np.int32) @ cc.astype(np.int32).T
    assert D.dtype == np.int32 and sq8_ref.keys(qq, cc, sc).tobytes() == (D.astype(np.float32) * sc[None, :]).tobytes()


def test_reference_candidates_under_heavy_ties():
    rng = np.random.default_rng(2)
    n, nq = 500, 6
    K = rng.integers(-1, 2, (nq, n)).astype(np.float32)        # three key levels
    K[rng.random(K.shape) < 0.1] *= np.float32(-0.0)           # -0.0 == +0.0
    el = rng.random((nq, n)) < 0.8
    el[4] = False
    el[5, 10:] = False
    for refine in (1, 7, 256):
        cands, cc = sq8_ref.candidates(K, el, refine)
        assert cands.dtype == np.uint64 and cc.dtype == np.uint32
        for q in range(nq):
            want = sorted((i for i in range(n) if el[q, i]), key=lambda i: (-float(K[q, i]), i))[:refine]
            assert cc[q] == len(want) and cands[q, :cc[q]].tolist() == want and not cands[q, cc[q]:].any(), (refine, q)
    assert cc[4] == 0 and cc[5] == el[5].sum()


def test_reference_restricted_top_m():
    rng = np.random.default_rng(3)
    n, nq = 300, 4
    S = rng.integers(-2, 3, (nq, n)).astype(np.float32) * np.float32(0.25)
    cands = np.zeros((nq, 40), dtype=np.uint64)
    cc = np.array([40, 5, 0, 17], dtype=np.uint32)
    for q in range(nq):
        cands[q, :cc[q]] = rng.permutation(n)[:cc[q]]
    for M in (1, 10, 40):
        ids, sc, cnt = sq8_ref.restricted_top_m(S, cands, cc, M)
        for q in range(nq):
            want = sorted((int(i) for i in cands[q, :cc[q]]), key=lambda i: (-float(S[q, i]), i))[:M]
            assert cnt[q] == len(want) and ids[q, :cnt[q]].tolist() == want, (M, q)
            assert sc[q, :cnt[q]].tobytes() == S[q, want].tobytes() and np.isnan(sc[q, cnt[q]:]).all() and not ids[q, cnt[q]:].any()


def test_tight_case_defeats_the_codes():
    """the GPU test's data set: for every query and every refine of the test the true top-32 is not inside the coarse candidates"""
    X, Q = sq8_ref.tight_case()
    Xn, xbad = sq8_ref.normalised(X)
    Qn, qbad = sq8_ref.normalised(Q)
    assert not xbad.any() and not qbad.any()
    rc, rs = sq8_ref.codes(Xn)
    qc, _ = sq8_ref.codes(Qn)
    K = sq8_ref.keys(qc, rc, rs)
    S = Qn.astype(np.float64) @ Xn.astype(np.float64).T
    for R in (32, 64, 256):
        cands, cc = sq8_ref.candidates(K, np.ones(K.shape, dtype=bool), R)
        for q in range(len(Q)):
            true = np.argsort(-S[q], kind="stable")[:32]
            assert not np.isin(true, cands[q]).all(), (R, q)


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^(?:bn_status|void|size_t) (bn_sq8_\w+)\(", header, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "typedef struct bn_sq8 bn_sq8;" in header and "pub struct bn_sq8" in ffi
    assert hasattr(bn, "Sq8") and all(hasattr(bn.Sq8, m) for m in ("extend", "read", "search", "search_ids", "rows"))


class Outs:
    """search outputs pre-filled with sentinels"""

    def __init__(self, nq=2, stride=4, refine=4):
        self.ids = np.full(nq * stride, 0xABCDEF, dtype=np.uint64)
        self.sc = np.full(nq * stride, -7.5, dtype=np.float32)
        self.cnt = np.full(nq, 77, dtype=np.uint32)
        self.cand = np.full(nq * refine, 0xFEDCBA, dtype=np.uint64)
        self.cc = np.full(nq, 99, dtype=np.uint32)
        self.before = self.bytes()

    def bytes(self):
        return tuple(a.tobytes() for a in (self.ids, self.sc, self.cnt, self.cand, self.cc))

    def args(self):
        return (self.ids.ctypes.data_as(u64p), self.sc.ctypes.data_as(f32p), self.cnt.ctypes.data_as(u32p), self.cand.ctypes.data_as(u64p),
                self.cc.ctypes.data_as(u32p))

    def untouched(self):
        return self.bytes() == self.before


def test_arguments_are_refused_before_any_device_call(bn):
    """these refusals need neither a view nor a device: they are the same with and without a GPU"""
    assert bn.lib.bn_sq8_build(None, None) == INVALID_ARG and bn.last_error()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    # (refine, top_m, m_stride, word of the message)
    for refine, top_m, stride, msg in ((0, 1, 4, "refine"), (257, 4, 4, "refine"), (4, 0, 4, "top_m"), (4, 5, 8, "top_m"), (256, 257, 300, "top_m"),
                                       (4, 4, 3, "m_stride")):
        o = Outs()
        assert bn.lib.bn_sq8_search(None, q.ctypes.data_as(f32p), 2, refine, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert bn.lib.bn_sq8_search_ids(None, qi.ctypes.data_as(u64p), 2, -1, refine, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert o.untouched()
    o = Outs()
    assert bn.lib.bn_sq8_search(None, None, 2, 4, 4, 4, *o.args()) == INVALID_ARG
    assert bn.lib.bn_sq8_search_ids(None, None, 2, -1, 4, 4, 4, *o.args()) == INVALID_ARG
    for null in range(3):
        a = list(o.args())
        a[null] = None
        assert bn.lib.bn_sq8_search(None, q.ctypes.data_as(f32p), 2, 4, 4, 4, *a) == INVALID_ARG
        assert bn.lib.bn_sq8_search_ids(None, qi.ctypes.data_as(u64p), 2, 0, 4, 4, 4, *a) == INVALID_ARG
    assert o.untouched()
    # the calls that need no device
    assert bn.lib.bn_sq8_rows(None) == 0
    bn.lib.bn_sq8_free(None)


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    h = C.c_void_p(0x1234)
    assert bn.lib.bn_sq8_build(None, C.byref(h)) == NO_DEVICE and "gfx950" in bn.last_error()
    assert h.value == 0x1234
    assert bn.lib.bn_sq8_extend(None) == NO_DEVICE
    codes = np.full(8, 55, dtype=np.int8)
    scales = np.full(2, -7.5, dtype=np.float32)
    assert bn.lib.bn_sq8_read(None, 0, 2, codes.ctypes.data_as(i8p), scales.ctypes.data_as(f32p)) == NO_DEVICE
    assert (codes == 55).all() and (scales == -7.5).all()
    o = Outs()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    assert bn.lib.bn_sq8_search(None, q.ctypes.data_as(f32p), 2, 4, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert bn.lib.bn_sq8_search_ids(None, qi.ctypes.data_as(u64p), 2, 0, 4, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert o.untouched()
