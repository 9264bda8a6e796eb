"""bn_index_search_seq without a GPU: the numpy rule of tests/seq_ref.py against a float64 brute force on dyadic scores (where both are
exact) and, at seq_len 1, against tests/peaks_ref.py; the plan arithmetic of csrc/seq_plan.h under ASan / UBSan (tools/asan_seq_plan.cpp);
the header, the library, the harness and the Rust bindings agree on the new names; arguments that need no index are refused before the
device is asked for; without a device the calls refuse with the no-device status and leave the caller's outputs alone.

The seq_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import peaks_ref
import seq_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NAMES = ("bn_index_search_seq", "bn_index_search_seq_ids")
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def brute_force(S, qbad, xbad, L, radius, M, first_ids=None, ex=-1):
    """the header's sentences one start at a time, in float64: [(ids, scores)] per sequence"""
    n = S.shape[1]
    out = []
    for p in range(S.shape[0] // L):
        W = S[p * L:(p + 1) * L].astype(np.float64)
        score, el = {}, set()
        for i in range(n):
            if i + L > n or any(xbad[i + j] for j in range(L)) or qbad[p * L:(p + 1) * L].any():
                continue
            if first_ids is not None and ex >= 0 and abs(i - int(first_ids[p])) <= ex:
                continue
            el.add(i)
            score[i] = sum(W[j, i + j] for j in range(L)) / L
        before = lambda a, b: score[a] > score[b] or (score[a] == score[b] and a < b)
        hits = [i for i in sorted(el) if all(not (j in el and before(j, i)) for j in range(i - radius, i + radius + 1) if j != i)]
        hits.sort(key=lambda i: (-score[i], i))
        out.append((hits[:M], [score[i] for i in hits[:M]]))
    return out


def dyadic_case(seed, n_seq, L, n):
    """window scores k / 64 with |k| <= 64: every partial sum is exact in float32, and so is the mean when L is a power of two"""
    rng = np.random.default_rng(seed)
    S = (rng.integers(-64, 65, (n_seq * L, n)) / 64.0).astype(np.float32)
    k = S[:, 1::5].shape[1]
    S[:, 0:5 * k:5] = S[:, 1::5]                             # neighbouring ties
    xbad = rng.random(n) < 0.03
    qbad = np.zeros(n_seq * L, dtype=bool)
    if n_seq > 2:
        qbad[2 * L + L // 2] = True                          # one sequence with an invalid window
    return S, qbad, xbad


@pytest.mark.parametrize("L", [1, 2, 4, 8, 64])
def test_reference_equals_a_float64_brute_force_where_both_are_exact(L):
    for n in (L - 1, L, L + 1, 150):
        if n < 1:
            continue
        S, qbad, xbad = dyadic_case(100 + L, 3, L, n)
        for radius in (0, 1, 5, 64):
            for M in (1, 256):
                ids, sc, cnt = seq_ref.seq_top_m(S, qbad, xbad, L, radius, M)
                assert ids.dtype == np.uint64 and sc.dtype == np.float32 and cnt.dtype == np.uint32 and ids.shape == sc.shape == (3, M)
                for p, (wi, ws) in enumerate(brute_force(S, qbad, xbad, L, radius, M)):
                    assert cnt[p] == len(wi) and ids[p, :cnt[p]].tolist() == wi, (L, n, radius, M, p)
                    assert sc[p, :cnt[p]].astype(np.float64).tolist() == ws, "a dyadic mean over a power of two is exact in both"
                assert cnt[2] == 0, "an invalid window: the sequence returns nothing"
                if n < L:
                    assert not cnt.any()
                if n == L:
                    assert (cnt[:2] == (0 if xbad[:L].any() else 1)).all()


@pytest.mark.parametrize("L", [3, 5, 33])
def test_reference_order_equals_the_brute_force_at_other_lengths(L):
    """1 / L is rounded, so only the order is compared: the exact sums differ by at least 1 / 64, far more than the rounding moves them"""
    S, qbad, xbad = dyadic_case(200 + L, 3, L, 200)
    fi = [0, 90, 200 - L]
    for radius in (0, 2, 64):
        for ex in (-1, 0, L - 1):
            ids, sc, cnt = seq_ref.seq_top_m(S, qbad, xbad, L, radius, 256, fi, ex)
            for p, (wi, ws) in enumerate(brute_force(S, qbad, xbad, L, radius, 256, fi, ex)):
                assert cnt[p] == len(wi) and ids[p, :cnt[p]].tolist() == wi, (L, radius, ex, p)
                assert np.abs(sc[p, :cnt[p]].astype(np.float64) - np.array(ws)).max(initial=0) <= 2.0 ** -22
                if ex >= 0:
                    assert not (np.abs(ids[p, :cnt[p]].astype(np.int64) - fi[p]) <= ex).any()


def test_the_chain_is_float32_in_window_order():
    """three scores whose float32 sum depends on the order: (2^24 + 1) + -2^24 is 0 in float32 when added in j order, 1 in float64"""
    S = np.zeros((3, 3), dtype=np.float32)
    S[0, 0], S[1, 1], S[2, 2] = 2.0 ** 24, 1.0, -2.0 ** 24
    score, ok = seq_ref.seq_scores(S, np.zeros(3, dtype=bool), 3)
    assert ok.tolist() == [True, False, False] and score[0] == 0.0
    inv = np.float32(1) / np.float32(3)
    S[0, 0], S[1, 1], S[2, 2] = 0.25, 0.5, 0.125
    assert seq_ref.seq_scores(S, np.zeros(3, dtype=bool), 3)[0][0].tobytes() == (np.float32(0.875) * inv).tobytes()
    assert (np.float32(0.875) * inv).tobytes() != np.float32(0.875 / 3).tobytes(), "multiplying by the rounded reciprocal is not dividing"


def test_length_one_is_the_peaks_reference():
    rng = np.random.default_rng(5)
    S = rng.standard_normal((6, 300)).astype(np.float32)
    S[:, ::7] = np.round(S[:, ::7])
    S[rng.random(S.shape) < 0.05] *= np.float32(-0.0)
    xbad = rng.random(300) < 0.1
    qbad = np.array([False, True, False, False, False, False])
    qi = [0, 5, 150, 299, 64, 63]
    for radius in (0, 1, 2, 64):
        for ex in (None, -1, 0, 3):
            el = peaks_ref.eligibility(300, qbad, xbad, None if ex is None else qi, -1 if ex is None else ex)
            want = peaks_ref.peaks_top_m(S, el, radius, 256)
            got = seq_ref.seq_top_m(S, qbad, xbad, 1, radius, 256, None if ex is None else qi, -1 if ex is None else ex)
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes(), (radius, ex)


def test_an_invalid_row_removes_exactly_the_starts_that_cover_it():
    L, n = 4, 40
    S = np.full((L, n), 0.5, dtype=np.float32)
    xbad = np.zeros(n, dtype=bool)
    xbad[20] = True
    score, ok = seq_ref.seq_scores(S, xbad, L)
    assert np.flatnonzero(~ok).tolist() == [17, 18, 19, 20, 37, 38, 39]
    ids, _, cnt = seq_ref.seq_top_m(S, np.zeros(L, dtype=bool), xbad, L, 3, 256)
    assert ids[0, :cnt[0]].tolist() == [0, 21], "start 21 has no eligible start within 3 before it: the removed starts suppress nobody"


# ---- the plan arithmetic under the sanitizers -------------------------------------------------------------------------------------
def test_plan_and_refusals_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path / "asan_seq_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_seq_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the plan check failed:\n" + r.stderr[-3000:])
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"\d+ plans, 0 failures", r.stdout), r.stdout


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^bn_status (bn_index_search_seq\w*)\(", header, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "#define BN_SEQ_LEN_MAX 64" in header and "pub const BN_SEQ_LEN_MAX: usize = 64;" in ffi and bn.BN_SEQ_LEN_MAX == 64
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert all(hasattr(bn.Index, m) for m in ("search_seq", "search_seq_ids"))


class Outs:
    """search outputs pre-filled with sentinels"""

    def __init__(self, nq=2, stride=4):
        self.ids = np.full(nq * stride, 0xABCDEF, dtype=np.uint64)
        self.sc = np.full(nq * stride, -7.5, dtype=np.float32)
        self.cnt = np.full(nq, 77, dtype=np.uint32)
        self.before = self.bytes()

    def bytes(self):
        return tuple(a.tobytes() for a in (self.ids, self.sc, self.cnt))

    def args(self):
        return (self.ids.ctypes.data_as(u64p), self.sc.ctypes.data_as(f32p), self.cnt.ctypes.data_as(u32p))

    def untouched(self):
        return self.bytes() == self.before


def test_arguments_are_refused_before_any_device_call(bn):
    """these refusals need neither an index nor a device: they are the same with and without a GPU"""
    q = np.ones(2 * 3 * 8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    qp, qip = q.ctypes.data_as(f32p), qi.ctypes.data_as(u64p)
    o = Outs()
    for L, radius, top_m, stride, msg in ((3, 65, 4, 4, "peak_radius"), (3, 1 << 40, 4, 4, "peak_radius"), (3, 2, 0, 4, "top_m"), (3, 2, 257, 300, "top_m"),
                                          (3, 2, 4, 3, "m_stride"), (0, 2, 4, 4, "seq_len"), (65, 0, 4, 4, "seq_len"), (1 << 40, 0, 4, 4, "seq_len"),
                                          (0, 65, 0, 0, "top_m"), (0, 65, 4, 4, "seq_len")):
        assert bn.lib.bn_index_search_seq(None, qp, 2, L, radius, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error(), (L, radius, top_m, stride)
        assert bn.lib.bn_index_search_seq_ids(None, qip, 2, L, -1, radius, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert o.untouched()
    assert bn.lib.bn_index_search_seq(None, None, 2, 3, 2, 4, 4, *o.args()) == INVALID_ARG and "null" in bn.last_error()
    assert bn.lib.bn_index_search_seq_ids(None, None, 2, 3, -1, 2, 4, 4, *o.args()) == INVALID_ARG and "null" in bn.last_error()
    for null in range(3):
        a = list(o.args())
        a[null] = None
        for radius in (0, 2, 64):
            assert bn.lib.bn_index_search_seq(None, qp, 2, 3, radius, 4, 4, *a) == INVALID_ARG and "null" in bn.last_error()
            assert bn.lib.bn_index_search_seq_ids(None, qip, 2, 3, 0, radius, 4, 4, *a) == INVALID_ARG and "null" in bn.last_error()
    assert o.untouched()


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    o = Outs()
    q = np.ones(2 * 3 * 8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    for L, radius in ((1, 0), (3, 0), (3, 1), (64, 64)):
        qq = np.ones(2 * L * 8, dtype=np.float32)
        assert bn.lib.bn_index_search_seq(None, qq.ctypes.data_as(f32p), 2, L, radius, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
        assert bn.lib.bn_index_search_seq_ids(None, qi.ctypes.data_as(u64p), 2, L, 0, radius, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert o.untouched() and q.size == 48
