"""bn_ivf_* without a GPU: the header, the library, the harness and the Rust bindings agree on every entry point; arguments that need
no view are refused before the device is asked for; without a device the calls refuse with the no-device status and leave the
caller's outputs alone; and the numpy rules of tests/ivf_ref.py agree with brute force on hand-made cases.

The ivf_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cluster_ref
import index_ref as ir
import ivf_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NONE = ivf_ref.NONE
NAMES = ("bn_ivf_build", "bn_ivf_free", "bn_ivf_lists", "bn_ivf_rows", "bn_ivf_extend", "bn_ivf_list_sizes", "bn_ivf_read_list", "bn_ivf_search",
         "bn_ivf_search_ids")
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^(?:bn_status|void|size_t) (bn_ivf_\w+)\(", header, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "typedef struct bn_ivf bn_ivf;" in header and "pub struct bn_ivf" in ffi
    assert re.search(r"#define\s+BN_ABI_VERSION\s+2\b", header) and bn.lib.bn_abi_version() == 2
    assert hasattr(bn, "Ivf") and all(hasattr(bn.Ivf, m) for m in ("extend", "list_sizes", "read_list", "search", "search_ids", "rows"))


class Outs:
    """search outputs pre-filled with sentinels"""

    def __init__(self, nq=2, stride=4, nprobe=2):
        self.ids = np.full(nq * stride, 0xABCDEF, dtype=np.uint64)
        self.sc = np.full(nq * stride, -7.5, dtype=np.float32)
        self.cnt = np.full(nq, 77, dtype=np.uint32)
        self.pr = np.full(nq * nprobe, 0xDEADBEEF, dtype=np.uint32)
        self.scn = np.full(nq, 99, dtype=np.uint64)
        self.before = self.bytes()

    def bytes(self):
        return tuple(a.tobytes() for a in (self.ids, self.sc, self.cnt, self.pr, self.scn))

    def args(self):
        return (self.ids.ctypes.data_as(u64p), self.sc.ctypes.data_as(f32p), self.cnt.ctypes.data_as(u32p), self.pr.ctypes.data_as(u32p),
                self.scn.ctypes.data_as(u64p))

    def untouched(self):
        return self.bytes() == self.before


def test_arguments_are_refused_before_any_device_call(bn):
    """these refusals need neither a view nor a device: they are the same with and without a GPU"""
    cent = np.ones(8, dtype=np.float32)
    h = C.c_void_p(0x1234)
    for k in (0, 1025):
        assert bn.lib.bn_ivf_build(None, cent.ctypes.data_as(f32p), k, C.byref(h)) == INVALID_ARG and "k must be in 1..1024" in bn.last_error()
    assert bn.lib.bn_ivf_build(None, None, 2, C.byref(h)) == INVALID_ARG
    assert bn.lib.bn_ivf_build(None, cent.ctypes.data_as(f32p), 2, None) == INVALID_ARG
    assert h.value == 0x1234
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    for top_m, stride, msg in ((0, 4, "top_m"), (257, 300, "top_m"), (4, 3, "m_stride")):
        o = Outs()
        assert bn.lib.bn_ivf_search(None, q.ctypes.data_as(f32p), 2, 1, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert bn.lib.bn_ivf_search_ids(None, qi.ctypes.data_as(u64p), 2, -1, 1, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert o.untouched()
    o = Outs()
    assert bn.lib.bn_ivf_search(None, None, 2, 1, 4, 4, *o.args()) == INVALID_ARG
    assert bn.lib.bn_ivf_search_ids(None, None, 2, -1, 1, 4, 4, *o.args()) == INVALID_ARG
    assert bn.lib.bn_ivf_search(None, q.ctypes.data_as(f32p), 2, 1, 4, 4, None, o.sc.ctypes.data_as(f32p), o.cnt.ctypes.data_as(u32p), None, None) == INVALID_ARG
    assert o.untouched()
    # the calls that need no device
    sizes = np.full(3, 5, dtype=np.uint32)
    assert bn.lib.bn_ivf_list_sizes(None, sizes.ctypes.data_as(u32p)) == INVALID_ARG and sizes.tolist() == [5, 5, 5]
    assert bn.lib.bn_ivf_lists(None) == 0 and bn.lib.bn_ivf_rows(None) == 0
    bn.lib.bn_ivf_free(None)


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    cent = np.full(8, 3.5, dtype=np.float32)
    h = C.c_void_p(0x1234)
    assert bn.lib.bn_ivf_build(None, cent.ctypes.data_as(f32p), 2, C.byref(h)) == NO_DEVICE and "gfx950" in bn.last_error()
    assert h.value == 0x1234
    assert bn.lib.bn_ivf_extend(None) == NO_DEVICE
    ids = np.full(4, 0xABCDEF, dtype=np.uint64)
    n = C.c_size_t(55)
    assert bn.lib.bn_ivf_read_list(None, 0, ids.ctypes.data_as(u64p), 4, C.byref(n)) == NO_DEVICE
    assert n.value == 55 and (ids == 0xABCDEF).all()
    o = Outs()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    assert bn.lib.bn_ivf_search(None, q.ctypes.data_as(f32p), 2, 2, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert bn.lib.bn_ivf_search_ids(None, qi.ctypes.data_as(u64p), 2, 0, 2, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert o.untouched()


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def _brute_probes(Z, nprobe, qvalid):
    out = []
    for q in range(len(Z)):
        row = [NONE] * nprobe
        if qvalid[q]:
            left = [c for c in range(Z.shape[1]) if not math.isnan(float(Z[q, c]))]
            for slot in range(nprobe):
                if not left:
                    break
                best = left[0]
                for c in left[1:]:
                    if float(Z[q, c]) > float(Z[q, best]):  # strictly larger: the lowest index keeps a tie, -0.0 == +0.0
                        best = c
                row[slot] = best
                left.remove(best)
        out.append(row)
    return np.array(out, dtype=np.uint32).reshape(len(Z), nprobe)


def test_reference_probes_hand_made_cases():
    nan, inf = float("nan"), float("inf")
    Z = np.array([[1.0, 2.0, 2.0, 0.5, 2.0],      # ties between centroids: index order
                  [-0.0, 0.0, -1.0, 0.0, -0.0],   # -0.0 == +0.0
                  [nan, 3.0, nan, -inf, nan],     # fewer non-NaN scores than nprobe
                  [nan, nan, nan, nan, nan],      # nothing to probe
                  [5.0, 4.0, 3.0, 2.0, 1.0],      # an invalid query below
                  [inf, -inf, inf, 0.0, nan]], dtype=np.float32)
    qvalid = [1, 1, 1, 1, 0, 1]
    for nprobe in (1, 2, 3, 5):
        got = ivf_ref.probes(Z, nprobe, qvalid)
        assert got.dtype == np.uint32 and np.array_equal(got, _brute_probes(Z, nprobe, qvalid)), nprobe
    P = ivf_ref.probes(Z, 5, qvalid)
    assert P.tolist() == [[1, 2, 4, 0, 3], [0, 1, 3, 4, 2], [1, 3, NONE, NONE, NONE], [NONE] * 5, [NONE] * 5, [0, 2, 3, 1, NONE]]
    assert ivf_ref.scanned(P, [10, 0, 7, 1, 100]).tolist() == [118, 118, 1, 0, 0, 18]
    rng = np.random.default_rng(9)
    Z = rng.integers(-2, 3, (200, 9)).astype(np.float32) * np.float32(0.5)
    Z[rng.random(Z.shape) < 0.2] = np.nan
    Z[rng.random(Z.shape) < 0.1] *= np.float32(-0.0)
    qv = rng.random(200) < 0.9
    for nprobe in (1, 4, 9):
        assert np.array_equal(ivf_ref.probes(Z, nprobe, qv), _brute_probes(Z, nprobe, qv))


def _brute_top(S, qbad, xbad, assign, P, M, excluded, covered):
    out = []
    for q in range(S.shape[0]):
        rows = []
        if not qbad[q]:
            lists = set(int(c) for c in P[q] if c != NONE)
            rows = [i for i in range(min(S.shape[1], covered)) if int(assign[i]) in lists and not xbad[i] and not (excluded is not None and excluded[q, i])]
            rows.sort(key=lambda i: (-float(S[q, i]), i))
        out.append(rows[:M])
    return out


def test_reference_restricted_top_m():
    """an empty probed list, heavy score ties across lists, an exclusion mask, rows past `covered`, a NONE row, an invalid row"""
    rng = np.random.default_rng(10)
    n, k, nq = 300, 6, 7
    S = rng.integers(-1, 2, (nq, n)).astype(np.float32) * np.float32(0.5)   # three score levels: nearly everything ties
    assign = rng.integers(0, k - 1, n).astype(np.uint32)                    # list 5 is empty
    assign[rng.random(n) < 0.05] = NONE
    xbad = rng.random(n) < 0.05
    qbad = np.zeros(nq, dtype=bool)
    qbad[3] = True
    Z = rng.integers(-1, 2, (nq, k)).astype(np.float32)
    Z[:, 5] = 9.0                                                           # the empty list ranks first and uses a slot
    Z[6, 1] = np.nan
    excluded = rng.random((nq, n)) < 0.1
    for nprobe in (1, 2, 6):
        P = ivf_ref.probes(Z, nprobe, ~qbad)
        assert (P[~qbad, 0] == 5).all() and (P[3] == NONE).all()
        for M, ex, covered in ((1, None, n), (40, None, n), (256, excluded, n), (40, excluded, 150)):
            ids, sc, cnt = ivf_ref.restricted_top_m(S, qbad, xbad, assign, P, M, ex, covered)
            want = _brute_top(S, qbad, xbad, assign, P, M, ex, covered)
            for q in range(nq):
                assert cnt[q] == len(want[q]) and ids[q, :cnt[q]].tolist() == want[q], (nprobe, M, q)
                assert sc[q, :cnt[q]].tobytes() == S[q, want[q]].tobytes() and np.isnan(sc[q, cnt[q]:]).all()
            if nprobe == 1:
                assert not cnt.any()                                        # only the empty list was probed
    # nprobe == k without NONE rows and without NaN centroid scores is the unrestricted top-M
    assign = rng.integers(0, k, n).astype(np.uint32)
    P = ivf_ref.probes(np.nan_to_num(Z), k, ~qbad)                          # with a NaN score query 6 would leave list 1 out
    got = ivf_ref.restricted_top_m(S, qbad, xbad, assign, P, 64)
    want = ir.top_m_from_scores(S, qbad, xbad, 64)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("dim", [130, 1536])
def test_skewed_case_reaches_its_structure(dim):
    """the GPU test's data set: float32 products assign every row to the list it was drawn for, with margins no rounding can close"""
    X, cent, sizes, Q = ivf_ref.skewed_case(dim)
    with np.errstate(all="ignore"):
        U = (X / np.sqrt((X.astype(np.float64) ** 2).sum(axis=1, keepdims=True))).astype(np.float32)
    valid = np.isfinite(X).all(axis=1) & (X != 0).any(axis=1)
    assert (~valid).sum() == 3 and not valid[-3:].any()
    Z = U @ cent.T
    a, s = cluster_ref.assign(np.where(valid[:, None], Z, 0).astype(np.float32), valid)
    assert np.bincount(a[valid], minlength=12).tolist() == sizes.tolist()
    assert sorted(sizes.tolist())[:4] == [0, 0, 1, 10] and 64 in sizes and 65 in sizes and sizes.max() > 4900
    Zv = np.sort(Z[valid], axis=1)
    assert (Zv[:, -1] - Zv[:, -2]).min() > 0.5     # the winner leads by half a unit; an f32 chain's error is below 1e-4
    assert (a[~valid] == NONE).all()
