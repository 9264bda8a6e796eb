"""bn_index_assign / bn_index_cluster without a GPU: the header, the library, the harness and the Rust bindings agree on both entry
points and on BN_CLUSTER_NONE at ABI version 2; without a device both calls refuse with the no-device status and leave the caller's
outputs alone; and the numpy rules of tests/cluster_ref.py agree with brute force on hand-made cases.

The cluster_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the
entry points and fail where the library lacks them."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cluster_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 9


def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in ("bn_index_assign", "bn_index_cluster"):
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert re.search(r"^bn_status %s\(" % name, header, flags=re.M)
        assert "pub fn %s(" % name in ffi
    assert re.search(r"#define\s+BN_CLUSTER_NONE\s+4294967295u", header)
    assert bn.BN_CLUSTER_NONE == 0xFFFFFFFF == cluster_ref.NONE
    assert "pub const BN_CLUSTER_NONE: u32 = 4294967295;" in ffi
    assert "pub struct bn_cluster_opts" in ffi and "pub struct bn_cluster_report" in ffi
    assert re.search(r"#define\s+BN_ABI_VERSION\s+2\b", header) and bn.lib.bn_abi_version() == 2
    # the harness's structs have the header's fields, in order
    for cname, pyname in (("bn_cluster_opts", "BnClusterOpts"), ("bn_cluster_report", "BnClusterReport")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, flags=re.S).group(1)
        fields = [re.search(r"(\w+)$", f.strip()).group(1) for f in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if f.strip()]
        assert fields == [f[0] for f in getattr(bn, pyname)._fields_], cname


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    cent = np.full(8, 3.5, dtype=np.float32)
    assign = np.full(6, 0xDEADBEEF, dtype=np.uint32)
    score = np.full(6, -7.5, dtype=np.float32)
    counts = np.full(2, 77, dtype=np.uint32)
    rep = bn.BnClusterReport(11, 12, 13, 14, 15.5, 16)
    before = cent.tobytes(), assign.tobytes(), score.tobytes(), counts.tobytes(), bytes(rep)
    st = bn.lib.bn_index_assign(None, cent.ctypes.data_as(f32p), 2, 0, 0, assign.ctypes.data_as(u32p), score.ctypes.data_as(f32p))
    assert st == NO_DEVICE and "gfx950" in bn.last_error()
    st = bn.lib.bn_index_cluster(None, 2, 0, 0, None, 0, cent.ctypes.data_as(f32p), assign.ctypes.data_as(u32p), score.ctypes.data_as(f32p),
                                 counts.ctypes.data_as(u32p), C.byref(rep), C.sizeof(rep))
    assert st == NO_DEVICE and "gfx950" in bn.last_error()
    assert (cent.tobytes(), assign.tobytes(), score.tobytes(), counts.tobytes(), bytes(rep)) == before


def _brute_assign(Z, valid):
    out_a, out_s = [], []
    for i in range(Z.shape[0]):
        best = None
        if valid[i]:
            for c in range(Z.shape[1]):
                z = float(Z[i, c])
                if math.isnan(z):
                    continue
                if best is None or z > float(Z[i, best]):  # strictly larger: the lowest index keeps a tie, -0.0 == +0.0
                    best = c
        out_a.append(cluster_ref.NONE if best is None else best)
        out_s.append(np.float32(np.nan) if best is None else Z[i, best])
    return np.array(out_a, dtype=np.uint32), np.array(out_s, dtype=np.float32)


def _check_assign(Z, valid):
    Z = np.asarray(Z, dtype=np.float32)
    valid = np.asarray(valid, dtype=bool)
    a, s = cluster_ref.assign(Z, valid)
    wa, ws = _brute_assign(Z, valid)
    assert a.dtype == np.uint32 and s.dtype == np.float32
    assert np.array_equal(a, wa), (a, wa)
    assert s.tobytes() == ws.tobytes(), (s, ws)
    return a, s


def test_reference_assign_hand_made_cases():
    nan, inf = float("nan"), float("inf")
    Z = np.array([[1.0, 2.0, 2.0, 0.5],      # a tie: the lowest index
                  [-0.0, 0.0, -1.0, -2.0],   # -0.0 == +0.0: index 0, and the score keeps its sign bit
                  [0.0, -0.0, -1.0, nan],
                  [nan, -inf, -inf, nan],    # -inf beats NaN; among equals the first
                  [nan, nan, nan, nan],      # all NaN: NONE
                  [3.0, 2.0, 1.0, 0.0],      # an invalid row below
                  [nan, 1.0, inf, inf],
                  [-1.0, nan, -1.0, -1.0]], dtype=np.float32)
    valid = [1, 1, 1, 1, 1, 0, 1, 1]
    a, s = _check_assign(Z, valid)
    assert a.tolist() == [1, 0, 0, 1, cluster_ref.NONE, cluster_ref.NONE, 2, 0]
    assert np.signbit(s[1]) and not np.signbit(s[2]) and np.isnan(s[4]) and np.isnan(s[5])
    _check_assign(Z[:, 3:], valid)           # a NaN column alone: k = 1
    _check_assign(Z[:, ::-1], valid)
    _check_assign(Z, np.zeros(8))


def test_reference_assign_random_with_heavy_ties():
    rng = np.random.default_rng(5)
    Z = rng.integers(-2, 3, (300, 7)).astype(np.float32) * np.float32(0.5)
    Z[rng.random(Z.shape) < 0.2] = np.nan
    Z[rng.random(Z.shape) < 0.1] *= np.float32(-0.0)
    Z[rng.random(Z.shape) < 0.02] = -np.inf
    _check_assign(Z, rng.random(300) < 0.9)


def test_reference_update_against_fsum():
    rng = np.random.default_rng(6)
    n, dim, k = 200, 5, 4
    S = (rng.standard_normal((n, dim)) * 10.0 ** rng.integers(-3, 4, (n, 1))).astype(np.float32)
    a = rng.integers(0, 3, n).astype(np.uint32)      # cluster 3 has no members
    a[rng.random(n) < 0.1] = cluster_ref.NONE
    prev = rng.standard_normal((k, dim)).astype(np.float32)
    got, kept = cluster_ref.update(S, a, prev)
    sums, counts, mags = cluster_ref.member_sums(S, a, k)
    assert kept.tolist() == [False, False, False, True] and got[3].tobytes() == prev[3].tobytes()
    assert counts.tolist() == [int((a == c).sum()) for c in range(k)]
    for c in range(3):
        m = np.flatnonzero(a == c)
        exact = np.array([math.fsum(float(v) for v in S[m, j]) for j in range(dim)])
        assert np.all(np.abs(sums[c] - exact) <= len(m) * 2.0 ** -53 * mags[c])
        want = exact / math.sqrt(math.fsum(float(v) * float(v) for v in exact))
        assert np.all(np.abs(got[c].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + len(m) * 2.0 ** -52 * mags[c] / np.sqrt((exact ** 2).sum()))
    c64, bound = cluster_ref.update_bound(S, a, k)
    assert np.isinf(bound[3]).all() and np.all(np.abs(got[:3] - c64[:3]) <= bound[:3])
    # dyadic members: every order gives the same sums, exactly
    D = np.array([[0.5, -0.25], [0.25, 0.25], [1.0, 0.0], [-0.5, 2.0]], dtype=np.float32)
    sums, counts, _ = cluster_ref.member_sums(D, [0, 1, 0, 0], 2)
    assert sums.tolist() == [[1.0, 1.75], [0.25, 0.25]] and counts.tolist() == [3, 1]
    # a zero sum keeps the previous centroid
    Zs = np.array([[1.0, 0.0], [-1.0, 0.0], [3e38, 0.0], [3e38, 0.0]], dtype=np.float32)
    p = np.array([[0.6, 0.8], [0.0, 1.0]], dtype=np.float32)
    got, kept = cluster_ref.update(Zs, [0, 0, 1, 1], p)
    assert kept.tolist() == [True, False] and got[0].tobytes() == p[0].tobytes() and got[1].tolist() == [1.0, 0.0]
