"""bn_index_search_peaks without a GPU: the numpy rule of tests/peaks_ref.py against a brute-force double loop and against the
consequences include/birdnet_hip.h states; the header, the library, the harness and the Rust bindings agree on the new names; arguments
that need no index are refused before the device is asked for; without a device the calls refuse with the no-device status and leave the
caller's outputs alone.

The peaks_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import peaks_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NAMES = ("bn_index_search_peaks", "bn_index_search_peaks_ids")
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def brute_force(S, eligible, radius, M):
    """the header's sentences one pair at a time: [(ids, scores)] per query"""
    out = []
    nq, n = S.shape
    for q in range(nq):
        def before(j, i):                                   # j comes before i in the index's total order
            a, b = float(S[q, j]), float(S[q, i])
            return a > b or (a == b and j < i)
        peaks = []
        for i in range(n):
            if not eligible[q, i]:
                continue
            if all(not (eligible[q, j] and before(j, i)) for j in range(max(0, i - radius), min(n, i + radius + 1)) if j != i):
                peaks.append(i)
        peaks.sort(key=lambda i: (-float(S[q, i]), i))
        out.append(peaks[:M])
    return out


def check_against_brute_force(S, eligible, radii, Ms):
    for radius in radii:
        for M in Ms:
            ids, sc, cnt = peaks_ref.peaks_top_m(S, eligible, radius, M)
            assert ids.dtype == np.uint64 and sc.dtype == np.float32 and cnt.dtype == np.uint32
            assert ids.shape == sc.shape == (S.shape[0], M) and cnt.shape == (S.shape[0],)
            want = brute_force(S, eligible, radius, M)
            for q, w in enumerate(want):
                assert cnt[q] == len(w) and ids[q, :cnt[q]].tolist() == w, (radius, M, q)
                assert sc[q, :cnt[q]].tobytes() == S[q, w].astype(np.float32).tobytes()
                assert np.isnan(sc[q, cnt[q]:]).all() and not ids[q, cnt[q]:].any()


def test_reference_equals_a_brute_force_double_loop_on_random_scores():
    rng = np.random.default_rng(11)
    for n in (1, 2, 7, 150):
        for dtype in (np.float32, np.float64):
            S = rng.standard_normal((4, n)).astype(dtype)
            el = rng.random((4, n)) < 0.85
            el[3] = False                                   # an invalid query: nothing is eligible
            check_against_brute_force(S, el, (0, 1, 2, 5, 64), (1, 3, 256))


def test_reference_equals_a_brute_force_double_loop_on_heavy_ties():
    rng = np.random.default_rng(12)
    n = 200
    S = rng.integers(-1, 2, (5, n)).astype(np.float32)     # three score levels
    S[rng.random(S.shape) < 0.2] *= np.float32(-0.0)       # -0.0 == +0.0
    el = rng.random((5, n)) < 0.8
    el[0] = True
    check_against_brute_force(S, el, (0, 1, 3, 10, 64), (1, 7, 256))


def random_case(seed=13, nq=6, n=400):
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((nq, n)).astype(np.float32)
    S[:, ::7] = np.round(S[:, ::7])                        # some exact ties
    el = rng.random((nq, n)) < 0.9
    return S, el


def test_returned_ids_are_more_than_the_radius_apart():
    S, el = random_case()
    for radius in (1, 2, 8, 64):
        ids, _, cnt = peaks_ref.peaks_top_m(S, el, radius, 256)
        for q in range(len(S)):
            got = np.sort(ids[q, :cnt[q]].astype(np.int64))
            assert cnt[q] > 0 and (np.diff(got) > radius).all(), (radius, q)
            assert el[q, got].all(), "an ineligible row was returned"


def test_radius_zero_is_the_plain_top_m():
    S, el = random_case()
    for M in (1, 10, 256):
        ids, sc, cnt = peaks_ref.peaks_top_m(S, el, 0, M)
        for q in range(len(S)):
            c = np.flatnonzero(el[q])
            want = sorted(c.tolist(), key=lambda i: (-float(S[q, i]), i))[:M]
            assert cnt[q] == len(want) and ids[q, :cnt[q]].tolist() == want and sc[q, :cnt[q]].tobytes() == S[q, want].tobytes()


def test_a_monotone_ramp_has_one_peak():
    """greedy suppression would return the top and then one row every radius + 1 ids down the slope"""
    n = 300
    up = np.arange(n, dtype=np.float32)[None]
    el = np.ones((1, n), dtype=bool)
    for radius in (1, 2, 8, 64):
        ids, _, cnt = peaks_ref.peaks_top_m(up, el, radius, 256)
        assert cnt[0] == 1 and ids[0, 0] == n - 1, radius
        ids, _, cnt = peaks_ref.peaks_top_m(-up, el, radius, 256)
        assert cnt[0] == 1 and ids[0, 0] == 0, radius
    # a ramp cut by ineligible gaps wider than the radius: one peak per piece, its top
    el[0, 100:110] = False
    el[0, 200:203] = False
    ids, _, cnt = peaks_ref.peaks_top_m(up, el, 8, 256)
    assert ids[0, :cnt[0]].tolist() == [299, 99], "the three-row gap is bridged at radius 8, the ten-row gap is not"
    ids, _, cnt = peaks_ref.peaks_top_m(up, el, 2, 256)
    assert ids[0, :cnt[0]].tolist() == [299, 199, 99]


def test_a_run_of_exact_ties_has_one_peak_its_lowest_id():
    n = 300
    S = np.full((1, n), 0.5, dtype=np.float32)
    el = np.ones((1, n), dtype=bool)
    for radius in (1, 2, 64):
        ids, _, cnt = peaks_ref.peaks_top_m(S, el, radius, 256)
        assert ids[0, :cnt[0]].tolist() == [0], radius
    S[:] = -0.0
    S[0, ::2] = 0.0
    ids, _, cnt = peaks_ref.peaks_top_m(S, el, 3, 256)
    assert ids[0, :cnt[0]].tolist() == [0], "-0.0 and +0.0 tie"


def test_one_row_after_an_ineligible_gap_becomes_a_peak():
    """ineligible rows take no part: they are never peaks and never suppress a neighbour"""
    n = 40
    S = np.full((1, n), 1.0, dtype=np.float32)
    el = np.ones((1, n), dtype=bool)
    el[0, 10:13] = False                                   # rows 10..12 are out: with radius 3 row 13 has no eligible row before it
    S[0, 11] = 9.0                                         # the best score of all, ineligible: it suppresses nobody
    ids, _, cnt = peaks_ref.peaks_top_m(S, el, 3, 256)
    assert ids[0, :cnt[0]].tolist() == [0, 13]
    ids, _, cnt = peaks_ref.peaks_top_m(S, el, 4, 256)
    assert ids[0, :cnt[0]].tolist() == [0], "row 9 is within 4 of row 13"
    el[0, 11] = True
    ids, _, cnt = peaks_ref.peaks_top_m(S, el, 3, 256)
    assert ids[0, :cnt[0]].tolist() == [11, 0], "eligible again, row 11 suppresses 8..14"


def test_eligibility_of_the_two_calls():
    qbad, xbad = np.array([False, True, False]), np.zeros(10, dtype=bool)
    xbad[4] = True
    el = peaks_ref.eligibility(10, qbad, xbad)
    assert not el[1].any() and el[0].tolist() == [i != 4 for i in range(10)]
    el = peaks_ref.eligibility(10, qbad, xbad, [0, 5, 9], 1)
    assert np.flatnonzero(~el[0]).tolist() == [0, 1, 4] and np.flatnonzero(~el[2]).tolist() == [4, 8, 9]
    assert peaks_ref.eligibility(10, qbad, xbad, [0, 5, 9], -1).tobytes() == peaks_ref.eligibility(10, qbad, xbad).tobytes()


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^bn_status (bn_index_search_peaks\w*)\(", header, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "#define BN_PEAK_RADIUS_MAX 64" in header and "pub const BN_PEAK_RADIUS_MAX: usize = 64;" in ffi and bn.BN_PEAK_RADIUS_MAX == 64
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert all(hasattr(bn.Index, m) for m in ("search_peaks", "search_peaks_ids"))


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
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    qp, qip = q.ctypes.data_as(f32p), qi.ctypes.data_as(u64p)
    o = Outs()
    for radius, top_m, stride, msg in ((65, 4, 4, "peak_radius"), (1 << 40, 4, 4, "peak_radius"), (2, 0, 4, "top_m"), (2, 257, 300, "top_m"),
                                       (2, 4, 3, "m_stride"), (0, 0, 4, "top_m"), (0, 4, 3, "m_stride")):
        assert bn.lib.bn_index_search_peaks(None, qp, 2, radius, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error(), (radius, top_m, stride)
        assert bn.lib.bn_index_search_peaks_ids(None, qip, 2, -1, radius, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert o.untouched()
    assert bn.lib.bn_index_search_peaks(None, None, 2, 2, 4, 4, *o.args()) == INVALID_ARG and "null" in bn.last_error()
    assert bn.lib.bn_index_search_peaks_ids(None, None, 2, -1, 2, 4, 4, *o.args()) == INVALID_ARG and "null" in bn.last_error()
    for null in range(3):
        a = list(o.args())
        a[null] = None
        for radius in (0, 2, 64):
            assert bn.lib.bn_index_search_peaks(None, qp, 2, radius, 4, 4, *a) == INVALID_ARG and "null" in bn.last_error()
            assert bn.lib.bn_index_search_peaks_ids(None, qip, 2, 0, radius, 4, 4, *a) == INVALID_ARG and "null" in bn.last_error()
    assert o.untouched()


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    o = Outs()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    for radius in (0, 1, 64):
        assert bn.lib.bn_index_search_peaks(None, q.ctypes.data_as(f32p), 2, radius, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
        assert bn.lib.bn_index_search_peaks_ids(None, qi.ctypes.data_as(u64p), 2, 0, radius, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert o.untouched()
