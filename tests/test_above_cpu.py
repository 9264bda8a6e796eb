"""bn_index_search_above without a GPU: the numpy rule of tests/above_ref.py against a literal double loop over the header's sentences; the
header, the library, the harness and the Rust bindings agree on the new names; arguments that need no index are refused before the device
is asked for; without a device the calls refuse with the no-device status and leave the caller's outputs alone.

The above_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import above_ref
import index_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NAMES = ("bn_index_search_above", "bn_index_search_above_ids")
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
INF = float("inf")


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def double_loop(S, qbad, xbad, thr, lo, hi, qid, radius):
    """the header's sentences one pair at a time: [[(id, f32 score)]] per query, ids ascending because r ascends"""
    out = []
    for q in range(S.shape[0]):
        hits = []
        for r in range(S.shape[1]):
            if qbad[q] or xbad[r] or not lo <= r < hi:
                continue
            if qid is not None and radius >= 0 and abs(r - int(qid[q])) <= radius:
                continue
            if np.float32(S[q, r]) >= np.float32(thr[q]):
                hits.append((r, np.float32(S[q, r])))
        out.append(hits)
    return out


def small_case():
    """40 dyadic rows at known levels against 6 queries: query 0 is the canonical one, query 4 is invalid; row 7 is zeros, row 21 has a NaN"""
    rng = np.random.default_rng(5)
    lv = rng.integers(-16, 17, 40)
    lv[[3, 4, 5, 30]] = 8                                    # ties exactly at a threshold used below
    X = ir.rows_at_levels(rng, lv, 32, 16)
    X[7] = 0
    X[21, 2] = np.nan
    Q = np.concatenate([ir.canonical_query(32, 16)[None], ir.dyadic_rows(rng, 5, 32, 16)])
    Q[4] = 0
    S, qbad, xbad = ir.scores64(Q, X)
    assert qbad.tolist() == [False] * 4 + [True, False] and np.flatnonzero(xbad).tolist() == [7, 21]
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S), "dyadic scores are exact in f32"
    return S, qbad, xbad, lv


def test_reference_equals_a_literal_double_loop():
    S, qbad, xbad, lv = small_case()
    nq, n = S.shape
    thresholds = [np.full(nq, 0.5), np.full(nq, -INF), np.full(nq, INF), np.array([0.5, 0.0, -0.25, 1.0, 0.0, -INF]), np.full(nq, 0.5 - 2.0 ** -20)]
    qid = np.array([0, 3, 4, 39, 7, 20])
    for thr in thresholds:
        for first, cnt in ((0, 0), (0, n), (3, 3), (4, 27), (39, 0), (n, 0), (5, 1)):
            for ids, radius in ((None, -1), (qid, -1), (qid, 0), (qid, 2), (qid, 100)):
                lo, hi = above_ref.id_range(n, first, cnt)
                want = double_loop(S, qbad, xbad, thr, lo, hi, ids, radius)
                got = above_ref.hits_from_scores(S, qbad, xbad, thr, first, cnt, ids, radius)
                for q in range(nq):
                    assert got[q][0].tolist() == [r for r, _ in want[q]], (thr[q], first, cnt, radius, q)
                    assert got[q][1].tobytes() == np.array([s for _, s in want[q]], dtype=np.float32).tobytes()
                    assert got[q][1].dtype == np.float32 and (np.diff(got[q][0]) > 0).all()


def test_ties_at_the_threshold_are_hits_and_one_level_below_is_not():
    S, qbad, xbad, lv = small_case()
    at = above_ref.hits_from_scores(S[:1], qbad[:1], xbad, 8 / 16)[0][0]
    assert at.tolist() == [r for r in range(40) if lv[r] >= 8 and r not in (7, 21)] and {3, 4, 5, 30} <= set(at.tolist())
    just_above = above_ref.hits_from_scores(S[:1], qbad[:1], xbad, np.nextafter(np.float32(0.5), np.float32(1)))[0][0]
    assert just_above.tolist() == [r for r in range(40) if lv[r] > 8 and r not in (7, 21)]


def test_infinite_thresholds_invalid_rows_and_invalid_queries():
    S, qbad, xbad, _ = small_case()
    every = above_ref.hits_from_scores(S, qbad, xbad, -INF)
    none = above_ref.hits_from_scores(S, qbad, xbad, INF)
    valid = [r for r in range(40) if r not in (7, 21)]
    for q in range(6):
        assert every[q][0].tolist() == ([] if q == 4 else valid) and len(none[q][0]) == 0
    ranged = above_ref.hits_from_scores(S, qbad, xbad, -INF, 5, 20)
    assert ranged[0][0].tolist() == [r for r in range(5, 25) if r not in (7, 21)]
    with pytest.raises(AssertionError):
        above_ref.hits_from_scores(S, qbad, xbad, np.nan)
    for first, cnt in ((41, 0), (0, 41), (39, 2)):
        with pytest.raises(ValueError):
            above_ref.id_range(40, first, cnt)


def test_truncation_keeps_the_first_hits_and_the_total_count():
    S, qbad, xbad, _ = small_case()
    hits = above_ref.hits_from_scores(S, qbad, xbad, -0.25)
    tags = np.arange(40, dtype=np.uint32) * 3 + 1
    for max_hits, stride in ((0, 0), (1, 1), (5, 5), (5, 8), (64, 64)):
        ids, sc, tg, cnt = above_ref.layout(hits, max_hits, stride, tags)
        assert ids.shape == sc.shape == tg.shape == (6, stride) and ids.dtype == np.uint64 and sc.dtype == np.float32 and tg.dtype == cnt.dtype == np.uint32
        for q in range(6):
            k = min(len(hits[q][0]), max_hits)
            assert cnt[q] == len(hits[q][0]) and ids[q, :k].tolist() == hits[q][0][:k].tolist() and sc[q, :k].tobytes() == hits[q][1][:k].tobytes()
            assert tg[q, :k].tolist() == (3 * hits[q][0][:k] + 1).tolist()
            assert not ids[q, k:].any() and np.isnan(sc[q, k:]).all() and not tg[q, k:].any()
    assert max(len(h[0]) for h in hits) > 5, "the case must truncate"
    assert not above_ref.layout(hits, 5)[2].any(), "an index that never tagged gives zeros"
    # paging from the last returned id + 1 reproduces the list
    full = hits[0][0]
    got, first = [], 0
    while True:
        ids, _, _, cnt = above_ref.layout(above_ref.hits_from_scores(S[:1], qbad[:1], xbad, -0.25, first, 0), 4)
        k = min(int(cnt[0]), 4)
        got += ids[0, :k].tolist()
        if cnt[0] <= 4:
            break
        first = int(ids[0, k - 1]) + 1
    assert got == full.tolist()


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^bn_status (bn_index_search_above\w*)\(", header, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "#define BN_ABOVE_MAX_HITS 65536u" in header and "pub const BN_ABOVE_MAX_HITS: u32 = 65536;" in ffi and bn.BN_ABOVE_MAX_HITS == 65536
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert all(hasattr(bn.Index, m) for m in ("search_above", "search_above_ids", "count_above"))


class Outs:
    """outputs pre-filled with sentinels"""

    def __init__(self, nq=2, stride=4):
        self.ids = np.full(nq * stride, 0xABCDEF, dtype=np.uint64)
        self.sc = np.full(nq * stride, -7.5, dtype=np.float32)
        self.tg = np.full(nq * stride, 0xBEEF, dtype=np.uint32)
        self.cnt = np.full(nq, 77, dtype=np.uint32)
        self.before = self.bytes()

    def bytes(self):
        return tuple(a.tobytes() for a in (self.ids, self.sc, self.tg, self.cnt))

    def args(self):
        return (self.ids.ctypes.data_as(u64p), self.sc.ctypes.data_as(f32p), self.tg.ctypes.data_as(u32p), self.cnt.ctypes.data_as(u32p))

    def untouched(self):
        return self.bytes() == self.before


def both(bn, queries, ids, n, thr, first, n_ids, max_hits, stride, outs):
    """the two entry points with the same arguments: (status, message) of each"""
    a = bn.lib.bn_index_search_above(None, queries, n, thr, first, n_ids, max_hits, stride, *outs)
    ma = bn.last_error()
    b = bn.lib.bn_index_search_above_ids(None, ids, n, -1, thr, first, n_ids, max_hits, stride, *outs)
    return (a, ma), (b, bn.last_error())


def test_arguments_are_refused_before_any_device_call(bn):
    """these refusals need neither an index nor a device: they are the same with and without a GPU"""
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    thr = np.array([0.5, 0.25], dtype=np.float32)
    qp, qip, tp = q.ctypes.data_as(f32p), qi.ctypes.data_as(u64p), thr.ctypes.data_as(f32p)
    o = Outs()

    def refused(msg, *a):
        for st, text in both(bn, *a):
            assert st == INVALID_ARG and msg in text, (msg, st, text)
        assert o.untouched()

    refused("max_hits", qp, qip, 2, tp, 0, 0, 65537, 65537, o.args())
    refused("max_hits", qp, qip, 2, tp, 0, 0, 1 << 40, 1 << 40, o.args())
    refused("h_stride", qp, qip, 2, tp, 0, 0, 4, 3, o.args())
    refused("null", None, None, 2, tp, 0, 0, 4, 4, o.args())
    refused("null", qp, qip, 2, None, 0, 0, 4, 4, o.args())
    for null in (0, 1, 3):                                   # id_out, score_out, count_out; tag_out may be NULL
        a = list(o.args())
        a[null] = None
        refused("null", qp, qip, 2, tp, 0, 0, 4, 4, a)
    a = list(o.args())
    a[3] = None
    refused("null", qp, qip, 2, tp, 0, 0, 0, 0, a)           # a count still needs count_out
    for bad in (0, 1):
        t = thr.copy()
        t[bad] = np.nan
        refused("NaN", qp, qip, 2, t.ctypes.data_as(f32p), 0, 0, 4, 4, o.args())
        refused("NaN", qp, qip, 2, t.ctypes.data_as(f32p), 0, 0, 0, 0, o.args())


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    o = Outs()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    for t in (0.5, -INF, INF):
        thr = np.full(2, t, dtype=np.float32)
        for max_hits in (0, 4):
            for st, text in both(bn, q.ctypes.data_as(f32p), qi.ctypes.data_as(u64p), 2, thr.ctypes.data_as(f32p), 0, 0, max_hits, 4, o.args()):
                assert st == NO_DEVICE and "gfx950" in text
    # a count with NULL lists is a legal call: it gets as far as the device too
    thr = np.zeros(2, dtype=np.float32)
    st = bn.lib.bn_index_search_above(None, q.ctypes.data_as(f32p), 2, thr.ctypes.data_as(f32p), 0, 0, 0, 0, None, None, None, o.cnt.ctypes.data_as(u32p))
    assert st == NO_DEVICE and o.untouched()
    with pytest.raises(bn.EngineError):
        bn.Index(0, 8, 4)
