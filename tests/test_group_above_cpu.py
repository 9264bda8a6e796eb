"""bn_index_group_above without a GPU: the numpy rule of tests/group_above_ref.py against a literal double loop over the header's
sentences and against above_ref's counts; the header, the library, the harness and the Rust bindings agree on the new names; arguments
that need no index are refused before the device is asked for; without a device the calls refuse with the no-device status and leave
the caller's outputs alone; the plan arithmetic runs clean under ASan / UBSan (tools/asan_group_plan.cpp).

The group_above_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the
entry points and fail where the library lacks them."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import above_ref
import group_above_ref as gref
import index_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
NAMES = ("bn_index_group_above", "bn_index_group_above_ids")
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
INF = float("inf")
NO_ROW = gref.NO_ROW


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def double_loop(S, qbad, xbad, thr, tags, n_groups, lo, hi, qid, radius):
    """the header's sentences one pair at a time"""
    nq = S.shape[0]
    cnt = np.zeros((nq, n_groups), dtype=np.uint32)
    ids = [np.full((nq, n_groups), NO_ROW, dtype=np.uint64) for _ in range(3)]      # best, first, last
    bs = np.zeros((nq, n_groups), dtype=np.float32)
    other, total = np.zeros(nq, dtype=np.uint32), np.zeros(nq, dtype=np.uint32)
    for q in range(nq):
        for r in range(S.shape[1]):
            if qbad[q] or xbad[r] or not lo <= r < hi:
                continue
            if qid is not None and radius >= 0 and abs(r - int(qid[q])) <= radius:
                continue
            s = np.float32(S[q, r])
            if not s >= np.float32(thr[q]):
                continue
            total[q] += 1
            g = int(tags[r]) if tags is not None else 0
            if g >= n_groups:
                other[q] += 1
                continue
            if cnt[q, g] == 0 or s > bs[q, g]:               # r ascends, so a tie keeps the lower id
                ids[0][q, g], bs[q, g] = r, s
            if cnt[q, g] == 0:
                ids[1][q, g] = r
            ids[2][q, g] = r
            cnt[q, g] += 1
    return cnt, ids[0], bs, ids[1], ids[2], other, total


def small_case():
    """40 dyadic rows at few levels against 6 queries: heavy ties; query 4 is invalid; row 7 is zeros, row 21 has a NaN"""
    rng = np.random.default_rng(11)
    lv = rng.integers(-4, 5, 40) * 4
    lv[[3, 4, 5, 30]] = 8
    X = ir.rows_at_levels(rng, lv, 32, 16)
    X[7] = 0
    X[21, 2] = np.nan
    Q = np.concatenate([ir.canonical_query(32, 16)[None], ir.dyadic_rows(rng, 5, 32, 16)])
    Q[4] = 0
    S, qbad, xbad = ir.scores64(Q, X)
    assert qbad.tolist() == [False] * 4 + [True, False] and np.flatnonzero(xbad).tolist() == [7, 21]
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S), "dyadic scores are exact in f32"
    return S, qbad, xbad, rng


def tag_patterns(rng, n):
    return {"none": None, "zero": np.zeros(n, dtype=np.uint32), "runs": np.repeat(np.arange(8, dtype=np.uint32), 5)[:n],
            "random": rng.integers(0, 6, n).astype(np.uint32), "high": rng.choice(np.array([0, 1, 2, 63, 64, 65535], dtype=np.uint32), n)}


def test_reference_equals_a_literal_double_loop():
    S, qbad, xbad, rng = small_case()
    nq, n = S.shape
    thresholds = [np.full(nq, 0.5), np.full(nq, -INF), np.full(nq, INF), np.array([0.5, 0.0, -0.25, 1.0, 0.0, -INF])]
    qid = np.array([0, 3, 4, 39, 7, 20])
    seen_tie = False
    for name, tags in tag_patterns(rng, n).items():
        for thr in thresholds:
            for n_groups in (1, 2, 6, 64, 65):
                for first, cnt in ((0, 0), (4, 27), (39, 0), (n, 0), (5, 1)):
                    for ids, radius in ((None, -1), (qid, 0), (qid, 2)):
                        lo, hi = above_ref.id_range(n, first, cnt)
                        want = double_loop(S, qbad, xbad, thr, tags, n_groups, lo, hi, ids, radius)
                        got = gref.from_scores(S, qbad, xbad, thr, n_groups, tags, first, cnt, ids, radius)
                        gref.assert_same(got, want, (name, thr[0], n_groups, first, cnt, radius))
                        seen_tie = seen_tie or bool((got[0] > 1).any())
    assert seen_tie
    # a stride wider than n_groups: the binding's fills past n_groups
    got = gref.from_scores(S, qbad, xbad, 0.0, 3, tag_patterns(rng, n)["random"], g_stride=5)
    assert got[0].shape == (nq, 5) and not got[0][:, 3:].any() and (got[1][:, 3:] == NO_ROW).all() and np.isnan(got[2][:, 3:]).all()
    assert (got[3][:, 3:] == NO_ROW).all() and (got[4][:, 3:] == NO_ROW).all()


def test_best_hit_is_the_highest_score_then_the_lowest_id_and_zeros_tie():
    S = np.array([[0.5, 0.75, 0.75, 0.25, -0.0, 0.0, 0.75]])
    no = np.zeros(1, dtype=bool), np.zeros(7, dtype=bool)
    c, b, s, f, l, o, t = gref.from_scores(S, *no, -1.0, 2, np.array([0, 0, 0, 0, 1, 1, 0]))
    assert c.tolist() == [[5, 2]] and b.tolist() == [[1, 4]] and f.tolist() == [[0, 4]] and l.tolist() == [[6, 5]] and t.tolist() == [7] and o.tolist() == [0]
    assert s[0, 0] == 0.75 and s[0, 1] == 0 and s[:, 1].tobytes() == np.float32(-0.0).tobytes(), "the best hit's own bits: row 4 holds -0.0"
    # narrowed(): the records of fewer groups cut from the records of all of them
    S, qbad, xbad, rng = small_case()
    tags = tag_patterns(rng, 40)["high"]
    hit = above_ref.hit_mask(S, qbad, xbad, 0.0)
    full = gref.records(hit, S, tags, 65536)
    for n_groups, nq, stride in ((1, 6, None), (3, 2, 7), (64, 6, 64), (65, 1, None), (65536, 6, None)):
        gref.assert_same(gref.narrowed(full, hit, tags, n_groups, nq, stride), gref.records(hit[:nq], S[:nq], tags, n_groups, stride), (n_groups, nq))


def test_counts_sum_to_the_threshold_search_count():
    S, qbad, xbad, rng = small_case()
    for name, tags in tag_patterns(rng, 40).items():
        for thr in (0.5, 0.0, -INF, INF):
            for n_groups in (1, 3, 65536):
                for first, cnt, ids, radius in ((0, 0, None, -1), (4, 27, np.array([0, 3, 4, 39, 7, 20]), 2)):
                    got = gref.from_scores(S, qbad, xbad, thr, n_groups, tags, first, cnt, ids, radius)
                    hits = above_ref.hits_from_scores(S, qbad, xbad, thr, first, cnt, ids, radius)
                    assert got[6].tolist() == [len(h[0]) for h in hits]
                    assert np.array_equal(got[0].sum(axis=1, dtype=np.uint64) + got[5], got[6])
                    empty = got[0] == 0
                    assert (got[1][empty] == NO_ROW).all() and (got[3][empty] == NO_ROW).all() and (got[4][empty] == NO_ROW).all()
                    assert got[2][empty].tobytes() == np.zeros(int(empty.sum()), dtype=np.float32).tobytes()
                    assert (got[3][~empty] <= got[1][~empty]).all() and (got[1][~empty] <= got[4][~empty]).all()


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^bn_status (bn_index_group_above\w*)\(", header, flags=re.M)
    assert sorted(declared) == sorted(NAMES)
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "#define BN_GROUP_NO_ROW UINT64_MAX" in header and bn.BN_GROUP_NO_ROW == NO_ROW
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert header.index("bn_status bn_index_search_above_ids(") < header.index("bn_status bn_index_group_above(") < header.index("bn_status bn_index_save(")
    assert all(hasattr(bn.Index, m) for m in ("group_above", "group_above_ids"))


class Outs:
    """the seven outputs pre-filled with sentinels"""

    def __init__(self, nq=2, stride=4):
        self.arrays = [np.full(nq * stride, 77, dtype=np.uint32), np.full(nq * stride, 0xABCDEF, dtype=np.uint64), np.full(nq * stride, -7.5, dtype=np.float32),
                       np.full(nq * stride, 0xABCDE0, dtype=np.uint64), np.full(nq * stride, 0xABCDE1, dtype=np.uint64), np.full(nq, 78, dtype=np.uint32),
                       np.full(nq, 79, dtype=np.uint32)]
        self.before = self.bytes()

    def bytes(self):
        return tuple(a.tobytes() for a in self.arrays)

    def args(self, drop=()):
        types = (u32p, u64p, f32p, u64p, u64p, u32p, u32p)
        return [None if i in drop else a.ctypes.data_as(t) for i, (a, t) in enumerate(zip(self.arrays, types))]

    def untouched(self):
        return self.bytes() == self.before


def both(bn, queries, ids, n, thr, first, n_ids, n_groups, stride, outs):
    """the two entry points with the same arguments: (status, message) of each"""
    a = bn.lib.bn_index_group_above(None, queries, n, thr, first, n_ids, n_groups, stride, *outs)
    ma = bn.last_error()
    b = bn.lib.bn_index_group_above_ids(None, ids, n, -1, thr, first, n_ids, n_groups, stride, *outs)
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

    refused("n_groups", qp, qip, 2, tp, 0, 0, 0, 4, o.args())
    refused("n_groups", qp, qip, 2, tp, 0, 0, 65537, 65537, o.args())
    refused("n_groups", qp, qip, 2, tp, 0, 0, 1 << 40, 1 << 40, o.args())
    refused("g_stride", qp, qip, 2, tp, 0, 0, 4, 3, o.args())
    refused("pair", qp, qip, 2, tp, 0, 0, 4, 4, o.args(drop=(1,)))
    refused("pair", qp, qip, 2, tp, 0, 0, 4, 4, o.args(drop=(2,)))
    refused("null", None, None, 2, tp, 0, 0, 4, 4, o.args())
    refused("null", qp, qip, 2, None, 0, 0, 4, 4, o.args())
    refused("null", qp, qip, 2, tp, 0, 0, 4, 4, o.args(drop=(0,)))
    refused("null", qp, qip, 2, tp, 0, 0, 4, 4, o.args(drop=(0, 1, 2, 3, 4, 5, 6)))
    for bad in (0, 1):
        t = thr.copy()
        t[bad] = np.nan
        refused("NaN", qp, qip, 2, t.ctypes.data_as(f32p), 0, 0, 4, 4, o.args())
        refused("NaN", qp, qip, 2, t.ctypes.data_as(f32p), 0, 0, 1, 4, o.args(drop=(1, 2, 3, 4, 5, 6)))


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    o = Outs()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    for t in (0.5, -INF, INF):
        thr = np.full(2, t, dtype=np.float32)
        for drop in ((), (1, 2), (1, 2, 3, 4, 5, 6)):
            for st, text in both(bn, q.ctypes.data_as(f32p), qi.ctypes.data_as(u64p), 2, thr.ctypes.data_as(f32p), 0, 0, 4, 4, o.args(drop)):
                assert st == NO_DEVICE and "gfx950" in text
    assert o.untouched()


# ---- the plan arithmetic under the sanitizers -------------------------------------------------------------------------------------
def test_plan_and_refusals_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path / "asan_group_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_group_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the plan check failed:\n" + r.stderr[-3000:])
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert re.search(r"\d+ plans, \d+ refusals, 0 failures", r.stdout), r.stdout
