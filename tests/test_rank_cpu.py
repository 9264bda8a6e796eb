"""bn_head_rank_index without a GPU: the ABI declares and exports the entry point at ABI version 2, without a device the call
refuses with the no-device status and leaves the caller's outputs alone, and the numpy selection of tests/rank_ref.py agrees with a
brute-force sort under an explicit comparator on hand-made cases (ties, +-0, NaN, z against -z, ranges, exclusions).

The rank_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the
entry point and fail where the library lacks it."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 9


def test_header_library_and_harness_agree_on_the_entry_point(bn):
    L = C.CDLL(bn.LIB_PATH)
    assert hasattr(L, "bn_head_rank_index")
    assert "bn_head_rank_index" in bn.ENGINE_SYMBOLS
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    assert re.search(r"#define\s+BN_RANK_TOP\s+0u", header) and bn.BN_RANK_TOP == 0
    assert re.search(r"#define\s+BN_RANK_UNCERTAIN\s+1u", header) and bn.BN_RANK_UNCERTAIN == 1
    assert re.search(r"#define\s+BN_ABI_VERSION\s+2\b", header)
    assert bn.lib.bn_abi_version() == 2
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    assert "pub fn bn_head_rank_index(" in ffi


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    ids = np.full(8, 0xDEADBEEF, dtype=np.uint64)
    logits = np.full(8, -7.5, dtype=np.float32)
    counts = np.full(2, 77, dtype=np.uint32)
    before = ids.tobytes(), logits.tobytes(), counts.tobytes()
    st = bn.lib.bn_head_rank_index(None, None, 0, 0, 0, None, 0, 4, 4, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   logits.ctypes.data_as(C.POINTER(C.c_float)), counts.ctypes.data_as(C.POINTER(C.c_uint32)))
    assert st == NO_DEVICE and "gfx950" in bn.last_error()
    assert (ids.tobytes(), logits.tobytes(), counts.tobytes()) == before


def _brute(Z, valid, mode, M, first_id=0, n_ids=0, exclude=()):
    """per class: the eligible (id, z) pairs sorted by an explicit comparator, cut to M"""
    n, C_ = Z.shape
    last = n if n_ids == 0 else first_id + n_ids

    def cmp(a, b):
        ka, kb = (abs(a[1]), abs(b[1])) if mode == "uncertain" else (-a[1], -b[1])
        if ka < kb:
            return -1
        if ka > kb:
            return 1
        return -1 if a[0] < b[0] else (1 if a[0] > b[0] else 0)

    out = []
    for c in range(C_):
        rows = [(i, float(Z[i, c])) for i in range(n)
                if first_id <= i < last and valid[i] and i not in set(exclude) and not math.isnan(float(Z[i, c]))]
        out.append(sorted(rows, key=functools.cmp_to_key(cmp))[:M])
    return out


def _check(Z, valid, mode, M, **kw):
    Z = np.asarray(Z, dtype=np.float32)
    valid = np.asarray(valid, dtype=bool)
    ids, logits, counts = rank_ref.rank(Z, valid, mode, M, **kw)
    want = _brute(Z, valid, mode, M, **kw)
    for c, rows in enumerate(want):
        assert counts[c] == len(rows)
        assert ids[c, :len(rows)].tolist() == [r[0] for r in rows], (mode, c)
        assert logits[c, :len(rows)].tobytes() == np.array([r[1] for r in rows], dtype=np.float32).tobytes()
        assert np.all(ids[c, len(rows):] == 0) and np.all(np.isnan(logits[c, len(rows):]))
    return ids, logits, counts


@pytest.mark.parametrize("mode", ["top", "uncertain"])
def test_reference_hand_made_cases(mode):
    nan, inf = float("nan"), float("inf")
    # column 0: ties and both zeros; column 1: z against -z; column 2: NaN, infinities; column 3: all equal
    Z = np.array([[1.0, 2.0, nan, 3.0],
                  [0.0, -2.0, inf, 3.0],
                  [-0.0, 0.5, -inf, 3.0],
                  [1.0, -0.5, 0.25, 3.0],
                  [-1.0, 2.0, nan, 3.0],
                  [0.0, -2.0, -0.25, 3.0],
                  [5.0, 0.0, 1e-30, 3.0],
                  [-0.0, -0.0, -1e-30, 3.0]], dtype=np.float32)
    all_valid = np.ones(8, dtype=bool)
    for M in (1, 3, 8, 20):
        _check(Z, all_valid, mode, M)
        _check(Z, [1, 1, 0, 1, 1, 1, 0, 1], mode, M)
        _check(Z, all_valid, mode, M, first_id=2, n_ids=4)
        _check(Z, all_valid, mode, M, first_id=3)
        _check(Z, all_valid, mode, M, exclude=[0, 6, 6, 1])
        _check(Z, all_valid, mode, M, first_id=8)  # an empty range
    ids, logits, counts = _check(Z, all_valid, mode, 8)
    if mode == "top":
        assert ids[0, :counts[0]].tolist() == [6, 0, 3, 1, 2, 5, 7, 4]       # the four zeros in id order, whatever their sign
        assert ids[2, :counts[2]].tolist() == [1, 3, 6, 7, 5, 2] and counts[2] == 6  # NaN rows never returned
    else:
        assert ids[1, :counts[1]].tolist() == [6, 7, 2, 3, 0, 1, 4, 5]       # 2 and -2 tie, by id
        assert logits[1, :counts[1]].tolist() == [0.0, -0.0, 0.5, -0.5, 2.0, -2.0, 2.0, -2.0]  # the logit keeps its sign
        assert ids[2, :counts[2]].tolist() == [6, 7, 3, 5, 1, 2]
    assert ids[3].tolist() == list(range(8))


def test_reference_random_with_heavy_ties():
    rng = np.random.default_rng(11)
    Z = rng.integers(-3, 4, (200, 5)).astype(np.float32) * np.float32(0.5)
    Z[rng.random((200, 5)) < 0.05] = np.nan
    Z[rng.random((200, 5)) < 0.05] *= np.float32(-0.0)  # signed zeros
    valid = rng.random(200) < 0.9
    ex = rng.integers(0, 200, 30)
    for mode in ("top", "uncertain"):
        for M in (1, 17, 256):
            _check(Z, valid, mode, M, first_id=13, n_ids=150, exclude=ex)


def test_reference_m_stride_and_bad_range():
    Z = np.arange(6, dtype=np.float32).reshape(6, 1)
    ids, logits, counts = rank_ref.rank(Z, np.ones(6, dtype=bool), "top", 2, m_stride=5)
    assert ids.shape == (1, 5) and ids[0].tolist() == [5, 4, 0, 0, 0] and counts[0] == 2
    with pytest.raises(ValueError):
        rank_ref.rank(Z, np.ones(6, dtype=bool), "top", 2, first_id=4, n_ids=3)
