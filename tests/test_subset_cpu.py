"""bn_subset_* and the row tags without a GPU: the numpy rules of tests/subset_ref.py on hand-made cases; the header, the library, the
harness and the Rust bindings agree on every new name; arguments that need neither an index nor a subset are refused before the device
is asked for; without a device the calls refuse with the no-device status and leave the caller's outputs alone.

The subset_ref tests are self-checks of the reference: they touch no library code.  The tests that take the `bn` fixture need the entry
points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import subset_ref
from subset_ref import Filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, NO_DEVICE = 1, 9
SUBSET_NAMES = ("bn_subset_select", "bn_subset_from_ids", "bn_subset_free", "bn_subset_size", "bn_subset_read", "bn_subset_search",
                "bn_subset_search_ids")
TAG_NAMES = ("bn_index_set_tags", "bn_index_fill_tags", "bn_index_read_tags")
f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


# ---- the reference's own rules --------------------------------------------------------------------------------------------------
def test_reference_members_range_edges():
    tags = np.zeros(200, dtype=np.uint32)
    m = subset_ref.members
    assert m(tags, 200, Filter()).tolist() == list(range(200)) and m(tags, 200, Filter()).dtype == np.uint64
    assert m(tags, 200, Filter(63, 2)).tolist() == [63, 64]
    assert m(tags, 200, Filter(64, 64)).tolist() == list(range(64, 128))
    assert m(tags, 200, Filter(199, 0)).tolist() == [199] and m(tags, 200, Filter(199, 1)).tolist() == [199]
    assert m(tags, 200, Filter(200, 0)).tolist() == [], "n_ids 0 at the end of the index: the empty range"
    assert m(tags, 200, Filter(0, 200)).tolist() == list(range(200))
    assert m(np.zeros(0), 0, Filter()).tolist() == []
    for first, n in ((201, 0), (0, 201), (150, 51), (200, 1)):
        with pytest.raises(ValueError):
            m(tags, 200, Filter(first, n))


def test_reference_members_include_exclude_duplicates():
    tags = np.array([0, 3, 5, 5, 0, 65535, 3, 1, 0, 5], dtype=np.uint32)
    m = subset_ref.members
    assert m(tags, 10, Filter(tags=[3])).tolist() == [1, 6]
    assert m(tags, 10, Filter(tags=[0, 5, 5])).tolist() == [0, 2, 3, 4, 8, 9], "duplicates in the list are allowed"
    assert m(tags, 10, Filter(tags=[0], flags=subset_ref.EXCLUDE_TAGS)).tolist() == [1, 2, 3, 5, 6, 7, 9]
    assert m(tags, 10, Filter(tags=[0, 5, 5], flags=subset_ref.EXCLUDE_TAGS)).tolist() == [1, 5, 6, 7]
    assert m(tags, 10, Filter(tags=[65535])).tolist() == [5]
    assert m(tags, 10, Filter(tags=[7])).tolist() == [], "a tag nobody has: the empty subset"
    assert m(tags, 10, Filter(tags=[7], flags=subset_ref.EXCLUDE_TAGS)).tolist() == list(range(10))
    assert m(tags, 10, Filter(tags=[], flags=subset_ref.EXCLUDE_TAGS)).tolist() == list(range(10)), "an empty list tests nothing"
    assert m(tags, 10, Filter(2, 5, tags=[5, 3])).tolist() == [2, 3, 6], "range and tags together"
    for bad in (Filter(tags=[65536]), Filter(tags=[3, 1 << 20]), Filter(flags=2), Filter(tags=[1], flags=3)):
        with pytest.raises(ValueError):
            m(tags, 10, bad)


def test_reference_restricted_top_m_heavy_ties_ordered_by_id():
    rng = np.random.default_rng(2)
    n, nq = 500, 6
    S = rng.integers(-1, 2, (nq, n)).astype(np.float32)        # three score levels
    S[rng.random(S.shape) < 0.1] *= np.float32(-0.0)           # -0.0 == +0.0
    xbad = rng.random(n) < 0.1
    qbad = np.zeros(nq, dtype=bool)
    qbad[4] = True
    qid = rng.integers(0, n, nq)
    for mem in (np.arange(n), np.flatnonzero(rng.random(n) < 0.3), np.array([7]), np.flatnonzero(xbad), np.zeros(0, dtype=np.int64)):
        for radius in (-1, 0, 5):
            for M in (1, 7, 256):
                ids, sc, cnt = subset_ref.restricted_top_m(S, qbad, xbad, mem, M, qid, radius)
                assert ids.dtype == np.uint64 and sc.dtype == np.float32 and cnt.dtype == np.uint32
                for q in range(nq):
                    ok = [i for i in mem.tolist() if not xbad[i] and not (radius >= 0 and abs(i - int(qid[q])) <= radius)]
                    want = [] if qbad[q] else sorted(ok, key=lambda i: (-float(S[q, i]), i))[:M]
                    assert cnt[q] == len(want) and ids[q, :cnt[q]].tolist() == want, (len(mem), radius, M, q)
                    assert sc[q, :cnt[q]].tobytes() == S[q, want].tobytes() and np.isnan(sc[q, cnt[q]:]).all() and not ids[q, cnt[q]:].any()
    # without qid the radius has nothing to apply to
    a = subset_ref.restricted_top_m(S, qbad, xbad, np.arange(n), 9)
    b = subset_ref.restricted_top_m(S, qbad, xbad, np.arange(n)[::-1], 9, None, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "the member list is a set"
    with pytest.raises(ValueError):
        subset_ref.restricted_top_m(S, qbad, xbad, [3, 3], 2)


# ---- the library without a device ---------------------------------------------------------------------------------------------
def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    declared = re.findall(r"^(?:bn_status|void|size_t) (bn_subset_\w+)\(", header, flags=re.M)
    assert sorted(declared) == sorted(SUBSET_NAMES)
    declared = re.findall(r"^bn_status (bn_index_\w+_tags)\(", header, flags=re.M)
    assert sorted(declared) == sorted(TAG_NAMES)
    for name in SUBSET_NAMES + TAG_NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "pub fn %s(" % name in ffi
    assert "typedef struct bn_subset bn_subset;" in header and "pub struct bn_subset" in ffi
    assert "typedef struct bn_index_filter {" in header and "pub struct bn_index_filter {" in ffi
    assert "#define BN_INDEX_TAG_LIMIT 65536u" in header and "pub const BN_INDEX_TAG_LIMIT: u32 = 65536;" in ffi
    assert "#define BN_FILTER_EXCLUDE_TAGS 1u" in header and "pub const BN_FILTER_EXCLUDE_TAGS: u32 = 1;" in ffi
    assert bn.BN_INDEX_TAG_LIMIT == subset_ref.TAG_LIMIT == 65536 and bn.BN_FILTER_EXCLUDE_TAGS == subset_ref.EXCLUDE_TAGS == 1
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert hasattr(bn, "Subset") and all(hasattr(bn.Subset, m) for m in ("select", "from_ids", "ids", "search", "search_ids"))
    assert all(hasattr(bn.Index, m) for m in ("set_tags", "fill_tags", "tags"))
    # the ctypes mirror of bn_index_filter: the header's fields in order
    assert [f[0] for f in bn.BnIndexFilter._fields_] == ["first_id", "n_ids", "tags", "n_tags", "flags"]
    assert C.sizeof(bn.BnIndexFilter) == 40


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


def make_filter(bn, first_id=0, n_ids=0, tags=None, flags=0):
    t = None if tags is None else np.asarray(tags, dtype=np.uint32)
    f = bn.BnIndexFilter(first_id, n_ids, None if t is None else t.ctypes.data_as(u32p), 0 if t is None else len(t), flags)
    return f, t  # t must outlive the call


def test_arguments_are_refused_before_any_device_call(bn):
    """these refusals need neither an index, a subset nor a device: they are the same with and without a GPU"""
    size = C.sizeof(bn.BnIndexFilter)
    h = C.c_void_p(0x1234)
    # bn_subset_select
    f, _ = make_filter(bn)
    assert bn.lib.bn_subset_select(None, C.byref(f), size, None) == INVALID_ARG and "null" in bn.last_error()
    assert bn.lib.bn_subset_select(None, None, size, C.byref(h)) == INVALID_ARG and "null" in bn.last_error()
    for small in (0, 8, size - 1):
        assert bn.lib.bn_subset_select(None, C.byref(f), small, C.byref(h)) == INVALID_ARG and "struct_size" in bn.last_error()
    for flags in (2, 3, 0x80000000):
        f, _ = make_filter(bn, flags=flags)
        assert bn.lib.bn_subset_select(None, C.byref(f), size, C.byref(h)) == INVALID_ARG and "flags" in bn.last_error()
    for tags in ([65536], [1, 2, 1 << 31], [0, 65535, 70000]):
        for flags in (0, bn.BN_FILTER_EXCLUDE_TAGS):
            f, keep = make_filter(bn, tags=tags, flags=flags)
            assert bn.lib.bn_subset_select(None, C.byref(f), size, C.byref(h)) == INVALID_ARG and "tag" in bn.last_error()
    # bn_subset_from_ids
    ids = np.array([1, 2, 3], dtype=np.uint64)
    assert bn.lib.bn_subset_from_ids(None, ids.ctypes.data_as(u64p), 3, None) == INVALID_ARG and "null" in bn.last_error()
    assert bn.lib.bn_subset_from_ids(None, None, 3, C.byref(h)) == INVALID_ARG and "null" in bn.last_error()
    for bad in ([1, 1], [0, 5, 4], [3, 2, 1], [0, 1, 2, 2]):
        ids = np.array(bad, dtype=np.uint64)
        assert bn.lib.bn_subset_from_ids(None, ids.ctypes.data_as(u64p), len(bad), C.byref(h)) == INVALID_ARG and "ascending" in bn.last_error()
    assert h.value == 0x1234, "nothing created"
    # the searches: every refusal bn_index_search makes of its arguments
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    for top_m, stride, msg in ((0, 4, "top_m"), (257, 300, "top_m"), (4, 3, "m_stride")):
        o = Outs()
        assert bn.lib.bn_subset_search(None, q.ctypes.data_as(f32p), 2, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert bn.lib.bn_subset_search_ids(None, qi.ctypes.data_as(u64p), 2, -1, top_m, stride, *o.args()) == INVALID_ARG and msg in bn.last_error()
        assert o.untouched()
    o = Outs()
    assert bn.lib.bn_subset_search(None, None, 2, 4, 4, *o.args()) == INVALID_ARG
    assert bn.lib.bn_subset_search_ids(None, None, 2, -1, 4, 4, *o.args()) == INVALID_ARG
    for null in range(3):
        a = list(o.args())
        a[null] = None
        assert bn.lib.bn_subset_search(None, q.ctypes.data_as(f32p), 2, 4, 4, *a) == INVALID_ARG
        assert bn.lib.bn_subset_search_ids(None, qi.ctypes.data_as(u64p), 2, 0, 4, 4, *a) == INVALID_ARG
    assert o.untouched()
    assert bn.lib.bn_subset_read(None, 0, 2, None) == INVALID_ARG
    # the tag calls refuse a NULL index as every bn_index_* call does
    t = np.full(2, 9, dtype=np.uint32)
    assert bn.lib.bn_index_set_tags(None, 0, 2, t.ctypes.data_as(u32p)) == INVALID_ARG and bn.last_error()
    assert bn.lib.bn_index_fill_tags(None, 0, 2, 1) == INVALID_ARG
    assert bn.lib.bn_index_read_tags(None, 0, 2, t.ctypes.data_as(u32p)) == INVALID_ARG and (t == 9).all()
    # the calls that need no device
    assert bn.lib.bn_subset_size(None) == 0
    bn.lib.bn_subset_free(None)


def test_no_device_means_refusal_and_untouched_outputs(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    size = C.sizeof(bn.BnIndexFilter)
    h = C.c_void_p(0x1234)
    for tags, flags in ((None, 0), ([3, 3], 0), ([0], bn.BN_FILTER_EXCLUDE_TAGS)):
        f, keep = make_filter(bn, 0, 0, tags, flags)
        assert bn.lib.bn_subset_select(None, C.byref(f), size, C.byref(h)) == NO_DEVICE and "gfx950" in bn.last_error()
    ids = np.array([1, 2, 3], dtype=np.uint64)
    assert bn.lib.bn_subset_from_ids(None, ids.ctypes.data_as(u64p), 3, C.byref(h)) == NO_DEVICE and "gfx950" in bn.last_error()
    assert bn.lib.bn_subset_from_ids(None, None, 0, C.byref(h)) == NO_DEVICE
    assert h.value == 0x1234
    out = np.full(2, 55, dtype=np.uint64)
    assert bn.lib.bn_subset_read(None, 0, 2, out.ctypes.data_as(u64p)) == NO_DEVICE and (out == 55).all()
    o = Outs()
    q = np.ones(8, dtype=np.float32)
    qi = np.zeros(2, dtype=np.uint64)
    assert bn.lib.bn_subset_search(None, q.ctypes.data_as(f32p), 2, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert bn.lib.bn_subset_search_ids(None, qi.ctypes.data_as(u64p), 2, 0, 4, 4, *o.args()) == NO_DEVICE and "gfx950" in bn.last_error()
    assert o.untouched()
