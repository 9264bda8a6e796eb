"""CPU-side checks of matching against an attached index: match_ref's restatement of the threshold rule against
index_ref.top_m_exact on rows whose scores are exact, and the C ABI's three entry points (declared, exported, bound, and refusing
NULL handles with a message before any device call)."""
import ctypes as C
import os
import re

import numpy as np

import index_ref
import match_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH_SYMBOLS = ["bn_ctx_attach_index", "bn_step_index_results", "bn_index_match"]
DIM, NNZ = 64, 16
LEVELS = [16, 8, 8, 8, 8, 8, 4, 4, 0, 0, 0, -4, -16]  # score = level / 16


def _fixture():
    rng = np.random.default_rng(3)
    X = index_ref.rows_at_levels(rng, LEVELS, DIM, NNZ)
    Q = index_ref.canonical_query(DIM, NNZ)[None, :]
    tags = (np.arange(len(LEVELS)) * 7 + 1).astype(np.uint32)
    return Q, X, tags


def _ids_at_least(level):
    return [i for i, lv in enumerate(LEVELS) if lv >= level]  # LEVELS is descending: this is the expected order too


def test_threshold_equal_to_a_level_keeps_the_ties():
    Q, X, tags = _fixture()
    ids, scores, tg, counts = match_ref.match_exact(Q, X, 10, min_score=0.5, tags=tags)
    want = _ids_at_least(8)
    assert counts[0] == len(want) == 6 and ids[0, :6].tolist() == want
    assert scores[0, :6].tolist() == [1.0] + [0.5] * 5 and tg[0, :6].tolist() == tags[want].tolist()
    assert np.all(ids[0, 6:] == 0) and np.all(np.isnan(scores[0, 6:])) and np.all(tg[0, 6:] == 0)
    # more tied rows than top_m: the lowest ids of the level
    ids, scores, tg, counts = match_ref.match_exact(Q, X, 3, min_score=0.5, tags=tags)
    assert counts[0] == 3 and ids[0].tolist() == [0, 1, 2]
    # and the whole is the prefix of the unthresholded list
    full = index_ref.top_m_exact(Q, X, 10)
    assert match_ref.same(match_ref.match_exact(Q, X, 10, min_score=0.5, tags=tags), match_ref.prefix(*full, min_score=0.5, tags=tags)) is None


def test_threshold_between_levels_cuts_there():
    Q, X, tags = _fixture()
    ids, _, _, counts = match_ref.match_exact(Q, X, 13, min_score=0.3, tags=tags)
    assert counts[0] == 6 and ids[0, :6].tolist() == _ids_at_least(8)
    ids, _, _, counts = match_ref.match_exact(Q, X, 13, min_score=0.2, tags=tags)
    assert counts[0] == 8 and ids[0, :8].tolist() == _ids_at_least(4)


def test_threshold_above_every_score_gives_count_zero():
    Q, X, tags = _fixture()
    ids, scores, tg, counts = match_ref.match_exact(Q, X, 5, min_score=np.nextafter(np.float32(1), np.float32(2)), tags=tags)
    assert counts[0] == 0 and np.all(ids == 0) and np.all(np.isnan(scores)) and np.all(tg == 0)
    assert match_ref.match_exact(Q, X, 5, min_score=1.0)[3][0] == 1


def test_negative_zero_ties_positive_zero():
    Q, X, tags = _fixture()
    for zero in (0.0, -0.0):
        ids, scores, _, counts = match_ref.match_exact(Q, X, 13, min_score=zero, tags=tags)
        assert counts[0] == 11 and ids[0, :11].tolist() == _ids_at_least(0)
        assert np.all(scores[0, 8:11] == 0)
    # a list that holds -0.0 scores (as a search may return them) is cut the same way
    got = match_ref.prefix(np.array([[4, 9, 2]], dtype=np.uint64), np.array([[0.5, -0.0, -0.25]], dtype=np.float32), [3], min_score=0.0)
    assert got[3][0] == 2 and got[0][0].tolist() == [4, 9, 0]


def test_an_invalid_query_and_an_invalid_row():
    Q, X, tags = _fixture()
    Q2 = np.vstack([Q, np.zeros_like(Q)])
    X2 = X.copy()
    X2[0] = 0
    ids, _, _, counts = match_ref.match_exact(Q2, X2, 4, min_score=0.5, tags=tags)
    assert counts.tolist() == [4, 0] and ids[0].tolist() == [1, 2, 3, 4]


def test_every_match_symbol_is_declared_exported_and_bound(bn):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "birdnet_hip.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    L = C.CDLL(bn.LIB_PATH)
    for name in MATCH_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert L.bn_abi_version() == 2


def test_null_handles_are_refused_with_a_message(bn):
    L = C.CDLL(bn.LIB_PATH)
    for name in MATCH_SYMBOLS + ["bn_last_error"]:
        getattr(L, name).restype = C.c_int32 if name != "bn_last_error" else C.c_size_t
    buf = C.create_string_buffer(512)

    def message():
        L.bn_last_error(buf, C.c_size_t(512))
        return buf.value.decode()

    null = C.c_void_p(None)
    assert L.bn_ctx_attach_index(null, null, C.c_size_t(10), C.c_int32(0), C.c_float(0)) == 1
    assert "null context" in message()
    assert L.bn_step_index_results(null, null, null, null, null, null, null) == 1
    assert "null context" in message()
    assert L.bn_index_match(null, null, C.c_size_t(0), C.c_size_t(10), C.c_int32(0), C.c_float(0), C.c_size_t(10), null, null, null, null) == 1
    assert "null index" in message()
