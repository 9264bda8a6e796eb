"""The premise of test_gpu_index_exact.py, checked without a device: on dyadic rows an f32 dot product accumulated in ANY k order
equals the float64 cosine bit for bit, so a wrong id or score bit from the index is a kernel bug and not rounding; and the
generators and the reference top-M of tests/index_ref.py do what they say."""
import numpy as np
import pytest

import index_ref as ir

SHAPES = [(128, 64), (200, 64), (300, 256), (1, 1), (5, 4)]  # every (dim, nnz) of test_gpu_index_exact.py


def all_levels(dim, nnz):
    """levels reachable at (dim, nnz), ascending"""
    out = []
    for n in range(-nnz, nnz + 1):
        try:
            ir.rows_at_levels(np.random.default_rng(0), [n], dim, nnz)
            out.append(n)
        except ValueError:
            pass
    return out


@pytest.mark.parametrize("dim,nnz", SHAPES)
def test_f32_accumulation_in_any_order_is_the_float64_score(dim, nnz):
    rng = np.random.default_rng(dim * 1000 + nnz)
    X = np.concatenate([ir.dyadic_rows(rng, 300, dim, nnz), ir.rows_at_levels(rng, rng.choice(all_levels(dim, nnz), 200), dim, nnz)])
    Q = np.concatenate([ir.canonical_query(dim, nnz)[None], ir.dyadic_rows(rng, 9, dim, nnz)])
    assert np.all((X != 0).sum(axis=1) == nnz) and set(np.unique(X).tolist()) <= {-1.0, 0.0, 1.0}
    Xn, Qn = ir.stored(X, nnz), ir.stored(Q, nnz)
    # the stored form is the f32 normalisation itself: sum of squares 4^j, norm 2^j, x / 2^j
    ss = (X * X).sum(axis=1, dtype=np.float32)
    assert np.all(ss == nnz) and (X / np.sqrt(ss)[:, None]).astype(np.float32).tobytes() == Xn.tobytes()
    S64, qbad, xbad = ir.scores64(Q, X)
    assert not qbad.any() and not xbad.any()
    want = S64.astype(np.float32)
    assert np.all(want.astype(np.float64) == S64), "the float64 score is not an f32 number"
    assert np.all(S64 * nnz == np.round(S64 * nnz)) and np.abs(S64).max() <= 1
    orders = [np.arange(dim), np.arange(dim)[::-1]] + [rng.permutation(dim) for _ in range(4)]
    for order in orders:
        assert ir.f32_scores_in_order(Qn, Xn, order).tobytes() == want.tobytes()


@pytest.mark.parametrize("dim,nnz", SHAPES)
def test_rows_at_levels_hits_its_levels(dim, nnz):
    rng = np.random.default_rng(dim + nnz)
    reach = all_levels(dim, nnz)
    # a non-zero may leave the query's support only where the row has room for it
    assert reach == [n for n in range(-nnz, nnz + 1) if max(abs(n), 2 * nnz - dim) + ((max(abs(n), 2 * nnz - dim) - n) & 1) <= nnz]
    assert reach[0] == -nnz and reach[-1] == nnz
    lv = np.concatenate([np.array(reach), rng.choice(reach, 500)])
    X = ir.rows_at_levels(rng, lv, dim, nnz)
    assert X.dtype == np.float32 and X.shape == (len(lv), dim)
    assert np.all((X != 0).sum(axis=1) == nnz) and set(np.unique(X).tolist()) <= {-1.0, 0.0, 1.0}
    S, _, _ = ir.scores64(ir.canonical_query(dim, nnz)[None], X)
    assert np.all(S[0] * nnz == lv)
    assert np.all(ir.rows_at_levels(rng, [nnz] * 3, dim, nnz) == ir.canonical_query(dim, nnz))


def test_unreachable_levels_and_bad_nnz_raise():
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError):
        ir.rows_at_levels(rng, [0], 1, 1)          # one element: the score is +-1
    with pytest.raises(ValueError):
        ir.rows_at_levels(rng, [3, 5], 5, 4)       # |level| > nnz
    with pytest.raises(ValueError):
        ir.rows_at_levels(rng, [1], 4, 4)          # no room outside the support: a + b = 4, so a - b is even
    for call in (lambda: ir.dyadic_rows(rng, 2, 8, 3), lambda: ir.dyadic_rows(rng, 2, 3, 4), lambda: ir.canonical_query(8, 2)):
        with pytest.raises(ValueError):
            call()


def test_top_m_exact_order_masks_and_sentinels():
    Q = np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0], [np.nan, 1, 0, 0]], dtype=np.float32)
    X = np.array([[0, 1, 0, 0], [2, 0, 0, 0], [0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [np.inf, 0, 0, 0], [-3, 0, 0, 0], [0, 0, 5, 0]],
                 dtype=np.float32)
    ids, sc, cnt = ir.top_m_exact(Q, X, 7)
    assert list(cnt) == [6, 0, 6, 0]
    assert list(ids[0]) == [1, 3, 0, 2, 7, 6, 0] and sc[0, :6].tobytes() == np.array([1, 1, 0, 0, 0, -1], dtype=np.float32).tobytes()
    assert np.isnan(sc[0, 6]) and np.isnan(sc[1]).all() and not ids[1].any()
    assert not np.signbit(sc[0, :6][sc[0, :6] == 0]).any()  # -0.0 and +0.0 are one score, reported as +0.0
    assert list(ids[2, :6]) == [0, 1, 3, 6, 7, 2]
    ids, sc, cnt = ir.top_m_exact(Q[:1], X, 2, excluded=[np.array([1, 0])], invalid=np.arange(8) == 3)
    assert list(cnt) == [2] and list(ids[0]) == [2, 7]
    mask = np.zeros((1, 8), dtype=bool)
    mask[0, :7] = True
    ids, sc, cnt = ir.top_m_exact(Q[:1], X, 3, excluded=mask)
    assert list(cnt) == [1] and list(ids[0]) == [7, 0, 0]

