"""The yardstick of test_gpu_b3_precision.py, checked on its own (no GPU): the numpy model of the bf16x3 scheme (tests/b3_model.py) splits
exactly, is as good as an f32 matmul, and every mutant it builds bounds from is at least 16 x worse than the faithful model on the operands
of every GPU case -- so the geometric-mean bound leaves 4 x above the model and 4 x below the weakest mutant."""
import numpy as np
import pytest

import b3_model as b3


def test_split_is_exact_for_the_value_classes_of_the_device_split_test():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(100000).astype(np.float32) * np.float32(10.0) ** rng.integers(-20, 20, 100000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0, 3.4e38, 1.2e-30], dtype=np.float32)])
    x = x[(np.abs(x) >= np.float32(1e-30)) | (x == 0)]  # (below 2^-100 the third term leaves bf16's normal range: not activations)
    hi, mid, lo = b3.split(x)
    assert np.array_equal(hi + mid + lo, x)
    for part in (hi, mid, lo):
        assert not (part.view(np.uint32) & np.uint32(0xffff)).any()   # every term is a bf16 number
    assert (np.abs(mid) <= np.abs(x) * 2.0 ** -7).all() and (np.abs(lo) <= np.abs(x) * 2.0 ** -15).all()


@pytest.mark.parametrize("K,N,M", [(240, 80, 960), (672, 112, 960), (1152, 320, 240), (136, 816, 1280), (80, 100, 400), (48, 288, 576), (16, 96, 576)])
def test_six_product_model_is_within_2x_of_an_f32_matmul(K, N, M):
    rng = np.random.default_rng(K + N)
    X = b3.dense_inputs(rng, M, K)
    W, bias = b3.case_weights(K, N)
    ref, D, dead = b3.reference(X, W, bias)
    f32 = b3.statistic(X @ W.T + bias[None, :], ref, D, dead)
    six = b3.statistic(b3.emulate(X, W, bias), ref, D, dead)
    print(f"K={K} N={N}: f32 matmul rms {f32[0]:.3f} tile {f32[1]:.3f} | six products rms {six[0]:.3f} tile {six[1]:.3f}  (2^-24 D)")
    assert six[0] <= 2.0 * f32[0] and six[1] <= 2.0 * f32[1]
    # the three products of order 2^-8 and 1 are no "small terms": without one of them the result is off by thousands of units
    for t in (3, 4, 5):
        assert b3.statistic(b3.emulate(X, W, bias, drop=t), ref, D, dead)[0] >= 1000.0 * six[0]


def test_step_mutants_of_window_inputs_are_what_the_generic_emulation_gives():
    rng = np.random.default_rng(5)
    K, N, rows = 144, 40, 24
    W, bias = b3.case_weights(K, N)
    X, row_step = b3.window_inputs(rng, rows, K, b3.window_list(K))
    Yf = b3.emulate(X, W, bias)
    for t in b3.SMALL_TERMS:
        Yd = b3.emulate(X, W, bias, drop=t)
        for s in (0, 2, b3.n_steps(K) - 1):
            assert np.array_equal(b3.step_mutant(Yf, Yd, row_step, s), b3.emulate(X, W, bias, drop=t, step=s))
        assert np.array_equal(b3.emulate(X, W, bias, drop=t, step="last"), b3.emulate(X, W, bias, drop=t, step=b3.n_steps(K) - 1))
    # a one-tile mutant differs from the faithful result in that tile only
    Yt = b3.emulate_tile_mutant(Yf, X, W, bias, 0, (16, 16))
    diff = Yt != Yf
    assert diff[16:32, 16:32].any() and not diff[:16].any() and not diff[32:].any() and not diff[:, :16].any() and not diff[:, 32:].any()


def test_window_list_covers_first_step_slice_boundary_and_tail():
    for K in (80, 136, 144, 240, 256, 672, 1152, 232, 192):
        wl = b3.window_list(K)
        assert wl[0] == 0 and wl[-1] == (K - 1) // 8 * 8 and all(k % 8 == 0 for k in wl)
        half = (K // 2) // 32 * 32
        assert half in wl and half - 8 in wl
        assert {k // 32 for k in wl} >= {0, b3.n_steps(K) - 1, b3.n_steps(K) - 2}
        if K <= 384:
            assert wl == list(range(0, K, 8))
        else:
            assert len(wl) <= 48


def _operand_sets():
    """(id, K, N, rows per sample, batch sizes) of every GPU case; weights and batches are the GPU test's own (b3_model.case_weights, batches)."""
    for K, N, h, w, kernel in b3.GEMM_CASES:
        yield f"{kernel}-{K}x{N}", K, N, h * w, b3.GEMM_BATCHES
    for cin, h, w, cmid, k in b3.MBROW_CASES:
        yield f"mbrow-{cin}x{cmid}-k{k}", cin, cmid, h * w, (5,)
    for cin, h, w, cmid, k, expect in b3.MBMAP_CASES:
        yield f"mbmap-{cin}x{cmid}-{expect.split()[0]}", cin, cmid, h * w, (5,)


@pytest.mark.parametrize("name,K,N,rows,sizes", [pytest.param(*c, id=c[0]) for c in _operand_sets()])
def test_every_mutant_class_is_16x_the_faithful_model_on_the_gpu_cases_operands(name, K, N, rows, sizes):
    """Classes (a) dropped everywhere, (b) dropped in one tile (several positions), plane swaps: on the dense batches; (c) one k step, (d)
    the last step: on the window batch (a one-step fault is diluted by sqrt(steps) in a dense product).  The operands are the ones the GPU
    test runs -- which asserts the same ratio again next to its bounds."""
    W, bias = b3.case_weights(K, N)
    for batch, (X, row_step) in b3.batches(K, rows, sizes).items():
        r = b3.bounds_of(X, row_step, W, bias)
        print(f"{name} {batch}: model {r['model']} weakest mutant {r['mutant']} {r['names']} bound {r['bound']}")
        assert r["mutant"][0] >= 16.0 * r["model"][0] and r["mutant"][1] >= 16.0 * r["model"][1], (batch, r["model"], r["mutant"], r["names"])
        assert r["dead"].sum() == r["dead"][:, 5].sum() == X.shape[0]   # the dead filter row, nothing else


@pytest.mark.parametrize("which", b3.BANK_CASES)
@pytest.mark.parametrize("start", b3.BANK_STARTS)
def test_filter_bank_model_and_its_mutants(which, start):
    """The fold S[n] = ye[n] + ye[L/2 - n] / D[n] in f32 with the factored tables, against float64 over the ORIGINAL taps: as good as an
    f32 matmul over the original taps (within 2 x), every mutant >= 16 x the model, the dead row is the one dead output per frame."""
    bank, bias, hop = b3.bank_case(which)
    x = b3.bank_signal(which, start)[:, start:start + b3.BANK_SAMPLES]
    F, nf = b3.frames_of(x, bank.L, hop)
    r = b3.fold_bounds(F, bank, bias)
    f32 = b3.statistic(F[:, :bank.L] @ bank.taps.T + bias[None, :], r["ref"], r["D"], r["dead"])
    print(f"{which} start={start}: f32 matmul {f32} model {r['model']} weakest mutant {r['mutant']} {r['names']} bound {r['bound']}")
    assert r["model"][0] <= 2.0 * f32[0] and r["model"][1] <= 2.0 * f32[1]
    assert r["mutant"][0] >= 16.0 * r["model"][0] and r["mutant"][1] >= 16.0 * r["model"][1]
    assert r["dead"].sum() == r["dead"][:, 3].sum() == F.shape[0]
    assert np.array_equal(r["faithful"][:, 3], np.broadcast_to(bias[3], (F.shape[0],)))
