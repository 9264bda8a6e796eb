"""The float64 restatement of the denoiser (tests/denoise_ref.py) and bn_noise_floor, without a GPU.

The wrong-reference checks run at every frame length on the bound test's own inputs of test_gpu_denoise.py (denoise_ref.case: white
noise plus a tone, alpha 2, floor_gain 0.1, the true noise level) at n = W = 4 RUN H, where all five wrong rules leave the bound, and
at the longest, n = 2 W + H + 3, where four do: there, as at n = W + 1, the last frame holds three (one) samples under window values
below 0.04 (w_0 = 0), so by the rule itself it adds less than the bound allows (nothing), and dropping it is not wrong.  The shorter
lengths are no evidence either way: at n = 1 the only sample sits under w = 1 and every bin of its frame has the same power."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as ref


@pytest.mark.parametrize("N", ref.FRAMES)
def test_restatement_reconstructs_and_wrong_rules_leave_the_bound(bn, N):
    H = N // 2
    W = 4 * bn.BN_DENOISE_RUN * H
    for n, wrongs in ((W, ref.WRONG), (2 * W + H + 3, ref.WRONG[:4])):
        v, noise = ref.case(N, n)
        x = v.astype(np.float32) / np.float32(32768.0)
        same, _ = ref.denoise(x, N, 0.0, 0.1, noise)
        assert np.abs(same - x).max() <= 1e-12 * np.abs(x).max()
        y, E = ref.denoise(x, N, 2.0, 0.1, noise)
        assert ref.shares(y, y, E, N).max() == 0.0 and 0.2 < np.sqrt((y ** 2).mean() / (x.astype(np.float64) ** 2).mean()) < 0.98  # it gates, and keeps the tone
        for wrong in wrongs:
            worst = ref.shares(ref.denoise(x, N, 2.0, 0.1, noise, wrong=wrong)[0], y, E, N).max()
            print(N, n, wrong, "leaves the bound by a factor", worst)
            assert worst > 1.0, wrong


def test_the_clamped_known_answer_is_clamped(bn):
    """test_gpu_denoise's known answer: white noise under noise = 4 x its level, alpha 1.  A bin passes the clamp when
    P > 4 m / (1 - floor_gain); P / m is exponential, so at floor_gain 0.75 that is P > 16 m, e^-16 per bin and frame"""
    N, n = 512, 5000
    x = (np.random.RandomState(3).standard_normal(n) * 0.1).astype(np.float32)
    y, _ = ref.denoise(x, N, 1.0, 0.75, 4 * ref.white_level(N, 0.1))
    assert np.abs(y - 0.75 * x.astype(np.float64)).max() <= 1e-12


def test_noise_floor_against_numpy_sort(bn):
    rng = np.random.RandomState(5)
    planes = rng.uniform(0, 1, (7, 3, 9)).astype(np.float32)
    planes[2] = np.inf  # a BN_LEVEL_NONFINITE window sorts last
    for q, rank in ((0.0, 0), (0.25, 1), (0.5, 3), (0.99, 5), (1.0, 6)):
        assert bn.noise_floor(planes, q).tolist() == np.sort(planes[:, 0, :], axis=0)[rank].tolist()
    out = (C.c_float * 9)(*([7.0] * 9))
    p = planes.ctypes.data_as(C.POINTER(C.c_float))
    for args, word in (((p, 0, 9, 0.5, out), "count"), ((p, 7, 9, 1.5, out), "quantile"), ((p, 7, 9, float("nan"), out), "quantile"), ((None, 7, 9, 0.5, out), "null"),
                       ((p, 7, 9, 0.5, None), "null")):
        assert bn.lib.bn_noise_floor(*args) == 1 and word in bn.last_error() and list(out) == [7.0] * 9
