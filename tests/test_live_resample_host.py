"""CPU-side checks of the resampling live pool (bn_live_create_rates): bn_live_resampled_samples -- how many outputs of a
resampled stream are final after `pushed` source samples -- against a brute force over resample_kernel's tap indexing
(output n reads source indices up to (n*M)//L + T//2), its monotonicity, the T - 1 history the streaming kernel carries, and
that the new entry points are declared, exported and bound, and refuse bad arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(48000, 32000), (44100, 48000), (44100, 32000), (16000, 48000), (96000, 32000), (32000, 32000)]
LARGE = [100003, 1234567]


def factors(bn, src, dst, zc):
    _, L, M, T = bn.resample_table(src, dst, zc)
    return int(L), int(M), int(T)


def brute_final(L, M, T, pushed):
    """count of outputs n with (n*M)//L + T//2 < pushed: final outputs form a prefix, so count until the first that is not"""
    n = np.arange(0, (pushed * L) // M + 2, dtype=np.int64)
    final = (n * M) // L + T // 2 < pushed
    count = int(final.sum())
    assert final[:count].all() and not final[count:].any()
    return count


@pytest.mark.parametrize("zc", [0, 8])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_final_outputs_match_the_tap_indexing(bn, src, dst, zc):
    L, M, T = factors(bn, src, dst, zc)
    f = bn.lib.bn_live_resampled_samples
    for pushed in list(range(0, 4 * T)) + LARGE:
        closed = -(-pushed * L // M)
        if src == dst:
            assert f(src, dst, zc, pushed, 0) == pushed and f(src, dst, zc, pushed, 1) == pushed
            continue
        assert f(src, dst, zc, pushed, 0) == brute_final(L, M, T, pushed), (src, dst, zc, pushed)
        assert f(src, dst, zc, pushed, 1) == closed, (src, dst, zc, pushed)
        assert bn.live_resampled_samples(src, dst, pushed, False, zc) == f(src, dst, zc, pushed, 0)
        assert bn.live_resampled_samples(src, dst, pushed, True, zc) == closed


@pytest.mark.parametrize("zc", [0, 8])
@pytest.mark.parametrize("src,dst", PAIRS)
def test_final_outputs_are_monotonic_and_below_the_closed_count(bn, src, dst, zc):
    L, M, T = factors(bn, src, dst, zc)
    f = bn.lib.bn_live_resampled_samples
    for p in list(range(0, 4 * T)) + LARGE:
        a, b, c = f(src, dst, zc, p, 0), f(src, dst, zc, p + 1, 0), f(src, dst, zc, p + 1, 1)
        assert a <= b <= c, (src, dst, zc, p, a, b, c)
        # the tail a close flushes is at most ceil(T/2 * L / M) + 1 outputs
        assert f(src, dst, zc, p, 1) - a <= (0 if src == dst else -(-(T // 2) * L // M) + 1)


@pytest.mark.parametrize("zc", [0, 8])
@pytest.mark.parametrize("src,dst", [p for p in PAIRS if p[0] != p[1]])
def test_a_history_of_T_minus_1_source_samples_suffices(bn, src, dst, zc):
    """the earliest tap of the first output that a push makes final lies at most T - 1 samples before the push"""
    L, M, T = factors(bn, src, dst, zc)
    f = bn.lib.bn_live_resampled_samples
    worst = 0
    for p in list(range(0, 4 * T)) + LARGE:
        n = f(src, dst, zc, p, 0)  # first output not final at p
        first_tap = (n * M) // L - (T // 2 - 1)
        worst = max(worst, p - max(first_tap, 0))
        assert p - first_tap <= T - 1 or first_tap < 0, (p, n, first_tap)
    assert worst == T - 1


def test_zero_rates_yield_zero(bn):
    f = bn.lib.bn_live_resampled_samples
    assert f(0, 32000, 0, 1000, 0) == 0 and f(48000, 0, 0, 1000, 1) == 0


def test_new_symbols_are_declared_exported_and_bound(bn):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "birdnet_hip.h")).read(), flags=re.S)
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "birdnet_host.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    lib = C.CDLL(bn.LIB_PATH)
    for name in ("bn_live_create_rates", "bn_live_resampled_samples", "bn_live_source_rate"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in bn.ENGINE_SYMBOLS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert re.search(r"\bbnh_live_create_rates\s*\(", host) and hasattr(lib, "bnh_live_create_rates")
    assert "bnh_live_create_rates" in bn.HOST_SYMBOLS
    assert "source_rates" in host


def test_arguments_refused_before_any_device_call(bn):
    h = C.c_void_p()
    S = 96000
    rates = (C.c_uint32 * 2)(48000, 0)
    create = bn.lib.bn_live_create_rates
    assert create(0, 2, 0, S, S, 3 * S, 32000, rates, 0, C.byref(h)) == 1  # a zero source rate
    assert "source 1" in bn.last_error()
    rates[1] = 44100
    assert create(0, 2, 0, S, S, 3 * S, 0, rates, 0, C.byref(h)) == 1  # a zero model rate
    assert create(0, 2, 0, S, S, 3 * S, 32000, None, 0, C.byref(h)) == 1  # no rates
    assert create(0, 2, 7, S, S, 3 * S, 32000, rates, 0, C.byref(h)) == 1  # unknown format
    assert create(0, 2, 0, S + 2, S, 3 * S, 32000, rates, 0, C.byref(h)) == 1  # S % 4 != 0
    assert h.value is None
    assert bn.lib.bn_live_source_rate(None, 0) == 0
