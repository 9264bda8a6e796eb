"""PCEN without a GPU: bn_pcen_thresholds (host only) against its formula, the refusals that need no device, and the reference
tests/pcen_ref.py against the closed form of the rule for a constant input."""
import ctypes as C

import numpy as np
import pytest

import pcen_ref as ref


@pytest.mark.parametrize("max_value", (8.0, 0.3, 1e-40, 3e38))
def test_thresholds_are_the_formula(bn, max_value):
    thr, mx = bn.pcen_thresholds(max_value), float(np.float32(max_value))
    want = ((np.arange(1, 256) - 0.5) * mx / 255.0).astype(np.float32)
    assert thr.dtype == np.float32 and thr.tobytes() == np.maximum.accumulate(want).tobytes() and (np.diff(thr) >= 0).all()


def test_refusals_without_a_device(bn):
    thr = np.full(256, 7.0, dtype=np.float32)
    for mx in (0.0, -1.0, float("nan"), float("inf")):
        assert bn.lib.bn_pcen_thresholds(mx, thr.ctypes.data_as(C.POINTER(C.c_float))) == 1 and "max_value" in bn.last_error()
    assert bn.lib.bn_pcen_thresholds(8.0, None) == 1 and "null" in bn.last_error() and (thr == 7.0).all()
    assert bn.lib.bn_pcen_thresholds(8.0, thr.ctypes.data_as(C.POINTER(C.c_float))) == 0 and thr[255] == 7.0
    sp, ps, out = bn.BnSpectrogramSpec(256, 100, 0, 40, 0, 0.0, 0.0), bn.BnPcenSpec(0, 0.025, 1.0, 0.98, 2.0, 0.5, 1e-6, 0.0), np.full(8, 7.0, dtype=np.float32)
    assert bn.lib.bn_recording_pcen(None, 0, 2, C.byref(sp), 28, None, C.byref(ps), 32, None, None, out.ctypes.data_as(C.c_void_p), 32) == 1
    assert "null recording" in bn.last_error() and (out == 7.0).all()
    err = bn.BnhError()
    assert bn.lib.bnh_recording_pcen(None, 0, 2, C.byref(sp), None, C.byref(ps), None, None, out.ctypes.data_as(C.c_void_p), 32, C.byref(err)) != 0
    assert bn.lib.bnh_pcen_thresholds(0.0, thr.ctypes.data_as(C.POINTER(C.c_float)), C.byref(err)) != 0
    assert C.sizeof(bn.BnPcenSpec) == 32 and (bn.BN_PCEN_SMOOTH_DEPTH, bn.BN_PCEN_VALUE_DEPTH) == tuple(ref.header_constants()[k] for k in ("BN_PCEN_SMOOTH_DEPTH", "BN_PCEN_VALUE_DEPTH"))


@pytest.mark.parametrize("p", ((0.98, 2.0, 0.5, 1e-6), (0.8, 10.0, 0.25, 1e-9), (1.0, 0.0, 1.0, 1e-6)))
def test_the_reference_on_a_constant_input(p):
    """M = x from the first frame on, V = (x / (eps + x)^alpha + delta)^r - delta^r; a non-finite frame is +Inf and changes nothing"""
    alpha, delta, r, eps = (float(np.float32(v)) for v in p)
    E = np.tile(np.array([1e-7, 3e-5, 0.0], np.float32), (50, 1))
    E[20] = np.inf
    V, M, B, bound, M_end, B_end = ref.pcen(E, 0.025, 1e5, *p)
    x = float(np.float32(1e5)) * E[0].astype(np.float64)
    want = (x / (eps + x) ** alpha + delta) ** r - delta ** r
    ok = np.arange(50) != 20
    assert np.abs(M[ok] - x).max() <= 1e-12 * x.max() and np.abs(V[ok] - want).max() <= 1e-12 * (want.max() + 1) and np.isinf(V[20]).all()
    assert (V[:, 2] [ok] == 0).all() and (B[1:][ok[1:]] > 0)[:, :2].all() and (bound[20] == 0).all() and np.abs(M_end - x).max() <= 1e-12 * x.max()
    # a state in front: M decays from it towards x
    _, M2, _, _, _, _ = ref.pcen(E[:10], 0.025, 1e5, *p, state=np.array([5.0, 5.0, 5.0], np.float32))
    assert np.allclose(M2[:, 0], x[0] + (5.0 - x[0]) * (1 - float(np.float32(0.025))) ** np.arange(1, 11), rtol=1e-12)
