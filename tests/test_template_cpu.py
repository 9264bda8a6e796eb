"""Template matching without a GPU: bn_template_peaks (host only) against tests/template_ref.py byte for byte, its refusals, and
the integer rule of template_ref.scores against numpy.corrcoef: it is the Pearson correlation of the two code images."""
import ctypes as C

import numpy as np
import pytest

import template_ref as ref

NAN = np.float32(np.nan)
ROWS = {
    "plateau": [[0.5, 0.9, 0.9, 0.9, 0.2, 0.9, 0.9]],
    "ramp": [np.arange(12) / 12.0],  # monotone: exactly one hit at any radius >= 1
    "ends": [[0.9, 0.1, 0.2, 0.3, 0.2, 0.1, 0.95], [0.8, 0.8, 0.1, 0.1, 0.1, 0.7, 0.7]],
    "nans": [[NAN, 0.6, NAN, 0.7, 0.65, NAN, NAN, 0.2], [NAN] * 8],
    "random": np.random.RandomState(3).randint(0, 6, size=(3, 40)) / 5.0,  # many ties
}


@pytest.mark.parametrize("radius", (0, 1, 5))
@pytest.mark.parametrize("name", sorted(ROWS))
def test_peaks_equal_the_reference(bn, name, radius):
    sc = np.array(ROWS[name], dtype=np.float32)
    want, _ = ref.peaks(sc, 0.3, radius)
    got = bn.template_peaks(sc, 0.3, radius)
    assert got.tobytes() == np.array(want, dtype=bn.TEMPLATE_HIT_DTYPE).tobytes(), (got, want)
    if name == "ramp" and radius:
        assert got["offset"].tolist() == [11]
    # cap below the total: the first hits, and the total all the same
    cap, n = max(len(want) - 1, 0), C.c_size_t(0)
    out = np.zeros(cap + 1, dtype=bn.TEMPLATE_HIT_DTYPE)
    assert bn.lib.bn_template_peaks(sc.ctypes.data_as(C.POINTER(C.c_float)), *sc.shape, 0.3, radius, out.ctypes.data_as(C.POINTER(bn.BnTemplateHit)), cap, 16,
                                    C.byref(n)) == 0
    assert n.value == len(want) and out[:cap].tobytes() == got[:cap].tobytes() and not out[cap:].tobytes().strip(b"\0")


def test_peaks_refusals(bn):
    sc, out, n = np.ones((1, 4), dtype=np.float32), np.zeros(4, dtype=bn.TEMPLATE_HIT_DTYPE), C.c_size_t(77)
    sp, op = sc.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(bn.BnTemplateHit))
    for args, word in (((None, 1, 4, 0.5, 1, op, 4, 16, C.byref(n)), "null"), ((sp, 1, 4, 0.5, 1, None, 4, 16, C.byref(n)), "null"),
                       ((sp, 1, 4, 0.5, 1, op, 4, 16, None), "null"), ((sp, 1, 4, 0.5, 1, op, 4, 15, C.byref(n)), "struct_size"),
                       ((sp, 1, 4, float("nan"), 1, op, 4, 16, C.byref(n)), "NaN")):
        assert bn.lib.bn_template_peaks(*args) == 1 and word in bn.last_error(), (word, bn.last_error())
    assert n.value == 77 and not out.tobytes().strip(b"\0")
    assert [bn.lib.bn_templates_count(None), bn.lib.bn_templates_rows(None), bn.lib.bn_templates_max_frames(None)] == [0, 0, 0]


def test_the_integer_rule_is_the_pearson_correlation():
    rng = np.random.RandomState(11)
    image = rng.randint(0, 256, size=(30, 9)).astype(np.uint8)
    templates = [rng.randint(0, 256, size=(W, 9)).astype(np.uint8) for W in (1, 4, 7)] + [image[5:11].copy()]
    got = ref.scores(image, templates, np.float64)
    for q, t in enumerate(templates):
        for o in range(got.shape[1]):
            assert abs(got[q, o] - np.corrcoef(t.reshape(-1).astype(np.float64), image[o:o + len(t)].reshape(-1).astype(np.float64))[0, 1]) <= 1e-12
    assert got.shape == (4, 24) and ref.scores(image, templates)[3, 5] == 1.0 and ref.scores(image, templates).dtype == np.float32
    assert ref.scores(np.full((5, 9), 7, np.uint8), templates[:1]).tobytes() == bytes(5 * 4)  # a flat window: +0.0f
