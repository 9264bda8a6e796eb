"""Per-site species priors without a GPU: tests/prior_ref.py agrees with the oracle where the two overlap (its AFTER_TOPK rule is
oracle.filter_predictions over the site's full score list; its SELECT rule with nothing known and distinct confidences is oracle.top_k),
the ABI declares and exports the prior entry points, and without a device create refuses with the no-device status.

The tests that take the `bn` fixture need the prior entry points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import prior_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 9
INVALID_ARG = 1
PRIOR_SYMBOLS = ["bn_prior_create", "bn_prior_free", "bn_prior_sites", "bn_prior_species", "bn_prior_threshold", "bn_prior_flags", "bn_prior_read",
                 "bn_prior_apply_host", "bn_ctx_attach_prior", "bn_ctx_prior_site", "bn_step_prior_results"]


def _case(seed, n=97):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal(n) * 3).astype(np.float32)
    logits[10:30] = np.float32(1.25)          # ties, straddling any small K
    logits[40], logits[41] = 20.0, 20.5       # two logits whose sigmoids are the same f32 (1.0)
    prow = rng.uniform(0, 1, n).astype(np.float32)
    prow[rng.uniform(size=n) < 0.25] = prior_ref.UNKNOWN
    prow[12] = np.float32(0.3)                # exactly the threshold: admitted
    prow[13] = np.float32(0.0)
    return logits, prow


@pytest.mark.parametrize("rerank", [False, True])
@pytest.mark.parametrize("top_k", [1, 5, 24, 97])
@pytest.mark.parametrize("min_conf", [None, 0.4])
def test_after_topk_rule_is_the_oracles_filter_predictions(rerank, top_k, min_conf):
    for seed in range(4):
        logits, prow = _case(seed)
        thr = 0.3
        tk = oracle.top_k(logits, top_k, min_conf)
        ps, pc = [t[0] for t in tk], np.array([t[1] for t in tk], dtype=np.float32)
        known = np.nonzero(prow >= 0)[0]          # the site's FULL score list: every species the meta model knows
        pos, conf = oracle.filter_predictions(ps, pc, known, prow[known], thr, rerank)
        gi, gc = prior_ref.after_topk_row(logits, prow, thr, rerank, top_k, min_conf)
        assert np.array_equal(gi, np.array(ps, dtype=np.uint32)[pos])
        assert gc.tobytes() == conf.astype(np.float32).tobytes()


@pytest.mark.parametrize("top_k", [1, 7, 50, 200])
@pytest.mark.parametrize("min_conf", [None, 0.5])
def test_select_rule_with_nothing_known_is_the_oracles_top_k(top_k, min_conf):
    rng = np.random.default_rng(11)
    logits = np.unique((rng.standard_normal(400) * 2).astype(np.float32))[:150]
    rng.shuffle(logits)
    conf = prior_ref.sigmoid_row(logits)
    assert len(np.unique(conf)) == len(conf)      # distinct confidences: the heap's tie arrangement plays no part
    prow = np.full(len(logits), prior_ref.UNKNOWN)
    for rerank in (False, True):
        gi, gc = prior_ref.select_row(conf, prow, 0.3, rerank, top_k, min_conf)
        want = oracle.top_k(logits, top_k, min_conf)
        assert [int(i) for i in gi] == [w[0] for w in want]
        assert gc.tobytes() == np.array([w[1] for w in want], dtype=np.float32).tobytes()


def test_select_rule_orders_ties_by_index_and_total_cmp():
    conf = np.array([0.5, np.nan, 0.5, -np.nan, 0.0, -0.0, 0.5, 1.0], dtype=np.float32)
    prow = np.array([-1, -1, -1, -1, -1, -1, 0.1, -1], dtype=np.float32)
    gi, gc = prior_ref.select_row(conf, prow, 0.3, False, 8)
    assert list(gi) == [1, 7, 0, 2, 4, 5, 3]      # +NaN above everything, -NaN below, +0 above -0, 6 not admitted
    gi, gc = prior_ref.select_row(conf, prow, 0.3, False, 8, 0.0)
    assert list(gi) == [7, 0, 2, 4, 5]            # NaN fails >=, -0 >= 0 holds
    gi, gc = prior_ref.select_row(conf, np.array([0.5, 0.5, 2.0, 0.5, 0.5, 0.5, 0.5, 0.0], dtype=np.float32), 0.3, True, 3)
    assert list(gi) == [1, 2, 0] and gc.tobytes() == np.array([np.nan, 1.0, 0.25], dtype=np.float32).tobytes()


def test_rules_behind_range_filter_scores_match_the_oracle(bn):
    """RangeFilter.scores validates and computes the week as predict does, by the functions compared here (building a RangeFilter
    needs a device: tests/test_gpu_prior.py checks scores itself)."""
    for m in range(0, 14):
        for d in (0, 1, 7, 8, 14, 15, 21, 22, 28, 29, 31, 32):
            if oracle.validate_date(m, d) == 0:
                bn.validate_date(m, d)
                assert bn.calculate_week(m, d) == oracle.calculate_week(m, d)
            else:
                with pytest.raises(bn.Error):
                    bn.validate_date(m, d)
    for lat, lon in ((0.0, 0.0), (90.0, 180.0), (-90.0, -180.0), (90.5, 0.0), (0.0, -180.5), (float("nan"), 0.0), (0.0, float("inf"))):
        if oracle.validate_coordinates(lat, lon) == 0:
            bn.validate_coordinates(lat, lon)
        else:
            with pytest.raises(bn.Error):
                bn.validate_coordinates(lat, lon)


def test_abi_declares_and_exports_the_prior_entry_points(bn):
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    for s in PRIOR_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in bn.ENGINE_SYMBOLS and hasattr(bn.lib, s), s
    for name, value in (("BN_PRIOR_SELECT", "0u"), ("BN_PRIOR_AFTER_TOPK", "1u"), ("BN_PRIOR_RERANK", "2u"), ("BN_PRIOR_UNKNOWN", r"\(-1\.0f\)")):
        assert re.search(r"#define\s+%s\s+%s" % (name, value), header), name
    assert (bn.BN_PRIOR_SELECT, bn.BN_PRIOR_AFTER_TOPK, bn.BN_PRIOR_RERANK, bn.BN_PRIOR_UNKNOWN) == (0, 1, 2, -1.0)
    assert bn.lib.bn_abi_version() == 2
    host = open(os.path.join(ROOT, "include", "birdnet_host.h")).read()
    for s in ("bnh_range_filter_scores", "bnh_range_filter_prior_row", "bnh_prior_create", "bnh_prior_free", "bnh_prior_handle",
              "bnh_context_attach_prior", "bnh_context_set_prior_site", "bnh_context_prior_results"):
        assert re.search(r"\b%s\s*\(" % s, host) and s in bn.HOST_SYMBOLS and hasattr(bn.lib, s), s


def test_without_a_device_create_refuses_and_bad_arguments_are_named_first(bn):
    table = np.full((2, 5), 0.5, dtype=np.float32)
    f32p = C.POINTER(C.c_float)
    h = C.c_void_p()

    def create(n_sites, n_species, t, thr, flags):
        return bn.lib.bn_prior_create(0, n_sites, n_species, None if t is None else t.ctypes.data_as(f32p), C.c_float(thr), flags, C.byref(h))

    # refusals of the arguments do not need a device
    bad = table.copy()
    bad[1, 3] = np.inf
    for args in ((0, 5, table, 0.1, 0), (2, 5, None, 0.1, 0), (2, 5, bad, 0.1, 0), (2, 5, table, float("nan"), 0), (2, 5, table, 0.1, 4)):
        assert create(*args) == INVALID_ARG and bn.last_error() and not h.value, args
    if bn.device_count() > 0:  # with a device the same call succeeds
        assert create(2, 5, table, 0.1, 0) == 0 and h.value
        bn.lib.bn_prior_free(h)
        return
    assert create(2, 5, table, 0.1, 0) == NO_DEVICE and not h.value
    assert "device" in bn.last_error()
    with pytest.raises(bn.EngineError) as e:
        bn.Prior(0, table, 0.1)
    assert e.value.status == NO_DEVICE
