"""Detection events without a GPU: hand-written sequences for tests/track_ref.py itself (the restatement of the contract the device is
compared against in tests/test_gpu_track.py), the ABI's declarations, and the no-device status of create.

The tests that take the `bn` fixture need the tracker entry points and fail where the library lacks them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import track_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = 9
INVALID_ARG = 1
TRACK_SYMBOLS = ["bn_track_create", "bn_track_free", "bn_track_sources", "bn_track_species", "bn_track_open_events", "bn_track_update_host",
                 "bn_track_flush", "bn_track_reset", "bn_ctx_attach_track", "bn_ctx_track_source", "bn_step_track_results"]
HI, LO = 3.0, -3.0     # logits of a hit and of a miss at enter_conf 0.5
ENTER = 0.5


def _run(pattern, windows=None, min_hits=1, max_gap=0, logits=None):
    """One source, one species: pattern[i] truthy = a hit in window windows[i] (default i).  Events of the updates, then of the flush."""
    t = track_ref.Tracker(1, 1, ENTER, min_hits, max_gap)
    windows = list(range(len(pattern))) if windows is None else windows
    x = np.array([[HI if h else LO] for h in pattern], dtype=np.float32) if logits is None else np.asarray(logits, dtype=np.float32).reshape(-1, 1)
    ev = t.update(x, [0] * len(windows), windows)
    return ev, t.flush(), t


def _spans(ev):
    return [(int(e["first_window"]), int(e["last_window"]), int(e["hits"])) for e in ev]


def test_a_gap_of_max_gap_merges_and_one_more_splits():
    for gap in (0, 1, 3):
        merged = [1] + [0] * gap + [1]
        ev, fl, _ = _run(merged, max_gap=gap)
        assert _spans(ev) == [] and _spans(fl) == [(0, gap + 1, 2)]
        split = [1] + [0] * (gap + 1) + [1]
        ev, fl, _ = _run(split, max_gap=gap)
        assert _spans(ev) == [(0, 0, 1)] and _spans(fl) == [(gap + 2, gap + 2, 1)]
    # the event closes in the window that makes the misses exceed max_gap, not at the next hit
    t = track_ref.Tracker(1, 1, ENTER, 1, 1)
    assert len(t.update([[HI]], [0], [0])) == 0 and len(t.update([[LO]], [0], [1])) == 0 and t.open_events() == 1
    assert _spans(t.update([[LO]], [0], [2])) == [(0, 0, 1)] and t.open_events() == 0


def test_min_hits_drops_short_events_silently():
    ev, fl, t = _run([1, 1, 0, 1, 0, 1, 1, 1], min_hits=3)
    assert _spans(ev) == [] and _spans(fl) == [(5, 7, 3)] and t.open_events() == 0
    ev, fl, _ = _run([1, 1, 0, 1], min_hits=2)
    assert _spans(ev) == [(0, 1, 2)] and _spans(fl) == []     # the single hit at the end is dropped by the flush too


def test_a_window_number_that_never_arrives_counts_as_a_miss():
    ev, fl, _ = _run([1, 1], windows=[4, 6], max_gap=0)
    assert _spans(ev) == [(4, 4, 1)] and _spans(fl) == [(6, 6, 1)]
    ev, fl, _ = _run([1, 1], windows=[4, 6], max_gap=1)
    assert _spans(ev) == [] and _spans(fl) == [(4, 6, 2)]
    ev, fl, _ = _run([1, 0], windows=[4, 6], max_gap=1)      # window 5 missing + window 6 a miss: two misses
    assert _spans(ev) == [(4, 4, 1)] and _spans(fl) == []


def test_peak_mean_and_the_earliest_peak_wins_ties():
    z = [1.0, 2.5, 0.5, 2.5, 2.0]
    ev, fl, _ = _run(None, windows=[3, 4, 5, 6, 7], logits=z)
    assert len(ev) == 0 and len(fl) == 1
    e = fl[0]
    conf = np.array([oracle.sigmoid(v) for v in z], dtype=np.float32)
    total = np.float32(0)
    for c in conf:
        total = np.float32(total + c)
    assert (e["first_window"], e["last_window"], e["hits"], e["peak_window"]) == (3, 7, 5, 4)
    assert e["peak_conf"].tobytes() == conf[1].tobytes() and e["mean_conf"].tobytes() == (total / np.float32(5)).tobytes()
    assert fl.dtype == track_ref.EVENT_DTYPE and fl.dtype.itemsize == 32


def test_nan_is_never_a_hit_and_the_threshold_itself_is():
    ev, fl, _ = _run(None, windows=[0, 1, 2, 3], logits=[np.nan, -np.nan, np.inf, -np.inf])
    assert _spans(ev) == [(2, 2, 1)] and _spans(fl) == [] and ev[0]["peak_conf"] == 1.0   # closed by the miss in window 3
    t = track_ref.Tracker(1, 2, oracle.sigmoid(0.25))
    t.update([[0.25, 0.2499]], [0], [0])                    # conf == enter_conf is a hit, the next lower confidence is not
    assert [int(e["species"]) for e in t.flush()] == [0]


def test_flush_one_source_or_all_and_reset():
    t = track_ref.Tracker(3, 2, ENTER)
    x = np.full((3, 2), HI, dtype=np.float32)
    assert len(t.update(x, [2, 0, 1], [5, 5, 5])) == 0 and t.open_events() == 6 and t.open_events(1) == 2
    fl = t.flush(1)
    assert [(int(e["source"]), int(e["species"])) for e in fl] == [(1, 0), (1, 1)] and t.open_events() == 4
    t.reset(2)
    assert t.open_events(2) == 0 and t.last_window[2] == -1 and t.last_window[0] == 5
    assert len(t.update(x[:1], [2], [0])) == 0                 # a reset source starts over at any window
    with pytest.raises(AssertionError):
        t.update(x[:1], [0], [5])                              # any other must go on increasing, after a flush too
    fl = t.flush()
    assert [(int(e["source"]), int(e["species"]), int(e["first_window"])) for e in fl] == [(0, 0, 5), (0, 1, 5), (2, 0, 0), (2, 1, 0)]
    assert t.open_events() == 0 and len(t.flush()) == 0


def test_two_events_of_one_source_and_species_in_one_update_and_sorting():
    t = track_ref.Tracker(2, 2, ENTER)
    #          source 1            source 0 (rows of the sources interleaved)
    rows = [(1, 0, [HI, LO]), (0, 0, [LO, HI]), (1, 1, [LO, LO]), (1, 2, [HI, HI]), (0, 1, [LO, LO]), (1, 3, [LO, LO])]
    ev = t.update([r[2] for r in rows], [r[0] for r in rows], [r[1] for r in rows])
    assert [(int(e["source"]), int(e["species"]), int(e["first_window"])) for e in ev] == [(0, 1, 0), (1, 0, 0), (1, 0, 2), (1, 1, 2)]
    assert t.open_events() == 0


def test_prior_gates_hits_and_reranks_confidences():
    table = np.array([[0.5, 0.1, -1.0, 0.9], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    x = np.full((2, 4), HI, dtype=np.float32)
    t = track_ref.Tracker(1, 4, ENTER, prior=(table, 0.3, False))
    ev = t.update(x, [0, 0], [0, 1], sites=[0, 1])
    # species 1 is not admitted at site 0; site 1 admits nothing, so window 1 is a miss for all and closes what window 0 opened
    assert [(int(e["species"]), int(e["hits"])) for e in ev] == [(0, 1), (2, 1), (3, 1)] and len(t.flush()) == 0
    t = track_ref.Tracker(1, 4, ENTER, prior=(table, 0.3, True))
    t.update(x[:1], [0], [0], sites=[0])
    fl = t.flush()
    c = np.float32(oracle.sigmoid(HI))
    assert [int(e["species"]) for e in fl] == [2, 3]           # 0.95 * 0.5 falls below 0.5; the unknown species keeps its confidence
    assert fl[0]["peak_conf"].tobytes() == c.tobytes() and fl[1]["peak_conf"].tobytes() == np.float32(c * np.float32(0.9)).tobytes()


def test_abi_declares_and_exports_the_tracker_entry_points(bn):
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    for s in TRACK_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert s in bn.ENGINE_SYMBOLS and hasattr(bn.lib, s), s
    assert re.search(r"#define\s+BN_TRACK_PRIOR\s+1u", header) and bn.BN_TRACK_PRIOR == 1
    assert re.search(r"typedef struct bn_event \{", header)
    assert C.sizeof(bn.BnEvent) == 32 == bn.EVENT_DTYPE.itemsize
    assert [(n, bn.EVENT_DTYPE.fields[n][1]) for n in bn.EVENT_DTYPE.names] == [(f[0], getattr(bn.BnEvent, f[0]).offset) for f in bn.BnEvent._fields_]
    assert bn.EVENT_DTYPE == track_ref.EVENT_DTYPE
    assert bn.lib.bn_abi_version() == 2


def test_without_a_device_create_refuses_and_bad_arguments_are_named_first(bn):
    h = C.c_void_p()

    def create(n_sources, n_species, enter, min_hits, max_gap, max_events, flags):
        return bn.lib.bn_track_create(0, n_sources, n_species, C.c_float(enter), min_hits, max_gap, max_events, flags, C.byref(h))

    # refusals of the arguments do not need a device
    for args in ((0, 5, 0.5, 1, 0, 8, 0), (2, 0, 0.5, 1, 0, 8, 0), (2, 5, 0.5, 1, 0, 0, 0), (2, 5, float("nan"), 1, 0, 8, 0),
                 (2, 5, float("inf"), 1, 0, 8, 0), (2, 5, 0.5, 0, 0, 8, 0), (2, 5, 0.5, 1, 0, 8, 2)):
        assert create(*args) == INVALID_ARG and bn.last_error() and not h.value, args
    assert bn.lib.bn_track_create(0, 2, 5, C.c_float(0.5), 1, 0, 8, 0, None) == INVALID_ARG
    if bn.device_count() > 0:  # with a device the same call succeeds
        assert create(2, 5, 0.5, 1, 0, 8, 0) == 0 and h.value
        assert (bn.lib.bn_track_sources(h), bn.lib.bn_track_species(h), bn.lib.bn_track_open_events(h, -1)) == (2, 5, 0)
        bn.lib.bn_track_free(h)
        return
    assert create(2, 5, 0.5, 1, 0, 8, 0) == NO_DEVICE and not h.value
    assert "device" in bn.last_error()
    with pytest.raises(bn.EngineError) as e:
        bn.Tracker(0, 2, 5, 0.5)
    assert e.value.status == NO_DEVICE
    n, d = C.c_size_t(), C.c_size_t()
    assert bn.lib.bn_track_flush(None, -1, None, 0, C.byref(n), C.byref(d)) == NO_DEVICE
    assert bn.lib.bn_track_update_host(None, None, 1, None, None, None, None, None, 0, C.byref(n), C.byref(d)) == NO_DEVICE
    assert bn.lib.bn_track_sources(None) == 0 and bn.lib.bn_track_open_events(None, 0) == 0
