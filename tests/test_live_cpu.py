"""CPU-side checks of the live ingest pool's C ABI (bn_live_*, bn_step_live): exported, declared, bound in the Rust FFI and the
package's tables, refused without a gfx950 device instead of falling back to host windowing, and argument checks that come
before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE_SYMBOLS = ["bn_live_create", "bn_live_free", "bn_live_push", "bn_live_push_many", "bn_live_close", "bn_live_reset",
                "bn_live_ready", "bn_live_room", "bn_live_event_count", "bn_live_read_window", "bn_step_live"]
HOST_LIVE_SYMBOLS = ["bnh_live_create", "bnh_live_free", "bnh_live_push", "bnh_live_close", "bnh_live_ready", "bnh_predict_live"]


def test_every_live_symbol_is_declared_exported_and_bound(bn):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "birdnet_hip.h")).read(), flags=re.S)
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "birdnet_host.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    L = C.CDLL(bn.LIB_PATH)
    for name in LIVE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bn.ENGINE_SYMBOLS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    for name in HOST_LIVE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, host), name
        assert hasattr(L, name), name
        assert name in bn.HOST_SYMBOLS, name
    assert "pub struct bn_live" in ffi
    assert "class LiveSources" in host and "predict_live(" in host


def test_no_device_means_loud_failure_not_cpu_fallback(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(bn.EngineError) as e:
        bn.Live(0, 4, 144000, 72000, 144000 * 3)
    assert e.value.status == 9  # BN_ERR_NO_DEVICE


def test_arguments_refused_before_any_device_call(bn):
    h = C.c_void_p()
    S = 144000
    assert bn.lib.bn_live_create(0, 4, 7, S, S, 2 * S, C.byref(h)) == 1  # unknown format
    assert "format" in bn.last_error()
    assert bn.lib.bn_live_create(0, 0, 0, S, S, 2 * S, C.byref(h)) == 1  # no sources
    assert bn.lib.bn_live_create(0, 4, 0, S + 2, S, 2 * S + 2, C.byref(h)) == 1  # S % 4 != 0
    assert bn.lib.bn_live_create(0, 4, 0, S, 0, 2 * S, C.byref(h)) == 1  # step 0
    assert bn.lib.bn_live_create(0, 4, 0, S, S + 4, 3 * S, C.byref(h)) == 1  # step > S
    assert bn.lib.bn_live_create(0, 4, 0, S, S // 2, S + S // 2 - 1, C.byref(h)) == 1  # ring < S + step
    assert "ring" in bn.last_error()
    assert bn.lib.bn_live_create(0, 4, 0, S, S, 2 * S, None) == 1  # null out pointer
    assert not h.value
    # null pools: refused, and the queries of a null pool answer 0
    buf = (C.c_int16 * 4)()
    assert bn.lib.bn_live_push(None, 0, C.cast(buf, C.c_void_p), 4) == 1
    assert "null" in bn.last_error()
    assert bn.lib.bn_live_push_many(None, 0, None, None, None) == 1
    assert bn.lib.bn_live_close(None, 0) == 1
    assert bn.lib.bn_live_reset(None, 0) == 1
    assert bn.lib.bn_live_read_window(None, 0, 0, None) == 1
    n = C.c_size_t(7)
    assert bn.lib.bn_step_live(None, None, 1, 1, 0, C.c_float(0.0), None, None, C.byref(n), 0) == 1
    assert bn.lib.bn_live_ready(None, -1) == 0 and bn.lib.bn_live_room(None, 0) == 0 and bn.lib.bn_live_event_count(None) == 0
    bn.lib.bn_live_free(None)
