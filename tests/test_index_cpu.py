"""CPU-side checks of the embedding index's C ABI (bn_index_*): exported, bound in the Rust FFI, and refused without a gfx950
device instead of falling back to a host search; argument checks that come before any device call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_SYMBOLS = ["bn_index_create", "bn_index_free", "bn_index_size", "bn_index_dim", "bn_index_add_host", "bn_index_add_ctx",
                 "bn_index_read", "bn_index_search", "bn_index_search_ids"]


def test_every_index_symbol_is_declared_exported_and_bound(bn):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "birdnet_hip.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    L = C.CDLL(bn.LIB_PATH)
    for name in INDEX_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bn.ENGINE_SYMBOLS, name
        assert re.search(r"pub fn %s\(" % name, ffi), name
    assert "pub struct bn_index" in ffi


def test_no_device_means_loud_failure_not_cpu_fallback(bn):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    with pytest.raises(bn.EngineError) as e:
        bn.Index(0, 128, 16)
    assert e.value.status == 9  # BN_ERR_NO_DEVICE


def test_arguments_refused_before_any_device_call(bn):
    h = C.c_void_p()
    assert bn.lib.bn_index_create(0, 0, 16, C.byref(h)) == 1  # dim = 0
    assert "dim" in bn.last_error()
    assert bn.lib.bn_index_create(0, 128, 0, C.byref(h)) == 1  # capacity = 0
    assert "capacity" in bn.last_error()
    assert bn.lib.bn_index_create(0, 128, 16, None) == 1  # null out pointer
    assert not h.value
    # null handles: refused, and the queries of a null index answer 0
    assert bn.lib.bn_index_add_host(None, None, 0, None) == 1
    assert bn.lib.bn_index_add_ctx(None, None, 1, None) == 1
    assert bn.lib.bn_index_read(None, 0, 0, None) == 1
    assert bn.lib.bn_index_search(None, None, 0, 1, 1, None, None, None) == 1
    assert bn.lib.bn_index_search_ids(None, None, 0, -1, 1, 1, None, None, None) == 1
    assert bn.lib.bn_index_size(None) == 0 and bn.lib.bn_index_dim(None) == 0
    bn.lib.bn_index_free(None)
