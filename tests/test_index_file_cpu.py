"""The index file format without a GPU: bn_index_file_info and bn_index_file_verify (host only) against the numpy writer of
tests/index_file_ref.py, their refusals one by one, the stand-alone sanitizer build of the reader, and bn_index_load's refusal on a
machine without a device.  Every test here calls the new entry points and fails where the library lacks them."""
import ctypes as C
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import index_file_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, MODEL_LOAD, NO_DEVICE = 1, 6, 9
NAMES = ("bn_index_save", "bn_index_load", "bn_index_file_info", "bn_index_file_verify")


def stored_rows(n, dim, seed=0):
    """rows as an index would hold them: unit rows, with all-zero rows and -0.0 elements among them"""
    rng = np.random.default_rng(seed + 1000 * n + dim)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x /= np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32) if n else 1
    x = x.astype(np.float32)
    if n > 2:
        x[n // 2] = 0                      # an invalid row
        x[n - 1] = -0.0                    # an invalid row of negative zeros
        x[1, ::2] = -0.0                   # a valid row with negative zeros
        x[1, 1] = 1.0
    elif n == 1:
        x[0, 0] = -0.0
    return x


def write(tmp_path, data, name="x.bnindex"):
    p = tmp_path / name
    p.write_bytes(data)
    return str(p)


def refused(bn, call):
    with pytest.raises(bn.EngineError) as e:
        call()
    assert e.value.status == MODEL_LOAD, e.value
    return e.value


def test_header_library_harness_and_rust_agree(bn):
    L = C.CDLL(bn.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "src", "ffi.rs")).read()
    for name in NAMES:
        assert hasattr(L, name) and name in bn.ENGINE_SYMBOLS
        assert "bn_status %s(" % name in header and "pub fn %s(" % name in ffi
    assert "pub struct bn_index_file_info_t {" in ffi
    assert bn.lib.bn_abi_version() == 2
    assert all(hasattr(bn.Index, m) for m in ("save", "load")) and hasattr(bn, "index_file_info") and hasattr(bn, "index_file_verify")


def test_reference_digest_is_the_documented_function(bn, tmp_path):
    """splitmix64's finaliser over u * golden + b, by hand in Python integers: the numpy reference agrees with it, and so does the
    library, on a one-chunk file whose header and table are put together here from those integers"""
    M = (1 << 64) - 1

    def term(u, b):
        z = (u * 0x9E3779B97F4A7C15 + b) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    us = [0, 1, 13, 2 ** 31, 2 ** 40 + 7, 2 ** 52 - 1]
    bs = [0, 0x80000000, 0x3F800000, 0xFFFFFFFF, 1, 0x7F800000]
    got = fr.terms(np.array(us, dtype=np.uint64), np.array(bs, dtype=np.uint32))
    assert [int(g) for g in got] == [term(u, b) for u, b in zip(us, bs)]
    assert fr.digest(np.array(us, dtype=np.uint64), np.array(bs, dtype=np.uint32)) == sum(term(u, b) for u, b in zip(us, bs)) & M
    row = np.array([[0.5, -0.0, -2.0, 1e-40, 3.0]], dtype=np.float32)  # a negative zero and a subnormal among them
    bits = [int(b) for b in row.view(np.uint32)[0]]
    head = b"BNINDEX1" + struct.pack("<IIQIIQ", 1, 5, 1, 9, 1, 1) + bytes(16)
    words = struct.unpack("<14I", head)
    data = (head + struct.pack("<Q", sum(term(w, v) for w, v in enumerate(words)) & M)
            + struct.pack("<Q", sum(term(k, b) for k, b in enumerate(bits)) & M) + row.tobytes())
    assert data == fr.file_bytes(row, 9)
    p = write(tmp_path, data)
    bn.index_file_verify(p)
    assert bn.index_file_info(p) == {"dim": 5, "rows": 1, "valid_rows": 1, "chunk_rows": 9, "n_chunks": 1, "version": 1}


@pytest.mark.parametrize("chunk_rows", [1, 7, 1000])
@pytest.mark.parametrize("dim", [3, 130])
@pytest.mark.parametrize("rows", [0, 1, 65])
def test_reference_files_verify_and_report_their_fields(bn, tmp_path, rows, dim, chunk_rows):
    x = stored_rows(rows, dim)
    data = fr.file_bytes(x, chunk_rows)
    assert len(data) == 64 + 8 * -(-rows // chunk_rows) + 4 * rows * dim
    p = write(tmp_path, data)
    bn.index_file_verify(p)
    want = {"dim": dim, "rows": rows, "valid_rows": int(fr.valid_mask(x).sum()), "chunk_rows": chunk_rows, "n_chunks": -(-rows // chunk_rows),
            "version": 1}
    assert bn.index_file_info(p) == want
    if rows == 65:
        assert want["valid_rows"] == 63
    fields, _, payload = fr.read(data)
    assert fields == want and payload.tobytes() == x.tobytes()


def test_verify_names_the_chunk_of_a_flipped_payload_byte(bn, tmp_path):
    rows, dim, chunk_rows = 65, 130, 7
    data = bytearray(fr.file_bytes(stored_rows(rows, dim), chunk_rows))
    payload = 64 + 8 * 10
    for row, chunk in ((0, 0), (6, 0), (7, 1), (40, 5), (64, 9)):
        t = bytearray(data)
        t[payload + 4 * (row * dim + 5) + 1] ^= 0x10
        e = refused(bn, lambda: bn.index_file_verify(write(tmp_path, bytes(t))))
        assert e.first_bad_chunk == chunk and "chunk %d" % chunk in str(e)
        assert bn.index_file_info(write(tmp_path, bytes(t)))["rows"] == rows  # the header and the size are intact
    t = bytearray(data)
    t[64 + 8 * 3] ^= 1  # the table entry of chunk 3
    assert refused(bn, lambda: bn.index_file_verify(write(tmp_path, bytes(t)))).first_bad_chunk == 3


def test_verify_carries_rows_and_chunks_across_its_read_buffer(bn, tmp_path):
    """the verifier reads 2^18 elements at a time: 2100 x 130 = 273 000 elements cross that once, inside row 2016 (2^18 = 2016 * 130
    + 64) and inside chunk 2 of 1000 rows; 9 x 70 001 crosses it twice inside rows of more than a buffer"""
    rows, dim, cr = 2100, 130, 1000
    assert (1 << 18) // dim == 2016 and (1 << 18) % dim == 64
    x = stored_rows(rows, dim)
    x[2016] = 0
    x[2016, 100] = 0.25  # the row's only non-zero lies behind the boundary: its validity is carried over
    x[2015] = 0
    good = fr.file_bytes(x, cr)
    p = write(tmp_path, good)
    bn.index_file_verify(p)
    assert bn.index_file_info(p)["valid_rows"] == int(fr.valid_mask(x).sum()) == rows - 3
    payload = 64 + 8 * 3
    for row, col in ((2016, 10), (2016, 100), (2017, 0), (2099, 129)):
        t = bytearray(good)
        t[payload + 4 * (row * dim + col) + 2] ^= 0x20
        assert refused(bn, lambda: bn.index_file_verify(write(tmp_path, bytes(t)))).first_bad_chunk == 2
    y = x.copy()
    y[2016, 129] = np.inf
    e = refused(bn, lambda: bn.index_file_verify(write(tmp_path, fr.file_bytes(y, cr))))
    assert "non-finite" in str(e) and e.first_bad_chunk == 2
    wide = stored_rows(9, 70001)
    for cr in (1, 4):
        p = write(tmp_path, fr.file_bytes(wide, cr))
        bn.index_file_verify(p)
        t = bytearray(fr.file_bytes(wide, cr))
        t[64 + 8 * -(-9 // cr) + 4 * (7 * 70001 + 70000)] ^= 1
        assert refused(bn, lambda: bn.index_file_verify(write(tmp_path, bytes(t)))).first_bad_chunk == 7 // cr


def _good():
    return stored_rows(65, 3), 7


def test_refuses_wrong_magic(bn, tmp_path):
    x, cr = _good()
    data = fr.file_bytes(x, cr)
    body = data[64:]
    bad = fr.header(3, 65, cr, 10, int(fr.valid_mask(x).sum()), magic=b"BNINDEX2") + body  # its digest is right: the magic alone is wrong
    p = write(tmp_path, bad)
    assert "magic" in str(refused(bn, lambda: bn.index_file_info(p)))
    refused(bn, lambda: bn.index_file_verify(p))


def test_refuses_wrong_version(bn, tmp_path):
    x, cr = _good()
    bad = fr.header(3, 65, cr, 10, int(fr.valid_mask(x).sum()), version=2) + fr.file_bytes(x, cr)[64:]
    p = write(tmp_path, bad)
    assert "version" in str(refused(bn, lambda: bn.index_file_info(p)))
    refused(bn, lambda: bn.index_file_verify(p))


@pytest.mark.parametrize("pos", [12, 16, 24, 28, 32, 45, 56, 63])
def test_refuses_a_flipped_header_byte(bn, tmp_path, pos):
    x, cr = _good()
    t = bytearray(fr.file_bytes(x, cr))
    t[pos] ^= 1
    p = write(tmp_path, bytes(t))
    assert "header digest" in str(refused(bn, lambda: bn.index_file_info(p)))
    refused(bn, lambda: bn.index_file_verify(p))


def test_refuses_header_fields_outside_the_limits(bn, tmp_path):
    """headers whose digest is right and whose fields are not"""
    for dim, rows, cr, nc in ((0, 0, 1, 0), ((1 << 20) + 1, 0, 1, 0), (3, 0, 0, 0), (3, 5, 2, 2), (3, 0xFFFFFFFF - 64, 1 << 31, 2)):
        p = write(tmp_path, fr.header(dim, rows, cr, nc, 0))
        refused(bn, lambda: bn.index_file_info(p))
        refused(bn, lambda: bn.index_file_verify(p))


def test_refuses_one_byte_truncated(bn, tmp_path):
    x, cr = _good()
    p = write(tmp_path, fr.file_bytes(x, cr)[:-1])
    assert "truncated" in str(refused(bn, lambda: bn.index_file_info(p)))
    refused(bn, lambda: bn.index_file_verify(p))


def test_refuses_one_trailing_byte(bn, tmp_path):
    x, cr = _good()
    p = write(tmp_path, fr.file_bytes(x, cr) + b"\0")
    assert "trailing" in str(refused(bn, lambda: bn.index_file_info(p)))
    refused(bn, lambda: bn.index_file_verify(p))


def test_refuses_a_nan_element(bn, tmp_path):
    """a NaN (and an Inf) under digests recomputed for it: only the finite rule can refuse the file"""
    x, cr = _good()
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[30, 2] = v
        p = write(tmp_path, fr.file_bytes(y, cr))
        assert bn.index_file_info(p)["rows"] == 65   # info reads the header and the size only
        e = refused(bn, lambda: bn.index_file_verify(p))
        assert "non-finite" in str(e) and e.first_bad_chunk == 30 // cr


def test_refuses_a_wrong_valid_rows(bn, tmp_path):
    x, cr = _good()
    nv = int(fr.valid_mask(x).sum())
    for wrong in (nv - 1, nv + 1):
        p = write(tmp_path, fr.file_bytes(x, cr, valid_rows=wrong))
        assert bn.index_file_info(p)["valid_rows"] == wrong
        assert "valid rows" in str(refused(bn, lambda: bn.index_file_verify(p)))


def test_refuses_an_unreadable_path_and_null_arguments(bn, tmp_path):
    missing = str(tmp_path / "nothing_here.bnindex")
    refused(bn, lambda: bn.index_file_info(missing))
    refused(bn, lambda: bn.index_file_verify(missing))
    refused(bn, lambda: bn.index_file_info(str(tmp_path)))  # a directory
    info = bn.BnIndexFileInfo()
    assert bn.lib.bn_index_file_info(None, C.byref(info), C.sizeof(info)) == INVALID_ARG
    assert bn.lib.bn_index_file_info(missing.encode(), None, C.sizeof(info)) == INVALID_ARG
    p = write(tmp_path, fr.file_bytes(*_good()))
    assert bn.lib.bn_index_file_info(p.encode(), C.byref(info), C.sizeof(info) - 1) == INVALID_ARG
    assert bn.lib.bn_index_file_verify(None, None) == INVALID_ARG
    assert bn.lib.bn_index_file_verify(p.encode(), None) == 0  # first_bad_chunk may be NULL
    h = C.c_void_p(0x1234)
    assert bn.lib.bn_index_load(0, None, 0, C.byref(h)) == INVALID_ARG and h.value is None
    assert bn.lib.bn_index_load(0, p.encode(), 0, None) == INVALID_ARG
    assert bn.lib.bn_index_save(None, p.encode(), 0) == INVALID_ARG


def test_sanitizer_program_over_the_reader(tmp_path):
    """tools/asan_index_file.cpp: the host file code alone under ASan + UBSan (leaks included), as a child process"""
    out = tmp_path / "asan_index_file"
    src = os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + src, os.path.join(ROOT, "tools", "asan_index_file.cpp"), os.path.join(src, "index_file.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the index file reader failed:\n" + r.stderr[-3000:])
    good = tmp_path / "good.bnindex"
    good.write_bytes(fr.file_bytes(stored_rows(5, 3), 2))  # 64 + 24 + 60 bytes
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([str(out), str(good), str(work)], capture_output=True, text=True, timeout=300)
    if "LeakSanitizer has encountered a fatal error" in r.stderr:
        # LeakSanitizer stops the world through ptrace, which some containers forbid: it then aborts at exit whatever the program did.
        # Only in that case the run is repeated without the leak check; address and undefined-behaviour checks stay on
        r = subprocess.run([str(out), str(good), str(work)], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "148 truncations, 1 extension, 296 flipped bytes: 0 accepted or misreported" in r.stdout, r.stdout


def test_load_without_a_device_is_refused_loudly(bn, tmp_path):
    if bn.device_count() > 0:
        pytest.skip("a gfx950 device is present")
    p = write(tmp_path, fr.file_bytes(*_good()))
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(p)
    assert e.value.status == NO_DEVICE
    # the host-side checks come first: a malformed file is a malformed file on every machine
    bad = write(tmp_path, fr.file_bytes(*_good())[:-1], "bad.bnindex")
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(bad)
    assert e.value.status == MODEL_LOAD
