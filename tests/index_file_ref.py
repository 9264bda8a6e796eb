"""The index file format (include/birdnet_hip.h, bn_index_save) in numpy: a writer, a reader and the digest, written from the
format table of the header and from nothing else.  All digest arithmetic is uint64 and wraps mod 2^64.

    bytes 0..8 magic "BNINDEX1" | 8..12 u32 version = 1 | 12..16 u32 dim | 16..24 u64 rows | 24..28 u32 chunk_rows | 28..32 u32 n_chunks
    32..40 u64 valid_rows | 40..56 zero | 56..64 u64 header digest | n_chunks x u64 chunk digests | rows x dim f32, stride dim
"""
import struct

import numpy as np

MAGIC = b"BNINDEX1"
_C1, _C2, _C3 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def terms(u, b):
    """the digest term of every (u, b): u uint64 positions, b uint32 values"""
    with np.errstate(over="ignore"):
        z = np.asarray(u, dtype=np.uint64) * _C1 + np.asarray(b, dtype=np.uint32).astype(np.uint64)
        z = (z ^ (z >> np.uint64(30))) * _C2
        z = (z ^ (z >> np.uint64(27))) * _C3
        return z ^ (z >> np.uint64(31))


def digest(u, b):
    with np.errstate(over="ignore"):
        return int(np.add.reduce(terms(u, b), dtype=np.uint64)) if len(np.atleast_1d(b)) else 0


def default_chunk_rows(dim):
    return max(1, (1 << 21) // dim)


def chunk_digests(rows, chunk_rows):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    bits = rows.view(np.uint32).reshape(-1)
    out = []
    for r0 in range(0, n, chunk_rows):
        r1 = min(n, r0 + chunk_rows)
        out.append(digest(np.arange(r0 * dim, r1 * dim, dtype=np.uint64), bits[r0 * dim:r1 * dim]))
    return out


def valid_mask(rows):
    """a row is invalid exactly when every element is +0.0 or -0.0"""
    bits = np.ascontiguousarray(rows, dtype=np.float32).view(np.uint32)
    return ((bits & np.uint32(0x7FFFFFFF)) != 0).any(axis=1) if bits.size else np.zeros(bits.shape[0], dtype=bool)


def header(dim, rows, chunk_rows, n_chunks, valid_rows, version=1, magic=MAGIC):
    head = magic + struct.pack("<IIQIIQ", version, dim, rows, chunk_rows, n_chunks, valid_rows) + bytes(16)
    assert len(head) == 56
    words = np.frombuffer(head, dtype="<u4")
    return head + struct.pack("<Q", digest(np.arange(14, dtype=np.uint64), words))


def file_bytes(rows, chunk_rows=0, valid_rows=None):
    """the file of stored rows [n, dim] (f32, written as they are)"""
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n, dim = rows.shape
    chunk_rows = chunk_rows or default_chunk_rows(dim)
    table = chunk_digests(rows, chunk_rows)
    assert len(table) == -(-n // chunk_rows)
    nv = int(valid_mask(rows).sum()) if valid_rows is None else valid_rows
    return header(dim, n, chunk_rows, len(table), nv) + struct.pack("<%dQ" % len(table), *table) + rows.astype("<f4").tobytes()


def read(data):
    """(fields, table [n_chunks] uint64, rows [n, dim] f32) of a file's bytes; raises ValueError where the format is broken"""
    if len(data) < 64 or data[:8] != MAGIC:
        raise ValueError("not an index file")
    version, dim, rows, chunk_rows, n_chunks, valid_rows = struct.unpack("<IIQIIQ", data[8:40])
    if version != 1 or dim == 0 or chunk_rows == 0 or n_chunks != -(-rows // chunk_rows) or data[40:56] != bytes(16):
        raise ValueError("bad header fields")
    if struct.unpack("<Q", data[56:64])[0] != digest(np.arange(14, dtype=np.uint64), np.frombuffer(data[:56], dtype="<u4")):
        raise ValueError("header digest")
    if len(data) != 64 + 8 * n_chunks + 4 * rows * dim:
        raise ValueError("size")
    table = np.frombuffer(data, dtype="<u8", count=n_chunks, offset=64)
    payload = np.frombuffer(data, dtype="<f4", count=rows * dim, offset=64 + 8 * n_chunks).reshape(rows, dim)
    if [int(t) for t in table] != chunk_digests(payload, chunk_rows):
        raise ValueError("chunk digest")
    if not np.isfinite(payload).all() or int(valid_mask(payload).sum()) != valid_rows:
        raise ValueError("payload rules")
    fields = {"dim": dim, "rows": rows, "valid_rows": valid_rows, "chunk_rows": chunk_rows, "n_chunks": n_chunks, "version": version}
    return fields, table, payload
