"""bn_index_save / bn_index_load on the device: the file is the numpy reference writer's file of the stored rows, byte for byte; the
device digests are the host verifier's; a loaded index returns the original's bytes from every consumer of the slab (read, search,
search by id, clustering, an IVF view), takes further appends, and exists only if the file is whole.  Every comparison is == on bytes."""
import importlib
import os

import numpy as np
import pytest

import index_file_ref as fr
from gpu_helpers import write_model

pytestmark = pytest.mark.gpu
synth = importlib.import_module("rust-birdnet-onnx_amd.synth")

DIMS = [3, 128, 130]
ROWS = [0, 1, 63, 64, 65, 1000]
CHUNKS = [1, 7, 64, 1000, 5000, 0]  # 0: the default; 1000 rows at 7 are 143 chunks
_cases = {}


def source_rows(rows, dim):
    """random rows with an all-zero row, a row holding NaN, a row holding Inf (all three stored as zeros) and a row with negative zeros"""
    rng = np.random.default_rng(1000 * rows + dim)
    x = rng.standard_normal((rows, dim)).astype(np.float32)
    special = {}
    if rows >= 63:
        special = {"zero": rows // 2, "nan": rows // 3, "inf": rows - 1, "negzero": 1}
        x[special["zero"]] = 0
        x[special["nan"], dim // 2] = np.nan
        x[special["inf"], 0] = np.inf
        x[special["negzero"], ::2] = -0.0
    return x, special


def build(bn, x, capacity=None):
    """x appended by add_host calls of uneven sizes"""
    rows, dim = x.shape
    idx = bn.Index(0, dim, capacity or max(rows, 1))
    cuts = sorted({0, min(rows, 1), min(rows, 6), rows // 3, rows - rows // 5, rows})
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert idx.add(x[a:b]) == a
    assert len(idx) == rows
    return idx


def case(bn, rows, dim):
    """(source rows, special rows, the index, its stored rows): built once per shape, never changed by a test"""
    if (rows, dim) not in _cases:
        x, special = source_rows(rows, dim)
        idx = build(bn, x)
        _cases[(rows, dim)] = (x, special, idx, idx.read())
    return _cases[(rows, dim)]


def same(a, b):
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_saved_file_is_the_reference_writers_file(bn, tmp_path, rows, dim):
    x, special, idx, stored = case(bn, rows, dim)
    invalid = sorted(special[k] for k in ("zero", "nan", "inf")) if special else []
    assert [int(i) for i in np.flatnonzero(~fr.valid_mask(stored))] == invalid
    if special:
        neg = stored[special["negzero"], ::2].view(np.uint32)
        assert (neg == 0x80000000).all()  # the stored bits hold negative zeros
    for cr in CHUNKS:
        p = str(tmp_path / ("c%d.bnindex" % cr))
        idx.save(p, cr)
        got = open(p, "rb").read()
        want = fr.file_bytes(stored, cr)
        assert got == want, (rows, dim, cr, len(got), len(want))
        bn.index_file_verify(p)  # the CPU's digests: an implementation that shares only the digest function with the kernels
        info = bn.index_file_info(p)
        assert info == {"dim": dim, "rows": rows, "valid_rows": rows - len(invalid), "chunk_rows": cr or fr.default_chunk_rows(dim),
                        "n_chunks": -(-rows // (cr or fr.default_chunk_rows(dim))), "version": 1}
    assert sorted(os.listdir(tmp_path)) == sorted("c%d.bnindex" % cr for cr in CHUNKS)  # no temporary left
    assert idx.read().tobytes() == stored.tobytes() and len(idx) == rows


# A launch of the kernels covers a slice: the rows that fit one 8 MB staging block (16131 rows at dim 130, 1365 at dim 1536), and two
# device blocks and two pinned blocks rotate.  These shapes are about 36 MB: four full slices and a short fifth, so every block is
# reused, later slices start at row0 != 0, and chunks straddle slice boundaries (chunk_rows that do not divide a slice) or span
# several slices (chunk_rows above a slice).  The host verifier's 2^18-element read buffer is crossed some thirty times as well.
BIG = [(70000, 130, (1000, 20000)), (6000, 1536, (1000, 2000))]


@pytest.mark.parametrize("rows,dim,chunks", BIG, ids=["70000x130", "6000x1536"])
def test_many_slices_save_verify_load_and_a_late_flipped_bit(bn, tmp_path, rows, dim, chunks):
    slice_rows = (8 << 20) // (4 * dim)
    assert rows > 4 * slice_rows and rows % slice_rows and all(slice_rows % c and c % slice_rows for c in chunks) and max(chunks) > slice_rows
    rng = np.random.default_rng(rows + dim)
    x = rng.standard_normal((rows, dim), dtype=np.float32)
    invalid = [slice_rows - 1, slice_rows, 3 * slice_rows + 7, rows - 1]  # either side of a slice boundary, a late slice, the last row
    x[invalid[0]] = 0
    x[invalid[1], 5] = np.nan
    x[invalid[2], dim - 1] = np.inf
    x[invalid[3]] = 0
    idx = bn.Index(0, dim, rows)
    for a in range(0, rows, 9973):
        assert idx.add(x[a:a + 9973]) == a
    stored = idx.read()
    assert [int(i) for i in np.flatnonzero(~fr.valid_mask(stored))] == invalid
    p = str(tmp_path / "big.bnindex")
    for cr in chunks:
        idx.save(p, cr)
        data = open(p, "rb").read()
        assert data == fr.file_bytes(stored, cr), (rows, dim, cr)
        bn.index_file_verify(p)
        assert bn.index_file_info(p)["valid_rows"] == rows - 4
        got = bn.Index.load(p)
        assert len(got) == rows and got.read().tobytes() == stored.tobytes()
        q = x[[2, 4 * slice_rows + 11, rows - 2]] + np.float32(0.01)
        a, b = idx.search(q, 10), got.search(q, 10)
        assert same(a, b) and not set(b[0].reshape(-1).tolist()) & set(invalid)
        assert [int(i) for i in b[0][:, 0]] == [2, 4 * slice_rows + 11, rows - 2]  # rows of three different slices, each at its own id
        del got
    # one bit in the short last slice, and one in the fourth: load and the host verifier name the chunk, no index comes back
    cr = chunks[-1]  # the file `data` holds
    payload = 64 + 8 * -(-rows // cr)
    bad = str(tmp_path / "bad.bnindex")
    for row in (rows - 3, 3 * slice_rows + 100):
        t = bytearray(data)
        t[payload + 4 * (row * dim + 1)] ^= 0x01
        open(bad, "wb").write(bytes(t))
        with pytest.raises(bn.EngineError) as e:
            bn.Index.load(bad)
        assert e.value.status == 6 and "chunk %d of" % (row // cr) in str(e.value)
        with pytest.raises(bn.EngineError) as e:
            bn.index_file_verify(bad)
        assert e.value.first_bad_chunk == row // cr
    assert len(bn.Index.load(p)) == rows


def test_two_saves_are_identical_and_a_save_replaces_an_existing_file(bn, tmp_path):
    _, _, idx, stored = case(bn, 1000, 130)
    _, _, other, other_stored = case(bn, 65, 130)
    a, b = str(tmp_path / "a.bnindex"), str(tmp_path / "b.bnindex")
    idx.save(a, 7)
    idx.save(b, 7)
    assert open(a, "rb").read() == open(b, "rb").read()
    other.save(a, 7)  # over the larger file
    assert open(a, "rb").read() == fr.file_bytes(other_stored, 7)
    assert sorted(os.listdir(tmp_path)) == ["a.bnindex", "b.bnindex"]


def test_save_into_a_missing_directory_fails_and_leaves_nothing(bn, tmp_path):
    _, _, idx, stored = case(bn, 65, 3)
    with pytest.raises(bn.EngineError) as e:
        idx.save(str(tmp_path / "no_such_dir" / "x.bnindex"))
    assert e.value.status == 1 and "cannot create" in str(e.value)
    assert os.listdir(tmp_path) == []
    keep = tmp_path / "keep.bnindex"
    keep.write_bytes(b"an older file")
    with pytest.raises(bn.EngineError) as e:
        idx.save(str(keep), 1 << 32)  # refused before anything is written
    assert e.value.status == 1 and keep.read_bytes() == b"an older file" and os.listdir(tmp_path) == ["keep.bnindex"]
    assert idx.read().tobytes() == stored.tobytes()


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rows", ROWS)
def test_loaded_index_answers_as_the_saved_one(bn, tmp_path, rows, dim):
    x, special, idx, stored = case(bn, rows, dim)
    p = str(tmp_path / "x.bnindex")
    idx.save(p, 7)
    got = bn.Index.load(p)
    assert len(got) == rows and got.dim == dim and got.read().tobytes() == stored.tobytes()
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    if rows:
        q[1] = x[rows - 1 if not special else 2] + 0.1 * q[1]
    a, b = idx.search(q, 10), got.search(q, 10)
    assert same(a, b)
    invalid = [special[k] for k in ("zero", "nan", "inf")] if special else []
    assert (b[2] == min(10, rows - len(invalid))).all()
    for i in range(3):
        assert not set(b[0][i, :b[2][i]].tolist()) & set(invalid)
    if rows:
        ids = np.array(sorted({0, rows // 2, rows - 1} | set(invalid)), dtype=np.uint64)
        a, b = idx.search_ids(ids, 10, exclude_radius=2), got.search_ids(ids, 10, exclude_radius=2)
        assert same(a, b)
        for i, qid in enumerate(ids.tolist()):
            hits = set(b[0][i, :b[2][i]].tolist())
            assert not hits & set(invalid) and not hits & set(range(qid - 2, qid + 3))
            assert b[2][i] == 0 if qid in invalid else b[2][i] > 0 or rows <= 5
    # M beyond the valid rows: every valid row comes back, and only those
    full = got.search(q[:1], 256)
    if rows <= 256:
        assert sorted(full[0][0, :full[2][0]].tolist()) == [r for r in range(rows) if r not in invalid]


def test_load_with_spare_capacity_takes_further_appends(bn, tmp_path):
    x, special, idx, stored = case(bn, 65, 130)
    p = str(tmp_path / "x.bnindex")
    idx.save(p)
    got = bn.Index.load(p, capacity_rows=65 + 100)
    extra = np.random.default_rng(9).standard_normal((100, 130)).astype(np.float32)
    extra[50] = 0
    grown = build(bn, x, capacity=165)  # the same appends without the file
    assert got.add(extra[:37]) == 65 and grown.add(extra[:37]) == 65
    assert got.add(extra[37:]) == 102 and grown.add(extra[37:]) == 102
    assert len(got) == 165 and got.read().tobytes() == grown.read().tobytes()
    q = extra[[3, 60]] + np.float32(0.05)
    assert same(got.search(q, 20), grown.search(q, 20))
    with pytest.raises(bn.EngineError) as e:
        got.add(extra[:1])  # full, as the index it mirrors
    assert e.value.status == 1
    # and the grown index saves and loads again
    p2 = str(tmp_path / "y.bnindex")
    got.save(p2, 64)
    assert open(p2, "rb").read() == fr.file_bytes(grown.read(), 64)


def test_load_refuses_a_capacity_below_the_files_rows(bn, tmp_path):
    _, _, idx, _ = case(bn, 65, 3)
    p = str(tmp_path / "x.bnindex")
    idx.save(p)
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(p, capacity_rows=64)
    assert e.value.status == 1 and "capacity_rows" in str(e.value)
    assert len(bn.Index.load(p, capacity_rows=65)) == 65


@pytest.mark.parametrize("dim", [128, 130])
def test_clustering_and_ivf_on_a_loaded_index(bn, tmp_path, dim):
    """the valid bytes and the pad columns, through the consumers that read them: assignment, k-means, an IVF view"""
    x, special, idx, stored = case(bn, 1000, dim)
    p = str(tmp_path / "x.bnindex")
    idx.save(p, 64)
    got = bn.Index.load(p)
    init = np.array([5, 200, 401, 777, 900, 64], dtype=np.uint64)
    a = idx.cluster(6, max_iters=4, init_ids=init)
    b = got.cluster(6, max_iters=4, init_ids=init)
    assert same(a[:4], b[:4]) and a[4]["iters"] == b[4]["iters"] and a[4]["objective"] == b[4]["objective"]
    invalid = [special[k] for k in ("zero", "nan", "inf")]
    assert (b[1][invalid] == bn.BN_CLUSTER_NONE).all() and (np.delete(b[1], invalid) != bn.BN_CLUSTER_NONE).all()
    va, vb = bn.Ivf(idx, a[0]), bn.Ivf(got, b[0])
    assert va.list_sizes().tobytes() == vb.list_sizes().tobytes() and int(vb.list_sizes().sum()) == 1000 - 3
    q = x[[10, 500, 998]] + np.float32(0.02)
    assert same(va.search(q, 2, 10), vb.search(q, 2, 10))
    ids = np.array([0, 333, 999 - 1], dtype=np.uint64)
    assert same(va.search_ids(ids, 3, 10, exclude_radius=1), vb.search_ids(ids, 3, 10, exclude_radius=1))


def test_save_straight_after_add_ctx_contains_those_rows(bn, tmp_path):
    m = bn.Model(write_model(synth.perch_v2(num_species=700, width=0.35, depth=0.25, emb=192)))
    cfg = m.config
    S = int(cfg.sample_count)
    pcm = np.clip(synth.synthetic_segments(1, 4 * S, int(cfg.sample_rate))[0], -1, 1).astype(np.float32)
    rec = bn.Recording(pcm)
    ctx = bn.Context(m, 3)
    idx = bn.Index(0, int(cfg.embedding_dim), 8)
    _, emb = ctx.infer_windows(rec, S, 0, 3)
    assert idx.add_context(ctx, 3) == 0
    p = str(tmp_path / "x.bnindex")
    idx.save(p, 2)  # the append is still pending on the context's stream: the save waits for it as a search does
    stored = idx.read()
    assert fr.valid_mask(stored).all() and np.abs(np.sqrt((stored.astype(np.float64) ** 2).sum(axis=1)) - 1).max() < 1e-6
    assert open(p, "rb").read() == fr.file_bytes(stored, 2)
    got = bn.Index.load(p)
    assert got.read().tobytes() == stored.tobytes() and same(got.search(emb, 3), idx.search(emb, 3))


def test_load_refuses_a_damaged_file_and_then_loads_the_good_one(bn, tmp_path):
    _, _, idx, stored = case(bn, 1000, 130)
    good = str(tmp_path / "good.bnindex")
    idx.save(good, 64)  # 16 chunks; the last one holds rows 960..999
    data = bytearray(open(good, "rb").read())
    flipped = bytearray(data)
    flipped[len(data) - 4 * 130 * 20 + 2] ^= 0x04  # one bit of row 980
    bad = str(tmp_path / "bad.bnindex")
    open(bad, "wb").write(bytes(flipped))
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(bad)
    assert e.value.status == 6 and "chunk 15 of 16" in str(e.value)
    h = bn.C.c_void_p(0x1234)
    assert bn.lib.bn_index_load(0, bad.encode(), 0, bn.C.byref(h)) == 6 and h.value is None  # no index comes back
    with pytest.raises(bn.EngineError) as e:
        bn.index_file_verify(bad)
    assert e.value.first_bad_chunk == 15
    y = stored.copy()
    y[130, 7] = np.nan
    open(bad, "wb").write(fr.file_bytes(y, 64))  # a NaN under digests recomputed for it
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(bad)
    assert e.value.status == 6 and "non-finite element in chunk 2" in str(e.value)
    open(bad, "wb").write(fr.file_bytes(stored, 64, valid_rows=996))
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(bad)
    assert e.value.status == 6 and "valid rows" in str(e.value)
    open(bad, "wb").write(bytes(data[:-1]))
    with pytest.raises(bn.EngineError) as e:
        bn.Index.load(bad)
    assert e.value.status == 6 and "truncated" in str(e.value)
    got = bn.Index.load(good)
    assert len(got) == 1000 and got.read().tobytes() == stored.tobytes()
