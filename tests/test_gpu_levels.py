"""bn_recording_levels on the GPU against tests/levels_ref.py.

Shapes: S in {4, 1028, 144000} -- below one wave, one pass of the 1024 accumulators plus 4 samples, and the model's segment (141
terms per accumulator, the last pass partial); step S/2 and 5.5 steps of audio, so that windows 4 and 5 are padded; one
recording of S - 1 samples, shorter than a window.  peak and flags are compared exactly, mean and mean_square within the header's
bounds computed from BN_LEVEL_SUM_DEPTH and within the same bounds at the tree's own depth at that S; the invariance runs are compared byte for byte."""
import ctypes as C

import numpy as np
import pytest

import levels_ref
import pcm_ref

pytestmark = pytest.mark.gpu
SIZES = (4, 1028, 144000)
_CASES = {}


def _case(bn, S):
    """(int16 values, their f32 samples, the I16 mono recording, step, the float64 reference) per S, built once"""
    if S not in _CASES:
        step = S // 2
        n = 5 * step + max(step // 2, 1)
        rng = np.random.RandomState(100 + S % 97)
        v = rng.randint(-32768, 32768, size=n).astype(np.int16)
        v[n // 3] = -32768
        x = pcm_ref.mono(pcm_ref.pack(v, pcm_ref.I16), pcm_ref.I16, 1, 0)
        _CASES[S] = (v, x, bn.Recording(v), step, levels_ref.levels(x, S, step))
    return _CASES[S]


def _check(bn, got, ref, what, S):
    assert got.dtype == bn.LEVEL_DTYPE and len(got) == len(ref["peak"]), what
    assert got["flags"].tolist() == ref["flags"].tolist(), what
    assert got["peak"].tobytes() == ref["peak"].tobytes(), (what, got["peak"], ref["peak"])
    mean_abs, sq_rel = levels_ref.bounds(ref, bn.BN_LEVEL_SUM_DEPTH)
    err_mean = np.abs(got["mean"].astype(np.float64) - ref["mean"])
    err_sq = np.abs(got["mean_square"].astype(np.float64) - ref["mean_square"])
    print(what, "mean err / bound", (err_mean / np.maximum(mean_abs, 1e-300)).max(), "mean_square err / bound",
          (err_sq / np.maximum(sq_rel * ref["mean_square"], 1e-300)).max())
    assert (err_mean <= mean_abs).all(), (what, err_mean, mean_abs)
    assert (err_sq <= sq_rel * ref["mean_square"]).all(), (what, err_sq, sq_rel * ref["mean_square"])
    # the same derivation at the depth the tree has at THIS S (levels_ref.tree_depth): never looser than the header's
    assert levels_ref.tree_depth(S) <= bn.BN_LEVEL_SUM_DEPTH and levels_ref.tree_depth(1 << 20) == bn.BN_LEVEL_SUM_DEPTH
    mean_abs, sq_rel = levels_ref.bounds(ref, levels_ref.tree_depth(S))
    assert (err_mean <= mean_abs).all(), (what, "at the tree's depth", err_mean, mean_abs)
    assert (err_sq <= sq_rel * ref["mean_square"]).all(), (what, "at the tree's depth", err_sq, sq_rel * ref["mean_square"])


@pytest.mark.parametrize("S", SIZES)
def test_levels_against_float64(bn, S):
    v, x, rec, step, ref = _case(bn, S)
    got = rec.levels(S, step)
    assert len(got) == 6 and ref["flags"].tolist() == [0, 0, 0, 0, levels_ref.PADDED, levels_ref.PADDED]
    _check(bn, got, ref, ("i16", S), S)
    # a recording shorter than one window: one padded window, the divisor still S
    short = bn.Recording(v[:S - 1])
    _check(bn, short.levels(S, step), levels_ref.levels(x[:S - 1], S, step), ("short", S), S)
    assert short.levels(S, S).tolist() == short.levels(S, step)[:1].tolist()


@pytest.mark.parametrize("S", SIZES)
def test_a_window_depends_on_its_samples_alone(bn, S):
    v, x, rec, step, ref = _case(bn, S)
    whole = rec.levels(S, step)
    # first_window / count split three ways
    parts = np.concatenate([rec.levels(S, step, 0, 1), rec.levels(S, step, 1, 3), rec.levels(S, step, 4, 2)])
    assert parts.tobytes() == whole.tobytes()
    assert len(rec.levels(S, step, 6, 0)) == 0
    # another step that shares window starts: window k at step S is window 2k at step S / 2
    wide = rec.levels(S, 2 * step)
    assert len(wide) == 3 and wide.tobytes() == whole[::2].tobytes()
    # the same samples as F32 mono, and as the first channel of stereo I24 beside a silent one
    assert bn.Recording(x).levels(S, step).tobytes() == whole.tobytes()
    stereo = np.stack([v.astype(np.int64) * 256, np.zeros(len(v), dtype=np.int64)], axis=1)
    raw = pcm_ref.pack(stereo, pcm_ref.I24)
    assert pcm_ref.mono(raw, pcm_ref.I24, 2, 0).tobytes() == x.tobytes()
    i24 = bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 0)
    assert i24.levels(S, step).tobytes() == whole.tobytes()
    # ... at another length: the recording's end moves, the unpadded windows' bits stay
    longer = bn.Recording(np.concatenate([v, v[:step]]))
    assert longer.levels(S, step, 0, 4).tobytes() == whole[:4].tobytes()


def test_special_inputs(bn):
    S = 1028
    z = bn.Recording(np.zeros(3 * S, dtype=np.int16)).levels(S, S)
    assert z.tobytes() == bytes(3 * 16)
    full = np.zeros(2 * S, dtype=np.int16)
    full[S + 17] = -32768
    lv = bn.Recording(full).levels(S, S)
    assert lv["peak"].tolist() == [0.0, 1.0] and lv["mean_square"][1] == np.float32(1.0) / np.float32(S)
    x = np.random.RandomState(5).uniform(-1, 1, 4 * S).astype(np.float32)
    clean = bn.Recording(x).levels(S, S)
    for bad, at in ((np.nan, S + 3), (np.inf, 2 * S + 1027), (-np.inf, 3 * S)):
        y = x.copy()
        y[at] = bad
        got = bn.Recording(y).levels(S, S)
        k = at // S
        assert got["flags"].tolist() == [levels_ref.NONFINITE if i == k else 0 for i in range(4)], (bad, got)
        assert got["peak"][k] == np.inf and got["mean_square"][k] == np.inf and got["mean"][k] == 0
        keep = [i for i in range(4) if i != k]
        assert got[keep].tobytes() == clean[keep].tobytes()
        ref = levels_ref.levels(y, S, S)
        assert got["peak"].tobytes() == ref["peak"].tobytes() and got["flags"].tolist() == ref["flags"].tolist()


def test_refusals_and_struct_size(bn):
    S = 1028
    v, x, rec, step, ref = _case(bn, S)
    for args, word in (((S + 2, step, 0, 1), "multiple of 4"), ((S, step, 5, 2), "exceeds the 6 windows"), ((S, step, 7, 0), "exceeds the 6 windows"),
                       ((S, 0, 0, 1), "step_samples")):
        with pytest.raises(bn.EngineError) as e:
            rec.levels(*args)
        assert e.value.status == 1 and word in bn.last_error(), (args, bn.last_error())
    out = (bn.BnWindowLevel * 2)()
    assert bn.lib.bn_recording_levels(rec._h, S, step, 0, 2, out, C.sizeof(bn.BnWindowLevel) - 1) == 1 and "struct_size" in bn.last_error()
    assert bn.lib.bn_recording_levels(rec._h, S, step, 0, 2, None, C.sizeof(bn.BnWindowLevel)) == 1 and "null" in bn.last_error()
    # a caller compiled against a longer struct: its stride is kept, the bytes behind this header's fields are left alone
    wide = np.full(2 * 6, 0xA5A5A5A5, dtype=np.uint32)
    assert bn.lib.bn_recording_levels(rec._h, S, step, 1, 2, wide.ctypes.data_as(C.POINTER(bn.BnWindowLevel)), 24) == 0
    rows = wide.reshape(2, 6)
    assert rows[:, :4].tobytes() == rec.levels(S, step, 1, 2).tobytes() and (rows[:, 4:] == 0xA5A5A5A5).all()


def test_asynchronous_upload_gives_the_same_bits(bn):
    S = 144000
    v, x, rec, step, ref = _case(bn, S)
    a = bn.Recording(v, async_upload=True)
    assert a.levels(S, step).tobytes() == rec.levels(S, step).tobytes()
    a.wait()


def test_a_second_piece_continues_the_first(bn):
    """A call runs at most 2^20 windows per launch: 2^20 + 3 windows of S = 4 at step 1 take two.  The rows either side of the cut
    are those of a call on just that range (one piece), byte for byte, and the float64 reference's; a caller's longer struct keeps its
    stride across the cut."""
    S, piece = 4, 1 << 20
    count = piece + 3
    v = np.random.RandomState(2020).randint(-32768, 32768, size=count).astype(np.int16)
    rec = bn.Recording(v)
    assert rec.n_windows(1) == count
    whole = rec.levels(S, 1)
    first, n = piece - 2, 5
    edge = rec.levels(S, 1, first, n)
    assert len(whole) == count and whole[first:].tobytes() == edge.tobytes()
    x = pcm_ref.mono(pcm_ref.pack(v[first:], pcm_ref.I16), pcm_ref.I16, 1, 0)  # the samples these windows read: the last 5
    ref = levels_ref.levels(x, S, 1)
    assert ref["flags"].tolist() == [0, 0, levels_ref.PADDED, levels_ref.PADDED, levels_ref.PADDED]
    _check(bn, whole[first:], ref, "across the piece boundary", S)
    wide = np.full((count, 6), 0xA5A5A5A5, dtype=np.uint32)
    assert bn.lib.bn_recording_levels(rec._h, S, 1, 0, count, wide.ctypes.data_as(C.POINTER(bn.BnWindowLevel)), C.sizeof(bn.BnWindowLevel) + 8) == 0
    assert np.ascontiguousarray(wide[:, :4]).tobytes() == whole.tobytes() and (wide[:, 4:] == 0xA5A5A5A5).all()
