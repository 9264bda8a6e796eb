"""Spectrograms without a GPU: the two host-only designers (bn_mel_filterbank, bn_spectrogram_thresholds) against their restatement
(tests/spectrogram_ref.py) and the refusals of the three host-only entry points, through the library; the host arithmetic of
csrc/spectrogram_plan.h under ASan / UBSan (tools/asan_spectrogram_plan.cpp); and the reference itself on the GPU test's own random
inputs: four wrong rules leave the header's bounds.

The tests that take the `bn` fixture and the sanitizer build fail where the library lacks the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pcm_ref
import spectrogram_ref as ref


@pytest.mark.parametrize("rate,N,n_mels,fmin,fmax", [(48000, 1024, 64, 0.0, 24000.0), (48000, 2048, 128, 50.0, 15000.0), (32000, 256, 20, 300.0, 16000.0)])
def test_mel_designer_against_the_restatement(bn, rate, N, n_mels, fmin, fmax):
    W, want = bn.mel_filterbank(rate, N, n_mels, fmin, fmax), ref.mel_bank(rate, N, n_mels, fmin, fmax)
    assert W.shape == want.shape and W.dtype == np.float32 and (W >= 0).all() and (W.max(axis=1) > 0).all()
    # double on both sides, rounded once: half an f32 ulp of the weight, and the library's log10 / pow against numpy's
    assert (np.abs(W - want) <= 2.0 ** -24 * want + 1e-12).all()
    assert ((W > 0) == (want.astype(np.float32) > 0)).all()


@pytest.mark.parametrize("ref_power,range_db", [(1.0, 80.0), (3.7e-3, 96.5), (1e30, 1.0)])
def test_threshold_table_against_the_restatement(bn, ref_power, range_db):
    thr, want = bn.spectrogram_thresholds(ref_power, range_db), ref.thresholds(ref_power, range_db)
    assert thr.shape == (255,) and (np.diff(thr) >= 0).all()
    assert (np.abs(thr.astype(np.float64) - want) <= 2.0 ** -23 * want).all()  # pow against numpy's: one f32 ulp
    top = float(np.float32(ref_power))
    assert thr[-1] < top and ref.codes(thr, np.float32([top, top * 10 ** (-range_db / 10), 0.0])).tolist() == [255, 0, 0]


def test_refusals_of_the_host_only_entry_points(bn):
    L, err = bn.lib, bn.last_error
    w, thr, f = (C.c_float * (256 * 1025))(), (C.c_float * 255)(), C.c_float
    for i in range(len(w)):
        w[i] = -7.0  # poison
    nan, inf = float("nan"), float("inf")
    for args, word in (((0, 1024, 8, 0.0, 8000.0, w), "sample_rate"), ((48000, 1000, 8, 0.0, 8000.0, w), "frame"), ((48000, 1024, 0, 0.0, 8000.0, w), "n_mels"),
                       ((48000, 1024, 257, 0.0, 8000.0, w), "n_mels"), ((48000, 1024, 8, -1.0, 8000.0, w), "fmin_hz"), ((48000, 1024, 8, 8000.0, 8000.0, w), "below fmax_hz"),
                       ((48000, 1024, 8, 0.0, 24000.5, w), "half the sample rate"), ((48000, 1024, 8, nan, 8000.0, w), "fmin_hz"),
                       ((48000, 1024, 8, 0.0, nan, w), "fmax_hz"), ((48000, 1024, 8, 0.0, 8000.0, None), "null"),
                       ((48000, 256, 128, 0.0, 24000.0, w), "triangle 0 holds no bin centre")):
        assert L.bn_mel_filterbank(*args) == 1 and word in err(), (args, err())
    assert set(w) == {-7.0}  # nothing written, the refusal of a late triangle included
    for args, word in (((f(0.0), f(80.0), thr), "ref_power"), ((f(-1.0), f(80.0), thr), "ref_power"), ((f(inf), f(80.0), thr), "ref_power"),
                       ((f(nan), f(80.0), thr), "ref_power"), ((f(1.0), f(0.0), thr), "range_db"), ((f(1.0), f(inf), thr), "range_db"),
                       ((f(1.0), f(nan), thr), "range_db"), ((f(1.0), f(80.0), None), "null")):
        assert L.bn_spectrogram_thresholds(*args) == 1 and word in err(), (args, err())
    assert set(thr) == {0.0}
    h, good = C.c_void_p(), np.ones((2, 129), dtype=np.float32)
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for bad, word in ((-1.0, "negative or not finite"), (nan, "negative or not finite"), (inf, "negative or not finite")):
        Wb = good.copy()
        Wb[1, 128] = bad
        assert L.bn_filterbank_create(0, 256, 2, p(Wb), C.byref(h)) == 1 and word in err() and not h.value, err()
    Wz = good.copy()
    Wz[1] = 0.0
    for args, word in (((0, 256, 2, p(Wz), C.byref(h)), "row 1 of the filter bank is all zeros"), ((0, 256, 0, p(good), C.byref(h)), "n_rows"),
                       ((0, 256, 257, p(good), C.byref(h)), "n_rows"), ((0, 300, 2, p(good), C.byref(h)), "frame"), ((0, 256, 2, None, C.byref(h)), "null"),
                       ((0, 256, 2, p(good), None), "null")):
        assert L.bn_filterbank_create(*args) == 1 and word in err() and not h.value, (word, err())
    assert L.bn_filterbank_rows(None) == 0 and L.bn_filterbank_frame(None) == 0
    c = ref.header_constants()
    assert (c["BN_SPECTROGRAM_F32"], c["BN_SPECTROGRAM_U8"], c["BN_FILTERBANK_MAX_ROWS"], c["BN_SPECTROGRAM_POW_DEPTH"], c["BN_SPECTROGRAM_BANK_DEPTH"]) == \
        (bn.BN_SPECTROGRAM_F32, bn.BN_SPECTROGRAM_U8, bn.BN_FILTERBANK_MAX_ROWS, bn.BN_SPECTROGRAM_POW_DEPTH, bn.BN_SPECTROGRAM_BANK_DEPTH)
    assert C.sizeof(bn.BnSpectrogramSpec) == 28 and L.bn_abi_version() == 2


def test_plan_under_asan_ubsan(tmp_path):
    out = tmp_path / "asan_spectrogram_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ref.ROOT, "include"), "-I" + os.path.join(ref.ROOT, "rust-birdnet-onnx_amd", "csrc"),
           os.path.join(ref.ROOT, "tools", "asan_spectrogram_plan.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "0 failures" in r.stdout and "asan_spectrogram_plan: ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


@pytest.mark.parametrize("N", ref.FRAMES)
def test_bounds_reject_wrong_rules(N):
    """on the GPU test's inputs: a Hann window that is not periodic, a missing c_k, the bank on amplitudes, a bank row shifted by a bin"""
    n_frames, hop = 17, N // 2
    x = pcm_ref.mono(pcm_ref.pack(ref.noise(N, n_frames, hop), pcm_ref.I16), pcm_ref.I16, 1, 0)
    for kind in ({"bins": (0, N // 2 + 1)}, {"bank": ref.mel_bank(48000, N, 16, 0.0, 24000.0).astype(np.float32)}, {"bank": ref.random_bank(N, 17)}):
        want, bound = ref.image(x, 0, n_frames, N, hop, **kind)
        assert ref.worst_share(want, want, bound) == 0.0 and ref.worst_share(want.astype(np.float32), want, bound) < 0.1
        for wrong in ref.WRONG[:2] if "bins" in kind else ref.WRONG:
            assert ref.worst_share(ref.image(x, 0, n_frames, N, hop, wrong=wrong, **kind)[0], want, bound) > 1.0, (N, wrong, list(kind))
