"""tests/pcm_ref.py -- the numpy restatement of the PCM layout rule the GPU tests compare the device with -- against an
independent float64 evaluation written here from the table in include/birdnet_hip.h, and the parts of the feature that need no
device: the header's constants, the refusals that come before any device is touched, and the stand-alone sanitizer program over
pcm_layout.h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcm_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24  # one f32 rounding to nearest: at most this, relative to the value rounded


def exact64(raw, fmt):
    """every stored sample as the real number the table defines, float64 [n]; bytes decoded here, not by pcm_ref"""
    b = bytearray(raw)
    n = len(b) // P.SAMPLE_BYTES[fmt]
    out = np.empty(n, np.float64)
    for i in range(n):
        if fmt == P.I16:
            out[i] = int.from_bytes(b[2 * i:2 * i + 2], "little", signed=True) / 32768.0
        elif fmt == P.I24:
            out[i] = int.from_bytes(b[3 * i:3 * i + 3], "little", signed=True) / 8388608.0
        elif fmt == P.I32:
            out[i] = int.from_bytes(b[4 * i:4 * i + 4], "little", signed=True) / 2147483648.0
        elif fmt == P.U8:
            out[i] = (b[i] - 128) / 128.0
    return out


@pytest.mark.parametrize("fmt", [P.I16, P.I24, P.U8])
@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_select_is_exact_for_i16_i24_u8(fmt, channels):
    rng = np.random.RandomState(fmt * 31 + channels)
    raw = P.test_data(rng, fmt, 257, channels)
    want = exact64(raw, fmt).reshape(-1, channels)
    for ch in range(channels):
        got = P.mono(raw, fmt, channels, ch)
        assert got.dtype == np.float32
        assert np.array_equal(got.astype(np.float64), want[:, ch]), (fmt, channels, ch)


@pytest.mark.parametrize("channels", [1, 2, 3, 16])
def test_i32_select_is_within_one_rounding(channels):
    rng = np.random.RandomState(700 + channels)
    raw = P.test_data(rng, P.I32, 257, channels)
    want = exact64(raw, P.I32).reshape(-1, channels)
    for ch in range(channels):
        got = P.mono(raw, P.I32, channels, ch).astype(np.float64)
        assert np.all(np.abs(got - want[:, ch]) <= U * np.abs(want[:, ch])), (channels, ch)
    # the conversion is the correctly rounded one: 2^31 - 1 rounds up to 1.0, -2^31 is -1.0, 2^24 + 1 rounds to even
    edge = P.pack(np.array([2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3], np.int64), P.I32)
    assert P.mono(edge, P.I32, 1, 0).tolist() == [1.0, -1.0, 2.0 ** -7, (2 ** 24 + 4) * 2.0 ** -31]


@pytest.mark.parametrize("channels", [2, 3, 4, 5, 16])
def test_i32_mix_is_within_channels_minus_one_roundings_of_the_float64_mean(channels):
    """One rounding per add of the rule: each is at most U relative to a partial sum, and no partial sum exceeds sum |s[c]|, so
    after the division by `channels` the adds leave at most (channels - 1) * U * mean |s[c]|.  The mean is taken in float64 over
    the rule's f32 samples -- their own conversion rounding is test_i32_select_is_within_one_rounding's.

    For a power-of-two channel count inv = 1 / channels and the product acc * inv are exact, and (channels - 1) roundings is the
    whole bound.  For any other count the rule itself rounds twice more -- inv once, the product once, each at most U relative to
    the mean -- so the bound that can hold there is (channels - 1) + 2 roundings: measured on this data, 3 channels reach 2.18
    roundings, above the 2 the adds alone explain."""
    rng = np.random.RandomState(900 + channels)
    raw = P.test_data(rng, P.I32, 1003, channels)
    s = P.samples_f32(raw, P.I32).astype(np.float64).reshape(-1, channels)
    want = s.sum(axis=1) / channels
    got = P.mono(raw, P.I32, channels, P.MIX).astype(np.float64)
    unit = U * np.abs(s).sum(axis=1) / channels
    roundings = (channels - 1) + (0 if channels & (channels - 1) == 0 else 2)
    print("channels", channels, "max |mix - mean| in roundings:", float(np.max(np.abs(got - want) / unit)), "allowed", roundings)
    assert np.all(np.abs(got - want) <= roundings * unit), channels


def test_mix_follows_the_stated_order():
    """acc = s[0]; acc += s[c] ascending; * inv rounded once: a case where any other order, a float64 sum or a division gives
    other bits"""
    s = np.array([[1.0, 2.0 ** -24, 2.0 ** -24], [2.0 ** -24, 2.0 ** -24, 1.0]], np.float32)
    raw = P.pack(s, P.F32)
    inv = np.float32(1.0) / np.float32(3.0)
    want = np.array([np.float32(1.0) * inv, np.float32(np.float32(2.0 ** -23) + np.float32(1.0)) * inv], np.float32)
    assert P.mono(raw, P.F32, 3, P.MIX).tobytes() == want.tobytes()
    assert want[0] != want[1]  # the ascending order loses the two small terms in frame 0 only


def test_i24_sign_extension():
    raw = bytes([0xFF, 0xFF, 0x7F, 0x00, 0x00, 0x80, 0xFF, 0xFF, 0xFF])  # 0x7FFFFF, 0x800000, 0xFFFFFF
    assert P.unpack_ints(raw, P.I24).tolist() == [8388607, -8388608, -1]
    assert P.mono(raw, P.I24, 1, 0).tolist() == [8388607 / 8388608, -1.0, -1 / 8388608]
    assert P.pack(np.array([8388607, -8388608, -1]), P.I24) == raw


@pytest.mark.parametrize("op", [0, P.MIX])
def test_one_channel_is_todays_conversion(op):
    rng = np.random.RandomState(5)
    i16 = rng.randint(-32768, 32768, 999).astype(np.int16)
    i16[:3] = [-32768, 32767, 0]
    assert P.mono(i16.tobytes(), P.I16, 1, op).tobytes() == (i16.astype(np.float32) / np.float32(32768.0)).tobytes()
    f32 = P.edge_values(P.F32)
    assert P.mono(f32.tobytes(), P.F32, 1, op).tobytes() == f32.tobytes()  # bits preserved, the NaN's payload included


def test_f32_specials_survive_select_and_a_single_special_survives_mix():
    e = P.edge_values(P.F32)
    frames = np.zeros((len(e), 2), np.float32)
    frames[:, 1] = e
    raw = P.pack(frames, P.F32)
    assert P.mono(raw, P.F32, 2, 1).tobytes() == e.tobytes()
    m = P.mono(raw, P.F32, 2, P.MIX)
    assert np.isnan(m[4]) and np.isposinf(m[2]) and np.isneginf(m[3]) and m[5] == np.float32(2.0 ** -150) * 0 + np.float32(2.0 ** -149) * np.float32(0.5)


# ---- the library, without a device ----------------------------------------------------------------------------------
def test_header_constants_and_harness_agree(bn):
    header = open(os.path.join(ROOT, "include", "birdnet_hip.h")).read()
    for name, val in (("BN_PCM_I16", 0), ("BN_PCM_F32", 1), ("BN_PCM_I24", 2), ("BN_PCM_I32", 3), ("BN_PCM_U8", 4)):
        assert f"#define {name} {val}" in header and getattr(bn, name) == val == getattr(P, name[7:])
    assert "#define BN_PCM_MIX (-1)" in header and bn.BN_PCM_MIX == P.MIX == -1
    assert "#define BN_ABI_VERSION 2 " in header, "the new entry points come without an ABI bump"
    assert C.sizeof(bn.BnPcmLayout) == 12
    assert bn.PCM_SAMPLE_BYTES == P.SAMPLE_BYTES


def test_refusals_need_no_device(bn):
    """what is wrong with the arguments is said before a device is looked for, and no handle is written"""
    L = bn.lib
    pcm = (C.c_uint8 * 64)()
    rates = (C.c_uint32 * 1)(44100)

    def refused(call, needle):
        h = C.c_void_p(0xdead)
        assert call(h) == 1, needle  # BN_ERR_INVALID_ARG
        assert h.value is None, needle
        assert needle in bn.last_error(), (needle, bn.last_error())

    for lay, needle in ((bn.BnPcmLayout(5, 1, 0), "unknown PCM format"), (bn.BnPcmLayout(-1, 1, 0), "unknown PCM format"),
                        (bn.BnPcmLayout(2, 0, 0), "channels"), (bn.BnPcmLayout(2, 17, 0), "channels"),
                        (bn.BnPcmLayout(2, 2, 2), "channel"), (bn.BnPcmLayout(2, 2, -2), "channel")):
        refused(lambda h: L.bn_recording_create_layout(0, pcm, 2, C.byref(lay), C.sizeof(lay), C.byref(h)), needle)
        refused(lambda h: L.bn_recording_create_layout_async(0, pcm, 2, C.byref(lay), C.sizeof(lay), C.byref(h)), needle)
        refused(lambda h: L.bn_recording_create_layout_resampled(0, pcm, 2, C.byref(lay), C.sizeof(lay), 44100, 48000, 0, C.byref(h)), needle)
        refused(lambda h: L.bn_live_create_layout(0, 1, C.byref(lay), C.sizeof(lay), 256, 100, 1024, 0, None, 0, C.byref(h)), needle)
        refused(lambda h: L.bn_live_create_layout(0, 1, C.byref(lay), C.sizeof(lay), 256, 100, 4096, 48000, rates, 0, C.byref(h)), needle)
    ok = bn.BnPcmLayout(2, 2, -1)
    refused(lambda h: L.bn_recording_create_layout(0, pcm, 2, None, C.sizeof(ok), C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_recording_create_layout_async(0, pcm, 2, None, C.sizeof(ok), C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_recording_create_layout_resampled(0, pcm, 2, None, C.sizeof(ok), 1, 2, 0, C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_live_create_layout(0, 1, None, C.sizeof(ok), 256, 100, 1024, 0, None, 0, C.byref(h)), "null PCM layout")
    refused(lambda h: L.bn_recording_create_layout(0, pcm, 2, C.byref(ok), 8, C.byref(h)), "struct_size")
    refused(lambda h: L.bn_recording_create_layout(0, pcm, 2 ** 63, C.byref(ok), C.sizeof(ok), C.byref(h)), "exceeds the address space")
    refused(lambda h: L.bn_recording_view_channel(None, 0, C.byref(h)), "null recording")
    # the mono entry points still take I16 and F32 only
    refused(lambda h: L.bn_recording_create(0, pcm, 2, 2, C.byref(h)), "unknown PCM format")
    refused(lambda h: L.bn_live_create(0, 1, 4, 256, 100, 1024, C.byref(h)), "unknown PCM format")


def test_sanitizer_program_over_the_layout_arithmetic(tmp_path):
    """tools/asan_pcm_layout.cpp under -fsanitize=address,undefined: frame and byte offsets, chunk cuts at frame boundaries for
    every format x channels 1..16, overflow refusals"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "asan_pcm_layout")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "rust-birdnet-onnx_amd", "csrc"), os.path.join(ROOT, "tools", "asan_pcm_layout.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip; any other compile / link error is a finding
        if "cannot find -lasan" in r.stderr or "cannot find -lubsan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
            pytest.skip("no libasan / libubsan in this image")
        pytest.fail("host-only sanitizer build of the layout check failed:\n" + r.stderr[-3000:])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "asan_pcm_layout: ok" in out.stdout
