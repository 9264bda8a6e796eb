"""The PCM layout rule of include/birdnet_hip.h ("PCM layouts") restated in numpy: interleaved frames of `channels` samples in
one of five little-endian formats -> the mono f32 sample every consumer of a layout recording or pool must see.  Every operation
is an f32 operation, in the order the rule states; nothing is fused.  Shared by test_pcm_layout_cpu.py (which checks this file
against an independent float64 evaluation) and test_gpu_pcm_layout.py (which checks the device against this file, bit for bit)."""
import numpy as np

I16, F32, I24, I32, U8 = 0, 1, 2, 3, 4
MIX = -1
FORMATS = (I16, F32, I24, I32, U8)
SAMPLE_BYTES = {I16: 2, F32: 4, I24: 3, I32: 4, U8: 1}
NAMES = {I16: "i16", F32: "f32", I24: "i24", I32: "i32", U8: "u8"}


def pack(values, fmt) -> bytes:
    """integer sample values (float32 values for F32), any shape, row-major -> the storage bytes"""
    v = np.asarray(values)
    if fmt == I16:
        return v.astype("<i2").tobytes()
    if fmt == F32:
        return v.astype("<f4").tobytes()
    if fmt == I32:
        return v.astype("<i4").tobytes()
    if fmt == U8:
        return v.astype(np.uint8).tobytes()
    assert fmt == I24
    u = (v.astype(np.int64).reshape(-1) & 0xFFFFFF).astype(np.uint32)
    out = np.empty((u.shape[0], 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = u & 0xFF, (u >> 8) & 0xFF, (u >> 16) & 0xFF
    return out.tobytes()


def unpack_ints(raw: bytes, fmt) -> np.ndarray:
    """the stored integers of an integer format, int64 [n]; I24 sign-extended, U8 as stored (0..255)"""
    b = np.frombuffer(raw, np.uint8)
    if fmt == I16:
        return b.view("<i2").astype(np.int64)
    if fmt == I32:
        return b.view("<i4").astype(np.int64)
    if fmt == U8:
        return b.astype(np.int64)
    assert fmt == I24
    t = b.reshape(-1, 3).astype(np.int64)
    v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16)
    return np.where(v & 0x800000, v - (1 << 24), v)


def samples_f32(raw: bytes, fmt) -> np.ndarray:
    """every stored sample as the rule's f32, [n]"""
    if fmt == F32:
        return np.frombuffer(raw, "<f4").astype(np.float32)  # the bits as they are
    v = unpack_ints(raw, fmt)
    if fmt == I16:
        return v.astype(np.float32) / np.float32(32768.0)
    if fmt == I24:
        return v.astype(np.float32) / np.float32(8388608.0)
    if fmt == I32:
        return v.astype(np.int32).astype(np.float32) * np.float32(2.0 ** -31)  # int32 -> f32 rounds to nearest even
    return (v - 128).astype(np.float32) / np.float32(128.0)


def mono(raw: bytes, fmt, channels, channel) -> np.ndarray:
    """the rule: f32 [n_frames] of `raw` read as {fmt, channels, channel}"""
    s = samples_f32(raw, fmt).reshape(-1, channels)
    if channels == 1:
        return s[:, 0].copy()  # both ops are the identity
    if channel >= 0:
        return s[:, channel].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        acc = s[:, 0].copy()
        for c in range(1, channels):
            acc = (acc + s[:, c]).astype(np.float32)
        inv = np.float32(1.0) / np.float32(channels)
        return (acc * inv).astype(np.float32)


def chunk_audio(x, S, step) -> np.ndarray:
    """chunk_audio over f32 samples x: one window per k * step < len, the tail zero-padded; f32 [G, S]"""
    n = (len(x) + step - 1) // step if len(x) else 0
    out = np.zeros((n, S), dtype=np.float32)
    for k in range(n):
        seg = x[k * step:k * step + S]
        out[k, :len(seg)] = seg
    return out


def edge_values(fmt) -> np.ndarray:
    """min, max, zero and neighbours for an integer format; +-0, +-inf, a NaN with a payload and denormals for F32"""
    if fmt == F32:
        bits = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC12345, 0x00000001, 0x807FFFFF, 0x3F800000, 0xBF800000], np.uint32)
        return bits.view(np.float32)
    lo, hi = {I16: (-32768, 32767), I24: (-8388608, 8388607), I32: (-2 ** 31, 2 ** 31 - 1), U8: (0, 255)}[fmt]
    mid = 128 if fmt == U8 else 0
    return np.array([lo, hi, mid, lo + 1, hi - 1, mid + 1, mid - 1], np.int64)


def test_data(rng, fmt, n_frames, channels) -> bytes:
    """n_frames frames of random samples with the format's edge values spread over the channels and byte phases: edge value j
    sits in frame 5 j + 1, channel j % channels, three rounds of them.  One special value per frame at most: a mix of +inf and
    -inf, or of two NaNs, GENERATES a NaN, whose sign and payload IEEE 754 leaves to the implementation -- the rule cannot
    define its bits.  A single NaN or inf per frame propagates with its bits through the adds and the scale."""
    n = n_frames * channels
    e = edge_values(fmt)
    if fmt == F32:
        v = rng.uniform(-1, 1, n).astype(np.float32)
    else:
        lo, hi = {I16: (-32768, 32767), I24: (-8388608, 8388607), I32: (-2 ** 31, 2 ** 31 - 1), U8: (0, 255)}[fmt]
        v = rng.randint(lo, hi + 1, size=n, dtype=np.int64)
    v = v.reshape(n_frames, channels)
    for j in range(3 * len(e)):
        if 5 * j + 1 < n_frames:
            v[5 * j + 1, j % channels] = e[j % len(e)]
    return pack(v, fmt)
