"""bn_recording_spectrogram on the GPU against tests/spectrogram_ref.py (float64, numpy.fft.rfft over frames cut by the rule).

Every float is compared within the header's bound (spectrogram_ref.image, from the BN_SPECTROGRAM_* and BN_BAND_* constants as the
header declares them); U8 images byte for byte against the threshold table applied to the F32 image of the same call; the invariance
runs byte for byte.  tests/test_spectrogram_cpu.py shows on the inputs below that four wrong rules leave those bounds.  Each test
prints its worst error as a share of the bound."""
import ctypes as C

import numpy as np
import pytest

import pcm_ref
import spectrogram_ref as ref

pytestmark = pytest.mark.gpu


def _f32(v):
    return pcm_ref.mono(pcm_ref.pack(v, pcm_ref.I16), pcm_ref.I16, 1, 0)


def _check(got, x, first, n_frames, N, hop, what, **kind):
    want, bound = ref.image(x, first, n_frames, N, hop, **kind)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    share = ref.worst_share(got, want, bound)
    print(what, "worst error / bound", share)
    assert share <= 1.0, (what, share)
    return share


@pytest.mark.parametrize("n_frames", (1, 15, 16, 17, 33))
@pytest.mark.parametrize("N", ref.FRAMES)
def test_bins_against_float64(bn, N, n_frames):
    """a wave with no frame, a full tile, one frame into the next tile, three tiles; the input ends inside the last frame"""
    worst = 0.0
    for hop in (N, N // 2, 100):
        v = ref.noise(N, n_frames, hop)
        rec, x = bn.Recording(v), _f32(v)
        for bins in ((0, N // 2 + 1), (1, 2), (N // 4 - 3, N // 4 + 8)):
            worst = max(worst, _check(rec.spectrogram(0, n_frames, N, hop, bins=bins), x, 0, n_frames, N, hop, (N, n_frames, hop, bins), bins=bins))
    print("frame", N, "frames", n_frames, "worst error / bound:", worst)


@pytest.mark.parametrize("N,n_frames,bank", [(256, 17, ("random", 1)), (256, 17, ("random", 16)), (256, 17, ("random", 17)), (256, 33, ("random", 80)),
                                             (256, 17, ("mel", 16)), (2048, 17, ("mel", 128))])
def test_bank_against_float64(bn, N, n_frames, bank):
    """padding inside a row tile, waves without a tile, a wave with two tiles; a dense bank (every K step live) and mel banks (few
    steps per tile); 128 mel rows at frame 2048: the LDS opt-in and the longest chain"""
    W = ref.random_bank(N, bank[1]) if bank[0] == "random" else bn.mel_filterbank(48000, N, bank[1], 0.0, 24000.0)
    v = ref.noise(N, n_frames, 100)
    fb = bn.Filterbank(0, N, W)
    assert (fb.n_rows, fb.frame, bn.lib.bn_filterbank_frame(fb._h)) == (bank[1], N, N)
    _check(bn.Recording(v).spectrogram(0, n_frames, N, 100, bank=fb), _f32(v), 0, n_frames, N, 100, (N, n_frames, bank), bank=W)


@pytest.mark.parametrize("N", (256, 1024))
def test_selection_bank_is_the_bins_image(bn, N):
    """fragment order and step skipping: a row with one weight of 1.0 is that bin's row, far closer than any neighbouring bin"""
    W, cols = ref.selection_bank(N)
    rec, c = bn.Recording(ref.noise(N, 19, 100)), ref.header_constants()
    E, P = rec.spectrogram(0, 19, N, 100, bank=bn.Filterbank(0, N, W)).astype(np.float64), rec.spectrogram(0, 19, N, 100, bins=(0, N // 2 + 1))[:, cols].astype(np.float64)
    rel = np.abs(E - P) / P
    print("selection bank, frame", N, "worst relative difference", rel.max())
    assert P.min() > 0 and (rel <= 2.0 ** -21 + c["BN_SPECTROGRAM_BANK_DEPTH"] * ref.U).all()


@pytest.mark.parametrize("kind", ("bins", "bank"))
def test_u8_is_the_table(bn, kind):
    N, hop, n, range_db = 512, 100, 21, 20.0
    v = ref.noise(N, n, hop)
    v[5 * hop:5 * hop + N + hop] = 0  # frames 5 and 6 are silent: 0.0, code 0
    rec = bn.Recording(v)
    rows = {"bins": (3, 140)} if kind == "bins" else {"bank": bn.Filterbank(0, N, bn.mel_filterbank(48000, N, 30, 0.0, 24000.0))}
    img = rec.spectrogram(0, n, N, hop, **rows)
    # a ref_power that puts pixel (2, 7) exactly on a threshold: the table's own rounding decides, so ask the table
    pixel, ref_power = img[2, 7], None
    for j in range(254, 200, -1):
        rp = np.float32(float(pixel) / 10.0 ** (((j + 0.5) * range_db / 255.0 - range_db) / 10.0))
        if bn.spectrogram_thresholds(rp, range_db)[j] == pixel:
            ref_power = rp
            break
    assert ref_power is not None
    thr = bn.spectrogram_thresholds(ref_power, range_db)
    got, want = rec.spectrogram(0, n, N, hop, u8=(ref_power, range_db), **rows), ref.codes(thr, img)
    assert got.dtype == np.uint8 and got.tobytes() == want.tobytes()
    assert got[2, 7] == j + 1 and got.min() == 0 and got.max() == 255 and (got[5:7] == 0).all() and len(np.unique(got)) > 100


def test_known_answer(bn):
    """a bin-centred sine of amplitude a: a^2 / 2 in the centre bin and its two neighbours, 2/3 of it in the centre; silence is 0.0"""
    N, k0, a = 256, 20, 0.5
    x = np.concatenate([a * np.sin(2 * np.pi * k0 * np.arange(4 * N) / N), np.zeros(2 * N)]).astype(np.float32)
    rec = bn.Recording(x)
    img = rec.spectrogram(0, 6, N, N, bins=(0, N // 2 + 1))
    assert (np.abs(img[:4, k0 - 1:k0 + 2].sum(axis=1) - a * a / 2) < 1e-6).all() and (np.abs(img[:4, k0] - a * a / 3) < 1e-6).all()
    assert img[4:].tobytes() == bytes(img[4:].nbytes)
    assert not rec.spectrogram(0, 6, N, N, bins=(0, N // 2 + 1), u8=(1.0, 80.0))[4:].any()


def test_invariance_byte_for_byte(bn):
    N, hop, s = 512, 100, 333
    rng = np.random.RandomState(5)
    vals = rng.randint(-2 ** 23, 2 ** 23, size=(s + 40 * hop + N - 77, 2))
    raw = pcm_ref.pack(vals, pcm_ref.I24)
    x = pcm_ref.mono(raw, pcm_ref.I24, 2, 1)
    rec, W = bn.Recording(x), bn.mel_filterbank(48000, N, 30, 0.0, 24000.0)
    fb = bn.Filterbank(0, N, W)
    for kind in ({"bins": (2, 201)}, {"bank": fb, "u8": (1e-2, 60.0)}, {"bank": fb}):
        whole = rec.spectrogram(s, 40, N, hop, **kind)
        assert rec.spectrogram(s + 5 * hop, 35, N, hop, **kind).tobytes() == whole[5:].tobytes()  # where a frame falls in a tile and the grid
        assert bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 1).spectrogram(s, 40, N, hop, **kind).tobytes() == whole.tobytes()  # the layout
        assert np.concatenate([rec.spectrogram(s, 20, N, hop, **kind), rec.spectrogram(s + 20 * hop, 20, N, hop, **kind)]).tobytes() == whole.tobytes()
        longer = bn.Recording(np.concatenate([rng.standard_normal(4321).astype(np.float32), x]))  # the same samples before the same end
        assert longer.spectrogram(4321 + s, 40, N, hop, **kind).tobytes() == whole.tobytes()
    host = bn.HostRecording(raw, bn.BN_PCM_I24, 2, 1)
    assert host.spectrogram(s, 40, N, hop, bins=(2, 201)).tobytes() == rec.spectrogram(s, 40, N, hop, bins=(2, 201)).tobytes()
    assert host.spectrogram(s, 40, N, hop, bank=bn.HostFilterbank(N, W), u8=(1e-2, 60.0)).tobytes() == rec.spectrogram(s, 40, N, hop, bank=fb, u8=(1e-2, 60.0)).tobytes()
    # the row of bin k is plane 0 of the spectral profile of a window that holds only that frame
    _, planes = rec.spectral_profile(N, hop, N, N, (2, 201), first=3, count=4)
    assert planes[:, 0].tobytes() == rec.spectrogram(3 * hop, 4, N, hop, bins=(2, 201)).tobytes()
    # a filtered recording as source: it runs, and matches the reference on the samples it reads back
    filt = rec.filtered(bn.fir_bandpass(48000, 1000.0, 8000.0, 63))
    _check(filt.spectrogram(s, 40, N, hop, bank=fb), filt.read_f32(), s, 40, N, hop, "filtered source", bank=W)


def test_past_the_end_and_non_finite_samples(bn):
    N, hop = 256, 100
    x = _f32(ref.noise(N, 10, hop, seed=1)).copy()  # ends N // 3 short of frame 9's end
    n = 10 + 4  # frames 10 .. 13 start at or past the end, or reach it with a few samples
    clean = bn.Recording(x).spectrogram(0, n, N, hop, bins=(0, N // 2 + 1))
    _check(clean, x, 0, n, N, hop, "past the end", bins=(0, N // 2 + 1))
    assert bn.Recording(x).spectrogram(len(x), 3, N, hop, bins=(0, 5)).tobytes() == bytes(3 * 5 * 4)  # wholly past the end: zeros
    W = ref.random_bank(N, 17)
    fb, clean_bank = bn.Filterbank(0, N, W), bn.Recording(x).spectrogram(0, n, N, hop, bank=bn.Filterbank(0, N, W))
    for value in (np.nan, np.inf):
        y = x.copy()
        y[4 * hop + 7] = value  # read by frames 2, 3, 4
        hit = np.zeros(n, dtype=bool)
        hit[2:5] = True
        for got, base in ((bn.Recording(y).spectrogram(0, n, N, hop, bins=(0, N // 2 + 1)), clean), (bn.Recording(y).spectrogram(0, n, N, hop, bank=fb), clean_bank)):
            assert np.isposinf(got[hit]).all() and got[~hit].tobytes() == base[~hit].tobytes()
        assert (bn.Recording(y).spectrogram(0, n, N, hop, bank=fb, u8=(1.0, 80.0))[hit] == 255).all()


def test_refusals_leave_the_output_untouched(bn):
    L, N = bn.lib, 256
    rec, fb, fb512 = bn.Recording(np.zeros(1000, dtype=np.float32)), bn.Filterbank(0, N, np.ones((3, 129), np.float32)), bn.Filterbank(0, 512, np.ones((3, 257), np.float32))
    out = np.full(4 * 129 + 8, 0x5A, dtype=np.uint8)
    nan, inf = float("nan"), float("inf")

    def call(r=rec._h, first=0, n=1, spec=(N, 100, 0, 129, 0, 0.0, 0.0), size=28, bank=None, o=out, nbytes=4 * 129):
        sp = bn.BnSpectrogramSpec(*spec) if spec else None
        return L.bn_recording_spectrogram(r, first, n, C.byref(sp) if sp else None, size, bank, o.ctypes.data_as(C.c_void_p) if o is not None else None, nbytes)

    for kw, word in (({"r": None}, "null recording"), ({"spec": None}, "null spectrogram spec"), ({"o": None}, "null output"), ({"size": 27}, "spec_size"),
                     ({"spec": (1000, 100, 0, 129, 0, 0.0, 0.0)}, "frame 1000"), ({"spec": (N, 0, 0, 129, 0, 0.0, 0.0)}, "hop 0"),
                     ({"spec": (N, 257, 0, 129, 0, 0.0, 0.0)}, "hop 257"), ({"spec": (N, 100, 0, 129, 2, 0.0, 0.0)}, "format"),
                     ({"spec": (N, 100, 5, 5, 0, 0.0, 0.0)}, "bins ["), ({"spec": (N, 100, 0, 130, 0, 0.0, 0.0)}, "bins ["),
                     ({"spec": (N, 100, 0, 129, 0, 0.0, 0.0), "bank": fb._h}, "must both be 0"), ({"spec": (N, 100, 0, 0, 0, 0.0, 0.0), "bank": fb512._h}, "of frame 512"),
                     ({"spec": (N, 100, 0, 129, 1, 0.0, 80.0)}, "ref_power"), ({"spec": (N, 100, 0, 129, 1, inf, 80.0)}, "ref_power"),
                     ({"spec": (N, 100, 0, 129, 1, 1.0, -1.0)}, "range_db"), ({"spec": (N, 100, 0, 129, 1, 1.0, nan)}, "range_db"),
                     ({"first": 1001}, "first_sample 1001"), ({"nbytes": 4 * 129 - 1}, "out_bytes"), ({"n": 2 ** 62}, "do not fit")):
        assert call(**kw) == 1 and word in bn.last_error(), (kw, bn.last_error())
    assert (out == 0x5A).all()
    assert call(n=0, o=None, nbytes=0) == 0 and call(first=1000, n=0) == 0  # n_frames == 0 is BN_OK
    assert call() == 0 and (out[4 * 129:] == 0x5A).all() and not out[:4 * 129].any()  # silence, and nothing behind the image
    if bn.device_count() > 1:
        other = bn.Filterbank(1, N, np.ones((3, 129), np.float32))
        assert call(spec=(N, 100, 0, 0, 0, 0.0, 0.0), bank=other._h) == 1 and "device" in bn.last_error()
