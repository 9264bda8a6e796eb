"""bn_recording_template_match on the GPU against tests/template_ref.py (numpy int64 sums, float64 quotient).

In every case the reference's input is the uint8 image the device's own spectrogram(..., u8=...) returns for the frames the match
reads, so the new stage is isolated and "the match reads that image" is pinned.  Pass condition: every score within 1 float32 ulp
of the reference -- every integer is exact and the inexact steps are one double product, one root and one quotient, whose few
double ulps can move the final float32 rounding by one place at most.  The invariance runs byte for byte.  Each comparison prints
how many scores are not bit-identical.

A template of one element (1 frame x 1 row) has dT == 0 by the rule and is refused at creation: at R = 1 the sets' 1-frame
templates are asserted refused and run with 2 frames instead."""
import ctypes as C

import numpy as np
import pytest

import pcm_ref
import template_ref as ref

pytestmark = pytest.mark.gpu
N, HOP, U8, FRAMES = 256, 100, (1e-3, 60.0), 172  # 130 offsets + 40 frames - 1, and frames that start at or past the end
SCENES = {}


def _scene(bn, rows):
    """(recording, the spectrogram's row arguments, its uint8 image of FRAMES frames), made once per kind of rows: noise whose level
    wanders over 40 dB, so the codes spread"""
    if rows not in SCENES:
        rng, n = np.random.RandomState(17), (FRAMES - 2) * HOP
        level = 10.0 ** (-2.5 + np.cumsum(rng.standard_normal(n)) * 0.004 % 2.0)
        rec = bn.Recording((rng.standard_normal(n) * level).astype(np.float32))
        n_fft = 512 if rows == "mel" else N
        kw = {"bank": bn.Filterbank(0, 512, bn.mel_filterbank(48000, 512, 30, 0.0, 24000.0))} if rows == "mel" else {"bins": (3, 3 + rows)}
        img = rec.spectrogram(0, FRAMES, n_fft, HOP, u8=U8, **kw)
        assert len(np.unique(img)) > 30 and not img[-2:].any()
        SCENES[rows] = (rec, n_fft, kw, img)
    return SCENES[rows]


def _templates(img, lengths, seed=0):
    """even positions cut from the image, odd ones random bytes; none flat"""
    rng, out = np.random.RandomState(seed + len(lengths)), []
    for q, W in enumerate(lengths):
        at = rng.randint(0, len(img) - W - 2)
        t = img[at:at + W].copy() if q % 2 == 0 else rng.randint(0, 256, size=(W, img.shape[1])).astype(np.uint8)
        if t.min() == t.max():
            t[0, 0] ^= 1
        out.append(t)
    return out


def _check(got, image, templates, what):
    want = ref.scores(image, templates)
    assert got.dtype == np.float32 and got.shape == want.shape, what
    near = (got == want) | (got == np.nextafter(want, np.float32(2))) | (got == np.nextafter(want, np.float32(-2)))
    print(what, "scores not bit-identical:", int((got.view(np.uint32) != want.view(np.uint32)).sum()), "of", got.size)
    assert near.all() and np.signbit(got[want == 0]).sum() == 0, (what, got[~near], want[~near])


SETS = {"one": [1], "mixed": [1, 40, 7, 13, 2, 33, 5, 21, 3, 38, 11, 4, 27, 9, 16, 6, 30], "many": [3] * 64}


@pytest.mark.parametrize("n_offsets", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("rows", (1, 15, 16, 17, 80, "mel"))
@pytest.mark.parametrize("name", sorted(SETS))
def test_against_the_reference(bn, name, rows, n_offsets):
    """a partial tile, a full one, one offset into the next, three tiles; one unit and its padding, two units, five, a bank; one
    tile of templates, a ragged second tile, four full tiles"""
    rec, n_fft, kw, img = _scene(bn, rows)
    lengths = SETS[name]
    if rows == 1 and 1 in lengths:
        with pytest.raises(bn.EngineError):
            bn.Templates(0, _templates(img, lengths))
        assert "flat" in bn.last_error()
        lengths = [max(W, 2) for W in lengths]
    templates = _templates(img, lengths)
    tpl = bn.Templates(0, templates)
    assert (tpl.n_templates, tpl.n_rows, tpl.max_frames) == (len(lengths), img.shape[1], max(lengths))
    frames = n_offsets + max(lengths) - 1
    image = rec.spectrogram(0, frames, n_fft, HOP, u8=U8, **kw)
    assert image.tobytes() == img[:frames].tobytes()
    _check(rec.template_match(0, n_offsets, n_fft, HOP, tpl, u8=U8, **kw), image, templates, (name, rows, n_offsets))


def test_the_cap(bn):
    """one template of 128 x 512 = 65 536 elements over codes that are almost all 0 or 255: |A| and S2 near 2^30, K A near 2^46"""
    n_fft, hop, n_off = 1024, 256, 70
    rng, parts = np.random.RandomState(23), []
    while sum(map(len, parts)) < (n_off + 127) * hop + n_fft:
        parts += [rng.uniform(-1.0, 1.0, rng.randint(1500, 9000)).astype(np.float32), np.zeros(rng.randint(1500, 9000), np.float32)]
    rec, u8 = bn.Recording(np.concatenate(parts)), (1e-12, 10.0)
    image = rec.spectrogram(0, n_off + 127, n_fft, hop, bins=(0, 512), u8=u8)
    assert np.isin(image, (0, 255)).mean() >= 0.95 and 0.2 < (image == 255).mean() < 0.8
    templates = [image[5:133].copy(), 255 - image[5:133]]
    got = rec.template_match(0, n_off, n_fft, hop, bn.Templates(0, templates), bins=(0, 512), u8=u8)
    assert got[0, 5].tobytes() == np.float32(1.0).tobytes() and got[1, 5].tobytes() == np.float32(-1.0).tobytes()
    _check(got, image, templates, "the cap")


def test_known_answers(bn):
    rng = np.random.RandomState(29)
    x = (rng.standard_normal(60 * HOP + N) * 0.05).astype(np.float32)
    x[20 * HOP:32 * HOP] = 0.0   # frames 20 .. 28 are digital silence: code 0 in every row
    x[45 * HOP + 7] = np.nan     # frames 43, 44, 45 read it: code 255 in every row
    rec = bn.Recording(x)
    image = rec.spectrogram(0, 56, N, HOP, bins=(0, 40), u8=U8)
    assert not image[20:29].any() and (image[43:46] == 255).all() and len(np.unique(image[:20])) > 30
    templates = [image[4:9].copy(), image[36:42].copy(), image[41:47].copy()]  # the last one holds the NaN frames
    got = rec.template_match(0, 51, N, HOP, bn.Templates(0, templates), bins=(0, 40), u8=U8)
    _check(got, image, templates, "known answers")
    assert got[0, 20:25].tobytes() == bytes(5 * 4) and got[1, 20:24].tobytes() == bytes(4 * 4)  # a flat window: +0.0f bit for bit
    hits = bn.template_peaks(got, 0.999, 3)
    assert [(h["offset"], h["template_index"], h["score"]) for h in hits] == [(4, 0, 1.0), (36, 1, 1.0), (41, 2, 1.0)]


def test_invariance_byte_for_byte(bn):
    s, n, rng = 333, 90, np.random.RandomState(5)
    vals = rng.randint(-2 ** 23, 2 ** 23, size=(s + 110 * HOP + N - 77, 2))
    raw = pcm_ref.pack(vals, pcm_ref.I24)
    rec, kind = bn.Recording(pcm_ref.mono(raw, pcm_ref.I24, 2, 1)), {"bins": (2, 50), "u8": (1e-2, 60.0)}
    image = rec.spectrogram(s, n + 19, N, HOP, **kind)
    templates = _templates(image, [20, 3, 9, 14])
    tpl = bn.Templates(0, templates)
    whole = rec.template_match(s, n, N, HOP, tpl, **kind)
    _check(whole, image, templates, "invariance")
    split = np.concatenate([rec.template_match(s, 37, N, HOP, tpl, **kind), rec.template_match(s + 37 * HOP, n - 37, N, HOP, tpl, **kind)], axis=1)
    assert split.tobytes() == whole.tobytes()
    assert rec.template_match(s + 5 * HOP, n - 5, N, HOP, tpl, **kind).tobytes() == whole[:, 5:].tobytes()
    assert bn.Recording.from_layout(raw, bn.BN_PCM_I24, 2, 1).template_match(s, n, N, HOP, tpl, **kind).tobytes() == whole.tobytes()
    # alone, and inside a larger set that also holds shorter and longer templates (20 frames stay the longest: the same image)
    larger = bn.Templates(0, _templates(image, [5] * 17, seed=1) + templates + _templates(image, [20] * 30, seed=2))
    assert rec.template_match(s, n, N, HOP, larger, **kind)[17:21].tobytes() == whole.tobytes()
    for q in (0, 2):  # the longest alone, and a shorter one alone: its call reads a shorter image
        assert rec.template_match(s, n, N, HOP, bn.Templates(0, templates[q:q + 1]), **kind).tobytes() == whole[q].tobytes()
    host = bn.HostRecording(raw, bn.BN_PCM_I24, 2, 1)
    assert host.template_match(s, n, N, HOP, bn.HostTemplates(templates), **kind).tobytes() == whole.tobytes()


def test_refusals_leave_the_output_untouched(bn):
    L = bn.lib
    rec, fb = bn.Recording(np.zeros(1000, dtype=np.float32)), bn.Filterbank(0, N, np.ones((3, 129), np.float32))
    cut = np.arange(2 * 40, dtype=np.uint8).reshape(2, 40)
    tpl, tpl3 = bn.Templates(0, [cut, cut[:1]]), bn.Templates(0, [cut[:, :3]])
    out = np.full(2 * 4 + 2, 0x5A5A5A5A, dtype=np.uint32)

    def call(r=rec._h, first=0, n=4, spec=(N, 100, 0, 40, 1, 1.0, 80.0), size=28, bank=None, t=tpl._h, o=out, floats=8):
        sp = bn.BnSpectrogramSpec(*spec) if spec else None
        return L.bn_recording_template_match(r, first, n, C.byref(sp) if sp else None, size, bank, t, o.ctypes.data_as(C.POINTER(C.c_float)) if o is not None else None, floats)

    for kw, word in (({"r": None}, "null recording"), ({"spec": None}, "null spectrogram spec"), ({"size": 27}, "spec_size"), ({"spec": (1000, 100, 0, 40, 1, 1.0, 80.0)}, "frame 1000"),
                     ({"spec": (N, 0, 0, 40, 1, 1.0, 80.0)}, "hop 0"), ({"spec": (N, 100, 5, 5, 1, 1.0, 80.0)}, "bins ["), ({"spec": (N, 100, 0, 40, 1, 0.0, 80.0)}, "ref_power"),
                     ({"spec": (N, 100, 0, 40, 1, 1.0, 80.0), "bank": fb._h}, "must both be 0"), ({"first": 1001}, "first_sample 1001"),
                     ({"spec": (N, 100, 0, 40, 0, 0.0, 0.0)}, "U8"), ({"t": None}, "null templates"), ({"o": None}, "null output"),
                     ({"spec": (N, 100, 0, 41, 1, 1.0, 80.0)}, "40 rows"), ({"spec": (N, 100, 0, 0, 1, 1.0, 80.0), "bank": fb._h}, "40 rows"),
                     ({"floats": 7}, "out_floats"), ({"n": 2 ** 63}, "do not fit")):
        assert call(**kw) == 1 and word in bn.last_error(), (kw, bn.last_error())
    assert (out == 0x5A5A5A5A).all()
    assert call(n=0, floats=0) == 0 and call(spec=(N, 100, 0, 0, 1, 1.0, 80.0), bank=fb._h, t=tpl3._h, floats=4) == 0
    assert call() == 0 and (out[8:] == 0x5A5A5A5A).all() and not out[:8].any()  # silence scores +0.0f, and nothing behind the scores

    def create(n=1, rows=4, frames=(2,), codes=np.arange(8, dtype=np.uint8), o=True):
        h, fr = C.c_void_p(0x77), np.array(frames or (1,), dtype=np.uint32)
        st = L.bn_templates_create(0, n, rows, fr.ctypes.data_as(C.POINTER(C.c_uint32)) if frames else None,
                                   codes.ctypes.data_as(C.POINTER(C.c_uint8)) if codes is not None else None, C.byref(h) if o else None)
        assert st == 0 or not o or h.value is None
        return st

    big = np.arange(129 * 512, dtype=np.uint32).astype(np.uint8)
    for kw, word in (({"frames": None}, "null"), ({"codes": None}, "null"), ({"o": False}, "null"), ({"n": 0}, "n_templates 0"), ({"n": 65, "frames": (1,) * 65}, "n_templates 65"),
                     ({"rows": 0}, "n_rows 0"), ({"rows": 513}, "n_rows 513"), ({"frames": (0,)}, "template 0 has 0 frames"),
                     ({"rows": 4, "frames": (129,), "codes": big}, "129 frames"), ({"rows": 512, "frames": (128, 128), "n": 2, "codes": np.concatenate([big[:65536], np.zeros(65536, np.uint8)])}, "template 1 is flat"),
                     ({"n": 2, "frames": (1, 1), "codes": np.array([1, 2, 3, 4, 9, 9, 9, 9], np.uint8)}, "template 1 is flat")):
        assert create(**kw) == 1 and word in bn.last_error(), (kw, bn.last_error())
    if bn.device_count() > 1:
        assert call(t=bn.Templates(1, [cut])._h) == 1 and "device" in bn.last_error()
