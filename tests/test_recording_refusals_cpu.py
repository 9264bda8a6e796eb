"""The refusals of the recording entry points that are reached before a device is needed (include/birdnet_hip.h: bn_recording_*,
bn_infer_windows, bn_step_windows, bn_step_window_list, bn_chunk_count): every message word for word, and -- by giving an entry
point two faults at once -- the order in which they are looked for.  Through bn.lib alone; nothing here touches a device."""
import ctypes as C

INVALID = 1  # BN_ERR_INVALID_ARG
NULL_ARG = "null argument"
FORMAT = "unknown PCM format"
RATES = "sample rates must be positive"
NULL_LAYOUT = "null PCM layout"
SHORT_LAYOUT = "struct_size is below sizeof(bn_pcm_layout)"
CHANNELS = "channels must be in 1..16"
CHANNEL = "channel must be BN_PCM_MIX or in [0, channels)"
NULL_PCM = "null PCM buffer"
OVERFLOW = "n_frames * channels * bytes per sample exceeds the address space"
NULL_REC = "null recording"
SEGMENT = "segment_samples must be a positive multiple of 4"
I16, F32, I24 = 0, 1, 2


def refused(bn, status, message):
    assert status == INVALID, (status, message, bn.last_error())
    assert bn.last_error() == message, (bn.last_error(), message)


def creates(bn):
    """the six create forms as f(pcm, n, fmt or layout, out, **changes): mono forms take a format, layout forms a BnPcmLayout (or None)
    and `size`; the resampled forms take `rates`"""
    L = bn.lib

    def mono(fn, resampled):
        def call(pcm, n, fmt, out, rates=(44100, 48000)):
            return fn(0, pcm, n, fmt, *rates, 0, out) if resampled else fn(0, pcm, n, fmt, out)
        return call

    def layout(fn, resampled):
        def call(pcm, n, lay, out, rates=(44100, 48000), size=12):
            ref = None if lay is None else C.byref(lay)
            return fn(0, pcm, n, ref, size, *rates, 0, out) if resampled else fn(0, pcm, n, ref, size, out)
        return call

    return ({"create": mono(L.bn_recording_create, False), "create_async": mono(L.bn_recording_create_async, False),
             "create_resampled": mono(L.bn_recording_create_resampled, True)},
            {"create_layout": layout(L.bn_recording_create_layout, False), "create_layout_async": layout(L.bn_recording_create_layout_async, False),
             "create_layout_resampled": layout(L.bn_recording_create_layout_resampled, True)})


def test_every_create_form(bn):
    mono, lay = creates(bn)
    pcm = (C.c_uint8 * 96)()

    def check(call, message, *args, **kw):
        h = C.c_void_p(0xdead)
        refused(bn, call(*args, C.byref(h), **kw), message)
        assert h.value is None, (message, "the handle is cleared before anything is refused")

    for name, call in mono.items():
        refused(bn, call(pcm, 2, I16, None), NULL_ARG)
        refused(bn, call(None, 2, 7, None), NULL_ARG)  # ... before anything else
        for fmt in (-1, I24, 5):  # the mono forms take I16 and F32 only
            check(call, FORMAT, pcm, 2, fmt)
        check(call, FORMAT, None, 2, 5)  # the format before the buffer
        check(call, NULL_PCM, None, 2, I16)
        check(call, NULL_PCM, None, 2 ** 63, F32)  # the buffer before the size
        for n, fmt in ((2 ** 63, I16), (2 ** 63 - 1, I16), (2 ** 62, F32), (2 ** 64 - 1, F32)):
            check(call, OVERFLOW, pcm, n, fmt)
    for name, call in lay.items():
        ok = bn.BnPcmLayout(I24, 2, bn.BN_PCM_MIX)
        refused(bn, call(pcm, 2, ok, None), NULL_ARG)
        refused(bn, call(pcm, 2, None, None), NULL_ARG)
        check(call, NULL_LAYOUT, pcm, 2, None)
        check(call, NULL_LAYOUT, pcm, 2, None, size=4)  # the pointer before the size
        check(call, SHORT_LAYOUT, pcm, 2, ok, size=11)
        check(call, SHORT_LAYOUT, pcm, 2, bn.BnPcmLayout(9, 0, 5), size=0)  # the size before the layout is read
        for bad, message in ((bn.BnPcmLayout(5, 1, 0), FORMAT), (bn.BnPcmLayout(-1, 1, 0), FORMAT), (bn.BnPcmLayout(5, 0, 9), FORMAT),
                             (bn.BnPcmLayout(I24, 0, 0), CHANNELS), (bn.BnPcmLayout(I24, 17, 0), CHANNELS), (bn.BnPcmLayout(I24, 17, 17), CHANNELS),
                             (bn.BnPcmLayout(I24, 2, 2), CHANNEL), (bn.BnPcmLayout(I24, 2, -2), CHANNEL), (bn.BnPcmLayout(I16, 1, 1), CHANNEL)):
            check(call, message, pcm, 2, bad)
            check(call, message, None, 2 ** 63, bad)  # the layout before the buffer and the size
        check(call, NULL_PCM, None, 2, ok)
        check(call, NULL_PCM, None, 2 ** 63, ok)
        for n, l in ((2 ** 63, ok), (2 ** 64 // 6 + 1, ok), ((2 ** 64 - 16) // 6, ok), (2 ** 58, bn.BnPcmLayout(3, 16, 0))):
            check(call, OVERFLOW, pcm, n, l)
    # a longer struct of a later header is read through its first fields
    check(lay["create_layout"], NULL_PCM, None, 2, bn.BnPcmLayout(I24, 2, 0), size=64)

    # the resampled forms and their rates: the mono form looks at the rates before the format, the layout form reads and checks
    # the layout first
    for rates in ((0, 48000), (44100, 0), (0, 0)):
        check(mono["create_resampled"], RATES, pcm, 2, I16, rates=rates)
        check(mono["create_resampled"], RATES, pcm, 2, 5, rates=rates)  # two faults: the rates are reported
        check(mono["create_resampled"], RATES, None, 2 ** 63, I16, rates=rates)
        check(lay["create_layout_resampled"], RATES, pcm, 2, bn.BnPcmLayout(I24, 2, 0), rates=rates)
        check(lay["create_layout_resampled"], CHANNELS, pcm, 2, bn.BnPcmLayout(I24, 0, 0), rates=rates)  # two faults: the layout is reported
        check(lay["create_layout_resampled"], FORMAT, pcm, 2, bn.BnPcmLayout(5, 1, 0), rates=rates)
        check(lay["create_layout_resampled"], NULL_LAYOUT, pcm, 2, None, rates=rates)
        check(lay["create_layout_resampled"], SHORT_LAYOUT, pcm, 2, bn.BnPcmLayout(I24, 2, 0), rates=rates, size=8)
        check(lay["create_layout_resampled"], RATES, None, 2 ** 63, bn.BnPcmLayout(I24, 2, 0), rates=rates)  # the rates before buffer and size
    # equal rates take the plain path and refuse as it does
    check(mono["create_resampled"], NULL_PCM, None, 2, I16, rates=(48000, 48000))
    check(mono["create_resampled"], OVERFLOW, pcm, 2 ** 63, I16, rates=(48000, 48000))
    check(lay["create_layout_resampled"], NULL_PCM, None, 2, bn.BnPcmLayout(I24, 2, 0), rates=(48000, 48000))
    check(lay["create_layout_resampled"], OVERFLOW, pcm, 2 ** 63, bn.BnPcmLayout(I24, 2, 0), rates=(48000, 48000))


def test_a_null_recording(bn):
    L = bn.lib
    h = C.c_void_p(0xdead)
    refused(bn, L.bn_recording_view_channel(None, 0, C.byref(h)), NULL_REC)
    assert h.value is None
    refused(bn, L.bn_recording_view_channel(None, 0, None), NULL_ARG)  # the output before the recording
    refused(bn, L.bn_recording_wait(None), NULL_REC)
    out = (C.c_float * 8)()
    refused(bn, L.bn_recording_read_f32(None, 0, 4, out), NULL_ARG)
    refused(bn, L.bn_recording_read_f32(None, 0, 0, None), NULL_ARG)
    assert L.bn_recording_samples(None) == 0
    L.bn_recording_free(None)

    refused(bn, L.bn_recording_windows(None, 256, 100, 0, 1, out), NULL_REC)
    refused(bn, L.bn_recording_windows(None, 6, 0, 0, 1, None), NULL_REC)  # ... before the segment, the step and the buffer

    lv = (bn.BnWindowLevel * 2)()
    size = C.sizeof(bn.BnWindowLevel)
    refused(bn, L.bn_recording_levels(None, 256, 100, 0, 1, lv, size), NULL_REC)
    refused(bn, L.bn_recording_levels(None, 6, 0, 0, 1, None, size + 8), NULL_REC)
    refused(bn, L.bn_recording_levels(None, 256, 100, 0, 1, lv, size - 1), "struct_size is below sizeof(bn_window_level)")  # two faults: the size first
    refused(bn, L.bn_recording_levels(None, 256, 100, 0, 0, None, 0), "struct_size is below sizeof(bn_window_level)")

    bands = (bn.BnWindowBands * 2)()
    size = C.sizeof(bn.BnWindowBands)
    spec = bn.band_spec(256, 128, [(0, 10)])
    refused(bn, L.bn_recording_band_levels(None, 1024, 100, 0, 1, C.byref(spec), C.sizeof(spec), bands, size), NULL_REC)
    refused(bn, L.bn_recording_band_levels(None, 6, 0, 0, 1, None, 0, None, size + 8), NULL_REC)  # ... before the segment and the spec
    refused(bn, L.bn_recording_band_levels(None, 1024, 100, 0, 1, C.byref(spec), C.sizeof(spec), bands, size - 1),
            "struct_size is below sizeof(bn_window_bands)")  # two faults: the size first
    refused(bn, L.bn_recording_band_levels(None, 1024, 100, 0, 0, None, 0, None, 0), "struct_size is below sizeof(bn_window_bands)")


def test_window_list(bn):
    L = bn.lib
    size = C.sizeof(bn.BnWindowRef)
    refs = (bn.BnWindowRef * 2)()  # both rows name no recording
    out = (C.c_float * 16)()
    # an empty list is fine, whatever else is passed
    assert L.bn_recording_window_list(None, 0, 0, 0, None) == 0
    assert L.bn_recording_window_list(refs, 0, size, 8, out) == 0
    refused(bn, L.bn_recording_window_list(None, 1, size, 8, out), "null window list")
    refused(bn, L.bn_recording_window_list(None, 2 ** 32, 1, 6, None), "null window list")  # ... before everything else
    refused(bn, L.bn_recording_window_list(refs, 1, size - 1, 8, out), "struct_size is below sizeof(bn_window_ref)")
    refused(bn, L.bn_recording_window_list(refs, 2 ** 32, 0, 0, out), "struct_size is below sizeof(bn_window_ref)")  # ... before segment and count
    for S in (0, 6, 2 ** 32):
        refused(bn, L.bn_recording_window_list(refs, 1, size, S, out), SEGMENT)
        refused(bn, L.bn_recording_window_list(refs, 2 ** 32, size, S, out), SEGMENT)  # ... before the count
    refused(bn, L.bn_recording_window_list(refs, 2 ** 32, size, 8, out), "a window list holds fewer than 2^32 rows")
    refused(bn, L.bn_recording_window_list(refs, 2 ** 32, size, 8, None), "a window list holds fewer than 2^32 rows")
    refused(bn, L.bn_recording_window_list(refs, 2 ** 32 - 1, size, 2 ** 32 - 4, out), "count * segment_samples exceeds the address space")
    refused(bn, L.bn_recording_window_list(refs, 1, size, 8, out), "row 0: null recording")
    refused(bn, L.bn_recording_window_list(refs, 2, size, 8, None), "row 0: null recording")  # the rows before the host buffer
    # a longer struct: the rows are read at the caller's stride
    refused(bn, L.bn_recording_window_list(C.cast((C.c_uint8 * 128)(), C.POINTER(bn.BnWindowRef)), 2, 64, 8, out), "row 0: null recording")


def test_step_entry_points_without_a_context(bn):
    L = bn.lib
    refs = (bn.BnWindowRef * 1)()
    refused(bn, L.bn_infer_windows(None, None, 0, 0, 1, None, None, None, 0), "null context")
    refused(bn, L.bn_step_windows(None, None, 0, 0, 1, 0, 0, 0.0, 1), "null context")
    refused(bn, L.bn_step_window_list(None, refs, 1, C.sizeof(bn.BnWindowRef), 5, 0, 0.0, 1), "null context")
    refused(bn, L.bn_step_window_list(None, None, 0, 0, 0, 0, 0.0, 1), "null context")


def test_chunk_count(bn):
    L = bn.lib
    assert [L.bn_chunk_count(n, step) for n, step in ((0, 4), (5, 0), (8, 4), (9, 4))] == [0, 0, 2, 3]
    assert L.bn_chunk_count(0, 0) == 0 and L.bn_chunk_count(1, 2 ** 40) == 1 and L.bn_chunk_count(2 ** 40, 1) == 2 ** 40
