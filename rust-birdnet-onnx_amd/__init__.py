"""rust-birdnet-onnx_amd -- MI355X-native (gfx950 / HIP) BirdNET / Perch inference path.

Python here is a ctypes harness over the C ABI of ``libbirdnet_hip.so``
(``include/birdnet_hip.h`` = engine level, ``include/birdnet_host.h`` = the
compiled C++ mirror of the reference's ``Classifier`` API).  Nothing in this
package computes: if the shared library is missing the import fails loudly,
and if no gfx950 device is visible every load fails with ``NoDevice`` -- there
is no CPU fallback.

Names mirror the reference (tphakala/rust-birdnet-onnx ``src/lib.rs:93-108``):
``Classifier``, ``ClassifierBuilder``, ``BatchInferenceContext``,
``InferenceOptions``, ``CancellationToken``, ``ModelType``, ``ModelConfig``,
``Prediction``, ``PredictionResult``, ``Error``.
"""
from __future__ import annotations

import atexit
import ctypes as C
import weakref
import enum
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

# Several contexts in flight need hardware queues of their own: the ROCm runtime multiplexes streams onto
# GPU_MAX_HW_QUEUES (default 4) queues and the null stream takes one.  Read when the HIP runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

try:  # PyTorch, when present, must load ITS bundled HIP runtime first: the wheel's libamdhip64 and the
    # system one this library links against do not coexist in one process (torch.cuda then sees no GPU)
    import torch  # noqa: F401
except ImportError:  # the package itself needs no PyTorch
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BN_LIB") or os.path.join(_HERE, "libbirdnet_hip.so")  # BN_LIB: A/B builds of the same ABI

BN_MAX_OUTPUTS, BN_MAX_RANK, BN_NAME_LEN = 8, 6, 64
BN_CTX_DEFAULT, BN_CTX_ALL_OUTPUTS, BN_CTX_NO_GRAPH = 0, 1, 2
BN_PCM_I16, BN_PCM_F32 = 0, 1
BN_PCM_I24, BN_PCM_I32, BN_PCM_U8 = 2, 3, 4  # layout entry points only (include/birdnet_hip.h, "PCM layouts")
BN_PCM_MIX = -1  # bn_pcm_layout.channel: mix the frame down
PCM_SAMPLE_BYTES = {BN_PCM_I16: 2, BN_PCM_F32: 4, BN_PCM_I24: 3, BN_PCM_I32: 4, BN_PCM_U8: 1}
BN_ERR_MODEL_LOAD, BN_ERR_UNSUPPORTED_MODEL, BN_ERR_MODEL_DETECTION, BN_ERR_NO_DEVICE = 6, 7, 8, 9  # bn_status values the harness names

# every symbol include/birdnet_hip.h and include/birdnet_host.h declare
ENGINE_SYMBOLS = [
    "bn_abi_version", "bn_device_count", "bn_model_load", "bn_model_load_buffer", "bn_model_free",
    "bn_model_device", "bn_model_io_info", "bn_model_get_config", "bn_model_get_cost", "bn_detect_model_type", "bn_ctx_create", "bn_ctx_get_stats", "bn_ctx_input_device",
    "bn_ctx_destroy", "bn_ctx_max_batch", "bn_ctx_device_bytes", "bn_infer", "bn_infer_submit", "bn_infer_collect", "bn_infer_device",
    "bn_ctx_output_device", "bn_ctx_read_output", "bn_ctx_synchronize", "bn_ctx_stream", "bn_ctx_time_kernels", "bn_ctx_launch_costs",
    "bn_topk", "bn_topk_device", "bn_topk_host", "bn_step_device", "bn_step_results", "bn_plan_describe", "bn_model_survey", "bn_set_sharing_mode",
    "bn_recording_create", "bn_recording_create_async", "bn_recording_wait", "bn_recording_free", "bn_recording_samples", "bn_chunk_count", "bn_recording_windows",
    "bn_infer_windows", "bn_step_windows", "bn_ctx_step_device_rows", "bn_group_create", "bn_group_destroy", "bn_group_size",
    "bn_group_uses_rccl", "bn_group_get_stats", "bn_shard_range", "bn_group_analyze_recording", "bn_group_last_error", "bn_recording_create_resampled", "bn_resample_table", "bn_recording_read_f32", "bn_last_error",
    "bn_recording_create_layout", "bn_recording_create_layout_async", "bn_recording_create_layout_resampled", "bn_recording_view_channel", "bn_live_create_layout",
    "bn_recording_levels", "bn_step_window_list", "bn_recording_window_list", "bn_recording_band_levels", "bn_band_bins",
    "bn_index_create", "bn_index_free", "bn_index_size", "bn_index_dim", "bn_index_add_host", "bn_index_add_ctx", "bn_index_read",
    "bn_index_search", "bn_index_search_ids", "bn_index_assign", "bn_index_cluster",
    "bn_index_save", "bn_index_load", "bn_index_file_info", "bn_index_file_verify",
    "bn_ivf_build", "bn_ivf_free", "bn_ivf_lists", "bn_ivf_rows", "bn_ivf_extend", "bn_ivf_list_sizes", "bn_ivf_read_list", "bn_ivf_search",
    "bn_ivf_search_ids",
    "bn_sq8_build", "bn_sq8_free", "bn_sq8_rows", "bn_sq8_extend", "bn_sq8_read", "bn_sq8_search", "bn_sq8_search_ids",
    "bn_index_set_tags", "bn_index_fill_tags", "bn_index_read_tags",
    "bn_subset_select", "bn_subset_from_ids", "bn_subset_free", "bn_subset_size", "bn_subset_read", "bn_subset_search", "bn_subset_search_ids",
    "bn_index_append_rows", "bn_index_append_subset",
    "bn_index_search_peaks", "bn_index_search_peaks_ids",
    "bn_index_search_seq", "bn_index_search_seq_ids",
    "bn_index_search_above", "bn_index_search_above_ids",
    "bn_index_group_above", "bn_index_group_above_ids",
    "bn_head_create", "bn_head_free", "bn_head_dim", "bn_head_classes", "bn_head_flags", "bn_head_read", "bn_head_apply_host",
    "bn_head_fit", "bn_head_fit_index", "bn_head_rank_index", "bn_ctx_attach_head", "bn_step_head_results",
    "bn_ctx_attach_index", "bn_step_index_results", "bn_index_match",
    "bn_prior_create", "bn_prior_free", "bn_prior_sites", "bn_prior_species", "bn_prior_threshold", "bn_prior_flags", "bn_prior_read",
    "bn_prior_apply_host", "bn_ctx_attach_prior", "bn_ctx_prior_site", "bn_step_prior_results",
    "bn_track_create", "bn_track_free", "bn_track_sources", "bn_track_species", "bn_track_open_events", "bn_track_update_host",
    "bn_track_flush", "bn_track_reset", "bn_ctx_attach_track", "bn_ctx_track_source", "bn_step_track_results",
    "bn_live_create", "bn_live_free", "bn_live_push", "bn_live_push_many", "bn_live_close", "bn_live_reset", "bn_live_ready",
    "bn_live_room", "bn_live_event_count", "bn_live_read_window", "bn_step_live",
    "bn_live_create_rates", "bn_live_resampled_samples", "bn_live_source_rate",
]
HOST_SYMBOLS = [
    "bnh_classifier_build", "bnh_classifier_free", "bnh_classifier_config", "bnh_classifier_provider",
    "bnh_classifier_label_count", "bnh_classifier_label", "bnh_predict", "bnh_predict_batch",
    "bnh_create_batch_context", "bnh_create_native_batch_context", "bnh_context_read_output", "bnh_context_free", "bnh_context_max_batch_size", "bnh_context_sample_count",
    "bnh_context_input_buffer_capacity", "bnh_context_input_buffer_bytes", "bnh_context_model_type",
    "bnh_predict_batch_with_context", "bnh_predict_recording", "bnh_results_len", "bnh_result_model_type", "bnh_result_n_predictions",
    "bnh_result_species", "bnh_result_confidence", "bnh_result_index", "bnh_result_raw_scores",
    "bnh_result_embeddings", "bnh_results_free", "bnh_parse_labels", "bnh_parse_labels_format", "bnh_chunk_plan",
    "bnh_calculate_week", "bnh_validate_coordinates", "bnh_validate_date", "bnh_range_filter_build", "bnh_range_filter_free",
    "bnh_range_filter_predict", "bnh_range_filter_label", "bnh_filter_predictions",
    "bnh_range_filter_scores", "bnh_range_filter_prior_row", "bnh_prior_create", "bnh_prior_free", "bnh_prior_handle",
    "bnh_context_attach_prior", "bnh_context_set_prior_site", "bnh_context_prior_results",
    "bnh_live_create", "bnh_live_create_rates", "bnh_live_create_layout", "bnh_predict_recording_layout", "bnh_live_free", "bnh_live_push", "bnh_live_close", "bnh_live_ready", "bnh_predict_live",
    "bnh_recording_create", "bnh_recording_free", "bnh_recording_samples", "bnh_recording_levels", "bnh_predict_window_list",
    "bnh_recording_band_levels",
]


class BnIoInfo(C.Structure):
    _fields_ = [("input_rank", C.c_int32), ("input_shape", C.c_int64 * BN_MAX_RANK),
                ("input_name", C.c_char * BN_NAME_LEN), ("n_outputs", C.c_int32),
                ("output_rank", C.c_int32 * BN_MAX_OUTPUTS),
                ("output_shape", (C.c_int64 * BN_MAX_RANK) * BN_MAX_OUTPUTS),
                ("output_name", (C.c_char * BN_NAME_LEN) * BN_MAX_OUTPUTS)]


class BnModelConfig(C.Structure):
    _fields_ = [("model_type", C.c_int32), ("sample_rate", C.c_uint32), ("segment_duration", C.c_float),
                ("sample_count", C.c_uint64), ("num_species", C.c_uint64), ("has_embedding", C.c_int32),
                ("embedding_dim", C.c_uint64), ("logits_output", C.c_int32), ("embedding_output", C.c_int32)]


class BnModelCost(C.Structure):
    _fields_ = [("macs_mfma", C.c_double), ("macs_valu", C.c_double), ("weight_bytes", C.c_double),
                ("activation_bytes", C.c_double), ("n_launches", C.c_int32), ("dft_gemm_macs", C.c_double), ("fft_flops", C.c_double),
                ("dft_performed_macs", C.c_double), ("dft_fft_equiv_flops", C.c_double),
                ("recompute_macs", C.c_double)]


class BnCtxStats(C.Structure):
    _fields_ = [("captures", C.c_uint64), ("instantiates", C.c_uint64), ("replays", C.c_uint64), ("eager_runs", C.c_uint64),
                ("capture_fallbacks", C.c_uint64), ("evictions", C.c_uint64), ("cached_graphs", C.c_uint64), ("last_fallback", C.c_char * 192),
                ("input_copies", C.c_uint64)]


class BnHeadFitOpts(C.Structure):
    _fields_ = [("l2", C.c_float), ("tol", C.c_float), ("max_iters", C.c_uint32), ("flags", C.c_uint32), ("pos_weight", C.POINTER(C.c_float))]


class BnHeadFitReport(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("converged", C.c_int32), ("loss", C.c_double), ("certificate", C.c_double)]


class BnClusterOpts(C.Structure):
    _fields_ = [("max_iters", C.c_uint32), ("init_ids", C.POINTER(C.c_uint64)), ("init_centroids", C.POINTER(C.c_float)),
                ("start_ids_out", C.POINTER(C.c_uint64)), ("objective_history", C.POINTER(C.c_double)), ("history_capacity", C.c_size_t)]


class BnClusterReport(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("converged", C.c_int32), ("empty_clusters", C.c_uint32), ("moved_last", C.c_uint32),
                ("objective", C.c_double), ("history_len", C.c_uint32)]


class BnIndexFileInfo(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("valid_rows", C.c_uint64), ("dim", C.c_uint32), ("chunk_rows", C.c_uint32), ("n_chunks", C.c_uint32),
                ("version", C.c_uint32)]


class BnPcmLayout(C.Structure):
    _fields_ = [("format", C.c_int32), ("channels", C.c_uint32), ("channel", C.c_int32)]


class BnWindowLevel(C.Structure):
    _fields_ = [("peak", C.c_float), ("mean", C.c_float), ("mean_square", C.c_float), ("flags", C.c_uint32)]


class BnWindowRef(C.Structure):
    _fields_ = [("recording", C.c_void_p), ("start", C.c_uint64), ("source", C.c_int32), ("window", C.c_uint64)]


BN_LEVEL_NONFINITE, BN_LEVEL_PADDED = 1, 2  # bn_window_level.flags
BN_LEVEL_SUM_DEPTH = 1034  # include/birdnet_hip.h: the longest chain of f32 additions behind a level, for S <= 2^20
LEVEL_DTYPE = np.dtype([("peak", np.float32), ("mean", np.float32), ("mean_square", np.float32), ("flags", np.uint32)])


BN_BAND_MAX = 8  # include/birdnet_hip.h: bands per spec
BN_BAND_EPS_ULPS, BN_BAND_SUM_DEPTH = 80, 32  # the constants of the header's bound on a band level


class BnBandSpec(C.Structure):
    _fields_ = [("frame", C.c_uint32), ("hop", C.c_uint32), ("n_bands", C.c_uint32), ("bin_lo", C.c_uint32 * BN_BAND_MAX), ("bin_hi", C.c_uint32 * BN_BAND_MAX)]


class BnWindowBands(C.Structure):
    _fields_ = [("mean", C.c_float * BN_BAND_MAX), ("max", C.c_float * BN_BAND_MAX), ("total_mean", C.c_float), ("total_max", C.c_float),
                ("flags", C.c_uint32), ("n_frames", C.c_uint32)]


BAND_DTYPE = np.dtype([("mean", np.float32, (BN_BAND_MAX,)), ("max", np.float32, (BN_BAND_MAX,)), ("total_mean", np.float32), ("total_max", np.float32),
                       ("flags", np.uint32), ("n_frames", np.uint32)])


def band_spec(frame: int, hop: int, bands) -> BnBandSpec:
    """A bn_band_spec of frames of `frame` samples every `hop`, bands = [(bin_lo, bin_hi), ...]; nothing is checked here (more than
    BN_BAND_MAX bands keep their count and lose the bands past the eighth: the library refuses the count)."""
    sp = BnBandSpec(frame, hop, len(bands))
    for b, (lo, hi) in enumerate(list(bands)[:BN_BAND_MAX]):
        sp.bin_lo[b], sp.bin_hi[b] = lo, hi
    return sp


def band_bins(sample_rate: int, frame: int, lo_hz: float, hi_hz: float):
    """bn_band_bins: (bin_lo, bin_hi) of the band [lo_hz, hi_hz) for frames of `frame` samples at `sample_rate`; host only."""
    lo, hi = C.c_uint32(), C.c_uint32()
    st = lib.bn_band_bins(sample_rate, frame, lo_hz, hi_hz, C.byref(lo), C.byref(hi))
    if st:
        raise EngineError(st)
    return lo.value, hi.value


class BnIndexFilter(C.Structure):
    _fields_ = [("first_id", C.c_uint64), ("n_ids", C.c_uint64), ("tags", C.POINTER(C.c_uint32)), ("n_tags", C.c_size_t), ("flags", C.c_uint32)]


BN_INDEX_TAG_LIMIT = 65536  # row tags lie below it
BN_PEAK_RADIUS_MAX = 64  # largest peak_radius of Index.search_peaks / search_peaks_ids
BN_SEQ_LEN_MAX = 64  # largest seq_len of Index.search_seq / search_seq_ids
BN_ABOVE_MAX_HITS = 65536  # largest max_hits of Index.search_above / search_above_ids
BN_GROUP_NO_ROW = 0xFFFFFFFFFFFFFFFF  # the best / first / last id of a group without hits (Index.group_above / group_above_ids)
BN_FILTER_EXCLUDE_TAGS = 1  # bn_index_filter flag: the tag list names the tags left out
BN_CLUSTER_NONE = 0xFFFFFFFF  # the assignment of a row that belongs to no cluster
BN_HEAD_L2NORM = 1
BN_RANK_TOP, BN_RANK_UNCERTAIN = 0, 1
BN_PRIOR_UNKNOWN = -1.0  # table entry of a species the meta model does not know
BN_PRIOR_SELECT, BN_PRIOR_AFTER_TOPK, BN_PRIOR_RERANK = 0, 1, 2
BN_TRACK_PRIOR = 1  # bn_track_create flag: hits are those of admitted species, on the prior's conf'
BN_ABI_VERSION = 2  # include/birdnet_hip.h


class BnEvent(C.Structure):
    _fields_ = [("source", C.c_int32), ("species", C.c_uint32), ("first_window", C.c_uint32), ("last_window", C.c_uint32),
                ("hits", C.c_uint32), ("peak_window", C.c_uint32), ("peak_conf", C.c_float), ("mean_conf", C.c_float)]


# bn_event as a numpy record: arrays of it are what Tracker and Context.step_track_results return
EVENT_DTYPE = np.dtype([("source", np.int32), ("species", np.uint32), ("first_window", np.uint32), ("last_window", np.uint32),
                        ("hits", np.uint32), ("peak_window", np.uint32), ("peak_conf", np.float32), ("mean_conf", np.float32)])


class BnhError(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_uint64), ("expected", C.c_uint64), ("got", C.c_uint64),
                ("duration_ns", C.c_uint64), ("message", C.c_char * 512), ("latitude", C.c_float), ("longitude", C.c_float),
                ("month", C.c_uint32), ("day", C.c_uint32)]


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or `make`. "
            "This package has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    f32p, u32p, i64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    sig = {
        "bn_abi_version": (i32, []),
        "bn_device_count": (i32, []),
        "bn_model_load": (i32, [C.c_char_p, i32, i32, C.POINTER(vp)]),
        "bn_model_load_buffer": (i32, [vp, sz, i32, i32, C.POINTER(vp)]),
        "bn_model_free": (None, [vp]),
        "bn_model_device": (i32, [vp]),
        "bn_model_io_info": (i32, [vp, C.POINTER(BnIoInfo)]),
        "bn_model_get_config": (i32, [vp, C.POINTER(BnModelConfig)]),
        "bn_model_get_cost": (i32, [vp, C.POINTER(BnModelCost), sz]),
        "bn_ctx_get_stats": (i32, [vp, C.POINTER(BnCtxStats), sz]),
        "bn_ctx_input_device": (i32, [vp, C.POINTER(vp), C.POINTER(sz)]),
        "bn_detect_model_type": (i32, [i64p, sz, i64p, C.POINTER(sz), sz, i32, C.POINTER(BnModelConfig)]),
        "bn_ctx_create": (i32, [vp, sz, C.c_uint32, C.POINTER(vp)]),
        "bn_ctx_destroy": (None, [vp]),
        "bn_ctx_max_batch": (sz, [vp]),
        "bn_ctx_device_bytes": (sz, [vp]),
        "bn_infer": (i32, [vp, C.POINTER(f32p), sz, f32p, f32p, C.POINTER(C.c_int32), C.c_uint64]),
        "bn_infer_submit": (i32, [vp, C.POINTER(f32p), sz, sz, i32, C.c_float, C.POINTER(C.c_uint64)]),
        "bn_infer_collect": (i32, [vp, C.c_uint64, f32p, f32p, sz, u32p, f32p, u32p, C.POINTER(C.c_int32), C.c_uint64]),
        "bn_infer_device": (i32, [vp, vp, sz, i32]),
        "bn_ctx_output_device": (i32, [vp, i32, C.POINTER(vp), C.POINTER(sz)]),
        "bn_ctx_read_output": (i32, [vp, i32, sz, f32p]),
        "bn_ctx_synchronize": (i32, [vp]),
        "bn_ctx_stream": (vp, [vp]),
        "bn_ctx_time_kernels": (sz, [vp, sz, vp, f32p, C.POINTER(C.c_double), C.POINTER(C.c_double), sz]),
        "bn_ctx_launch_costs": (sz, [vp, sz, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), sz]),
        "bn_topk": (i32, [vp, sz, sz, i32, C.c_float, sz, u32p, f32p, u32p]),
        "bn_topk_device": (i32, [i32, vp, sz, sz, sz, i32, C.c_float, sz, u32p, f32p, u32p]),
        "bn_topk_host": (i32, [i32, f32p, sz, sz, sz, i32, C.c_float, sz, u32p, f32p, u32p]),
        "bn_step_device": (i32, [vp, vp, sz, sz, i32, C.c_float, i32]),
        "bn_step_results": (i32, [vp, C.POINTER(f32p), C.POINTER(u32p), C.POINTER(f32p), C.POINTER(u32p), C.POINTER(sz)]),
        "bn_plan_describe": (sz, [C.c_char_p, i32, i32, C.c_char_p, sz, C.POINTER(i32)]),
        "bn_model_survey": (sz, [C.c_char_p, C.c_char_p, sz, C.POINTER(i32)]),
        "bn_set_sharing_mode": (None, [i32]),
        "bn_recording_create": (i32, [i32, vp, sz, i32, C.POINTER(vp)]),
        "bn_recording_create_async": (i32, [i32, vp, sz, i32, C.POINTER(vp)]),
        "bn_recording_wait": (i32, [vp]),
        "bn_recording_free": (None, [vp]),
        "bn_recording_samples": (sz, [vp]),
        "bn_chunk_count": (sz, [sz, sz]),
        "bn_recording_windows": (i32, [vp, sz, sz, sz, sz, f32p]),
        "bn_infer_windows": (i32, [vp, vp, sz, sz, sz, f32p, f32p, C.POINTER(C.c_int32), C.c_uint64]),
        "bn_step_windows": (i32, [vp, vp, sz, sz, sz, sz, i32, C.c_float, i32]),
        "bn_recording_create_resampled": (i32, [i32, vp, sz, i32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "bn_resample_table": (sz, [C.c_uint32, C.c_uint32, C.c_uint32, f32p, sz, u32p, u32p, u32p]),
        "bn_recording_read_f32": (i32, [vp, sz, sz, f32p]),
        "bn_recording_create_layout": (i32, [i32, vp, sz, C.POINTER(BnPcmLayout), sz, C.POINTER(vp)]),
        "bn_recording_create_layout_async": (i32, [i32, vp, sz, C.POINTER(BnPcmLayout), sz, C.POINTER(vp)]),
        "bn_recording_create_layout_resampled": (i32, [i32, vp, sz, C.POINTER(BnPcmLayout), sz, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
        "bn_recording_view_channel": (i32, [vp, i32, C.POINTER(vp)]),
        "bn_recording_levels": (i32, [vp, sz, sz, sz, sz, C.POINTER(BnWindowLevel), sz]),
        "bn_step_window_list": (i32, [vp, C.POINTER(BnWindowRef), sz, sz, sz, i32, C.c_float, i32]),
        "bn_recording_band_levels": (i32, [vp, sz, sz, sz, sz, C.POINTER(BnBandSpec), sz, C.POINTER(BnWindowBands), sz]),
        "bn_band_bins": (i32, [C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
        "bn_recording_window_list": (i32, [C.POINTER(BnWindowRef), sz, sz, sz, f32p]),
        "bn_last_error": (sz, [C.c_char_p, sz]),
        "bn_ctx_step_device_rows": (i32, [vp, C.POINTER(u32p)]),
        "bn_group_create": (i32, [C.POINTER(vp), C.POINTER(C.c_int32), i32, sz, i32, C.POINTER(vp)]),
        "bn_group_destroy": (None, [vp]),
        "bn_group_size": (i32, [vp]),
        "bn_group_uses_rccl": (i32, [vp]),
        "bn_group_get_stats": (i32, [vp, C.POINTER(BnCtxStats), sz]),
        "bn_shard_range": (None, [sz, i32, i32, C.POINTER(sz), C.POINTER(sz)]),
        "bn_group_analyze_recording": (i32, [vp, vp, sz, i32, sz, sz, i32, C.c_float, f32p, sz, u32p, f32p, u32p, C.POINTER(sz)]),
        "bn_group_last_error": (sz, [C.c_char_p, sz]),
        "bn_index_create": (i32, [i32, sz, sz, C.POINTER(vp)]),
        "bn_index_free": (None, [vp]),
        "bn_index_size": (sz, [vp]),
        "bn_index_dim": (sz, [vp]),
        "bn_index_add_host": (i32, [vp, f32p, sz, C.POINTER(C.c_uint64)]),
        "bn_index_add_ctx": (i32, [vp, vp, sz, C.POINTER(C.c_uint64)]),
        "bn_index_read": (i32, [vp, C.c_uint64, sz, f32p]),
        "bn_index_search": (i32, [vp, f32p, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_search_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_assign": (i32, [vp, f32p, sz, C.c_uint64, C.c_uint64, u32p, f32p]),
        "bn_index_cluster": (i32, [vp, sz, C.c_uint64, C.c_uint64, C.POINTER(BnClusterOpts), sz, f32p, u32p, f32p, u32p, C.POINTER(BnClusterReport), sz]),
        "bn_index_save": (i32, [vp, C.c_char_p, sz]),
        "bn_index_load": (i32, [i32, C.c_char_p, sz, C.POINTER(vp)]),
        "bn_index_file_info": (i32, [C.c_char_p, C.POINTER(BnIndexFileInfo), sz]),
        "bn_index_file_verify": (i32, [C.c_char_p, C.POINTER(C.c_uint64)]),
        "bn_ivf_build": (i32, [vp, f32p, sz, C.POINTER(vp)]),
        "bn_ivf_free": (None, [vp]),
        "bn_ivf_lists": (sz, [vp]),
        "bn_ivf_rows": (sz, [vp]),
        "bn_ivf_extend": (i32, [vp]),
        "bn_ivf_list_sizes": (i32, [vp, u32p]),
        "bn_ivf_read_list": (i32, [vp, sz, C.POINTER(C.c_uint64), sz, C.POINTER(sz)]),
        "bn_ivf_search": (i32, [vp, f32p, sz, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p, u32p, C.POINTER(C.c_uint64)]),
        "bn_ivf_search_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p, u32p, C.POINTER(C.c_uint64)]),
        "bn_sq8_build": (i32, [vp, C.POINTER(vp)]),
        "bn_sq8_free": (None, [vp]),
        "bn_sq8_rows": (sz, [vp]),
        "bn_sq8_extend": (i32, [vp]),
        "bn_sq8_read": (i32, [vp, C.c_uint64, sz, C.POINTER(C.c_int8), f32p]),
        "bn_sq8_search": (i32, [vp, f32p, sz, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p, C.POINTER(C.c_uint64), u32p]),
        "bn_sq8_search_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p, C.POINTER(C.c_uint64), u32p]),
        "bn_index_set_tags": (i32, [vp, C.c_uint64, sz, u32p]),
        "bn_index_fill_tags": (i32, [vp, C.c_uint64, sz, C.c_uint32]),
        "bn_index_read_tags": (i32, [vp, C.c_uint64, sz, u32p]),
        "bn_subset_select": (i32, [vp, C.POINTER(BnIndexFilter), sz, C.POINTER(vp)]),
        "bn_subset_from_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.POINTER(vp)]),
        "bn_subset_free": (None, [vp]),
        "bn_subset_size": (sz, [vp]),
        "bn_subset_read": (i32, [vp, sz, sz, C.POINTER(C.c_uint64)]),
        "bn_subset_search": (i32, [vp, f32p, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_subset_search_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_append_rows": (i32, [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
        "bn_index_append_subset": (i32, [vp, vp, C.POINTER(C.c_uint64)]),
        "bn_index_search_peaks": (i32, [vp, f32p, sz, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_search_peaks_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_search_seq": (i32, [vp, f32p, sz, sz, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_search_seq_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, sz, C.c_int64, sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_index_search_above": (i32, [vp, f32p, sz, f32p, C.c_uint64, C.c_uint64, sz, sz, C.POINTER(C.c_uint64), f32p, u32p, u32p]),
        "bn_index_search_above_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, f32p, C.c_uint64, C.c_uint64, sz, sz, C.POINTER(C.c_uint64), f32p,
                                            u32p, u32p]),
        "bn_index_group_above": (i32, [vp, f32p, sz, f32p, C.c_uint64, C.c_uint64, sz, sz, u32p, C.POINTER(C.c_uint64), f32p, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), u32p, u32p]),
        "bn_index_group_above_ids": (i32, [vp, C.POINTER(C.c_uint64), sz, C.c_int64, f32p, C.c_uint64, C.c_uint64, sz, sz, u32p, C.POINTER(C.c_uint64), f32p,
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), u32p, u32p]),
        "bn_head_create": (i32, [i32, sz, sz, f32p, f32p, C.c_uint32, C.POINTER(vp)]),
        "bn_head_free": (None, [vp]),
        "bn_head_dim": (sz, [vp]),
        "bn_head_classes": (sz, [vp]),
        "bn_head_flags": (C.c_uint32, [vp]),
        "bn_head_read": (i32, [vp, f32p, f32p]),
        "bn_head_apply_host": (i32, [vp, f32p, sz, f32p]),
        "bn_head_fit": (i32, [i32, sz, sz, f32p, C.POINTER(C.c_uint8), sz, C.POINTER(BnHeadFitOpts), sz, C.POINTER(vp), C.POINTER(BnHeadFitReport), sz]),
        "bn_head_fit_index": (i32, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), sz, sz, C.POINTER(BnHeadFitOpts), sz, C.POINTER(vp),
                                    C.POINTER(BnHeadFitReport), sz]),
        "bn_head_rank_index": (i32, [vp, vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), sz, sz, sz, C.POINTER(C.c_uint64), f32p, u32p]),
        "bn_ctx_attach_head": (i32, [vp, vp, sz, i32, C.c_float]),
        "bn_step_head_results": (i32, [vp, C.POINTER(f32p), C.POINTER(u32p), C.POINTER(f32p), C.POINTER(u32p), C.POINTER(sz), C.POINTER(sz)]),
        "bn_ctx_attach_index": (i32, [vp, vp, sz, i32, C.c_float]),
        "bn_step_index_results": (i32, [vp, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(f32p), C.POINTER(u32p), C.POINTER(u32p), C.POINTER(sz), C.POINTER(sz)]),
        "bn_index_match": (i32, [vp, f32p, sz, sz, i32, C.c_float, sz, C.POINTER(C.c_uint64), f32p, u32p, u32p]),
        "bn_prior_create": (i32, [i32, sz, sz, f32p, C.c_float, C.c_uint32, C.POINTER(vp)]),
        "bn_prior_free": (None, [vp]),
        "bn_prior_sites": (sz, [vp]),
        "bn_prior_species": (sz, [vp]),
        "bn_prior_threshold": (C.c_float, [vp]),
        "bn_prior_flags": (C.c_uint32, [vp]),
        "bn_prior_read": (i32, [vp, sz, sz, f32p]),
        "bn_prior_apply_host": (i32, [vp, f32p, sz, C.POINTER(C.c_int32), sz, i32, C.c_float, sz, u32p, f32p, u32p]),
        "bn_ctx_attach_prior": (i32, [vp, vp, C.POINTER(C.c_int32), sz, sz, i32, C.c_float]),
        "bn_ctx_prior_site": (i32, [vp, i32]),
        "bn_step_prior_results": (i32, [vp, C.POINTER(u32p), C.POINTER(f32p), C.POINTER(u32p), C.POINTER(sz)]),
        "bn_track_create": (i32, [i32, sz, sz, C.c_float, C.c_uint32, C.c_uint32, sz, C.c_uint32, C.POINTER(vp)]),
        "bn_track_free": (None, [vp]),
        "bn_track_sources": (sz, [vp]),
        "bn_track_species": (sz, [vp]),
        "bn_track_open_events": (sz, [vp, i32]),
        "bn_track_update_host": (i32, [vp, f32p, sz, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), vp, C.POINTER(C.c_int32), C.POINTER(BnEvent), sz,
                                       C.POINTER(sz), C.POINTER(sz)]),
        "bn_track_flush": (i32, [vp, i32, C.POINTER(BnEvent), sz, C.POINTER(sz), C.POINTER(sz)]),
        "bn_track_reset": (i32, [vp, i32]),
        "bn_ctx_attach_track": (i32, [vp, vp]),
        "bn_ctx_track_source": (i32, [vp, i32]),
        "bn_step_track_results": (i32, [vp, C.POINTER(C.POINTER(BnEvent)), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
        "bn_live_create": (i32, [i32, i32, i32, sz, sz, sz, C.POINTER(vp)]),
        "bn_live_create_rates": (i32, [i32, i32, i32, sz, sz, sz, C.c_uint32, u32p, C.c_uint32, C.POINTER(vp)]),
        "bn_live_create_layout": (i32, [i32, i32, C.POINTER(BnPcmLayout), sz, sz, sz, sz, C.c_uint32, u32p, C.c_uint32, C.POINTER(vp)]),
        "bn_live_resampled_samples": (sz, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, i32]),
        "bn_live_source_rate": (C.c_uint32, [vp, i32]),
        "bn_live_free": (None, [vp]),
        "bn_live_push": (i32, [vp, i32, vp, sz]),
        "bn_live_push_many": (i32, [vp, sz, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(sz)]),
        "bn_live_close": (i32, [vp, i32]),
        "bn_live_reset": (i32, [vp, i32]),
        "bn_live_ready": (sz, [vp, i32]),
        "bn_live_room": (sz, [vp, i32]),
        "bn_live_event_count": (sz, [vp]),
        "bn_live_read_window": (i32, [vp, i32, C.c_uint64, f32p]),
        "bn_step_live": (i32, [vp, vp, sz, sz, i32, C.c_float, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(sz), i32]),
        # host mirror
        "bnh_classifier_build": (i32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), sz, i32, C.c_int64, i32,
                                       C.c_float, i32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_classifier_free": (None, [vp]),
        "bnh_classifier_config": (None, [vp, C.POINTER(BnModelConfig)]),
        "bnh_classifier_provider": (C.c_char_p, [vp]),
        "bnh_classifier_label_count": (sz, [vp]),
        "bnh_classifier_label": (C.c_char_p, [vp, sz]),
        "bnh_predict": (i32, [vp, f32p, sz, C.c_int64, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_predict_batch": (i32, [vp, C.POINTER(f32p), C.POINTER(sz), sz, C.c_int64, C.POINTER(C.c_int32),
                                    C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_create_batch_context": (i32, [vp, sz, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_create_native_batch_context": (i32, [vp, sz, i32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_context_read_output": (sz, [vp, i32, sz, f32p, sz, C.POINTER(sz), C.POINTER(BnhError)]),
        "bnh_context_free": (None, [vp]),
        "bnh_context_max_batch_size": (sz, [vp]),
        "bnh_context_sample_count": (sz, [vp]),
        "bnh_context_input_buffer_capacity": (sz, [vp]),
        "bnh_context_input_buffer_bytes": (sz, [vp]),
        "bnh_context_model_type": (i32, [vp]),
        "bnh_predict_batch_with_context": (i32, [vp, vp, C.POINTER(f32p), C.POINTER(sz), sz, C.c_int64,
                                                 C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_predict_recording": (i32, [vp, vp, vp, sz, i32, C.c_float, sz, sz, C.c_int64, C.POINTER(C.c_int32), C.POINTER(vp),
                                        f32p, sz, C.POINTER(BnhError)]),
        "bnh_predict_recording_layout": (i32, [vp, vp, vp, sz, i32, C.c_uint32, i32, C.c_float, sz, sz, C.c_int64, C.POINTER(C.c_int32), C.POINTER(vp),
                                               f32p, sz, C.POINTER(BnhError)]),
        "bnh_parse_labels_format": (sz, [C.c_char_p, i32, C.c_char_p, sz, C.POINTER(BnhError)]),
        "bnh_calculate_week": (C.c_float, [C.c_uint32, C.c_uint32]),
        "bnh_validate_coordinates": (i32, [C.c_float, C.c_float, C.POINTER(BnhError)]),
        "bnh_validate_date": (i32, [C.c_uint32, C.c_uint32, C.POINTER(BnhError)]),
        "bnh_range_filter_build": (i32, [C.c_char_p, C.c_char_p, C.POINTER(C.c_char_p), sz, C.c_float, i32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_range_filter_free": (None, [vp]),
        "bnh_range_filter_predict": (i32, [vp, C.c_float, C.c_float, C.c_uint32, C.c_uint32, u32p, f32p, sz, C.POINTER(sz), C.POINTER(BnhError)]),
        "bnh_range_filter_label": (C.c_char_p, [vp, sz]),
        "bnh_range_filter_scores": (i32, [vp, C.c_float, C.c_float, C.c_uint32, C.c_uint32, f32p, sz, C.POINTER(sz), C.POINTER(BnhError)]),
        "bnh_range_filter_prior_row": (i32, [vp, C.POINTER(C.c_char_p), sz, C.c_float, C.c_float, C.c_uint32, C.c_uint32, f32p, C.POINTER(BnhError)]),
        "bnh_prior_create": (i32, [i32, sz, sz, f32p, C.c_float, C.c_uint32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_prior_free": (None, [vp]),
        "bnh_prior_handle": (vp, [vp]),
        "bnh_context_attach_prior": (i32, [vp, vp, C.POINTER(C.c_int32), sz, sz, i32, C.c_float, C.POINTER(BnhError)]),
        "bnh_context_set_prior_site": (i32, [vp, i32, C.POINTER(BnhError)]),
        "bnh_context_prior_results": (i32, [vp, sz, u32p, f32p, sz, u32p, C.POINTER(sz), C.POINTER(BnhError)]),
        "bnh_filter_predictions": (sz, [C.POINTER(C.c_char_p), f32p, sz, C.POINTER(C.c_char_p), f32p, sz, C.c_float, i32, u32p, f32p]),
        "bnh_live_create": (i32, [vp, i32, i32, C.c_float, sz, i32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_live_create_rates": (i32, [vp, i32, u32p, i32, C.c_float, sz, i32, C.c_uint32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_live_create_layout": (i32, [vp, i32, i32, C.c_uint32, i32, u32p, C.c_float, sz, i32, C.c_uint32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_live_free": (None, [vp]),
        "bnh_live_push": (i32, [vp, i32, vp, sz, C.POINTER(BnhError)]),
        "bnh_live_close": (i32, [vp, i32, C.POINTER(BnhError)]),
        "bnh_live_ready": (sz, [vp, i32]),
        "bnh_recording_create": (i32, [vp, sz, i32, C.c_uint32, i32, i32, C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_recording_free": (None, [vp]),
        "bnh_recording_samples": (sz, [vp]),
        "bnh_recording_levels": (i32, [vp, sz, sz, sz, sz, C.POINTER(BnWindowLevel), sz, C.POINTER(sz), C.POINTER(BnhError)]),
        "bnh_recording_band_levels": (i32, [vp, sz, sz, C.POINTER(BnBandSpec), sz, sz, C.POINTER(BnWindowBands), sz, C.POINTER(sz), C.POINTER(BnhError)]),
        "bnh_predict_window_list": (i32, [vp, vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), sz, C.c_int64,
                                          C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(BnhError)]),
        "bnh_predict_live": (i32, [vp, vp, vp, sz, C.c_int64, C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint64), f32p, sz, C.POINTER(BnhError)]),
        "bnh_results_len": (sz, [vp]),
        "bnh_result_model_type": (i32, [vp, sz]),
        "bnh_result_n_predictions": (sz, [vp, sz]),
        "bnh_result_species": (C.c_char_p, [vp, sz, sz]),
        "bnh_result_confidence": (C.c_float, [vp, sz, sz]),
        "bnh_result_index": (sz, [vp, sz, sz]),
        "bnh_result_raw_scores": (sz, [vp, sz, C.POINTER(f32p)]),
        "bnh_result_embeddings": (sz, [vp, sz, C.POINTER(f32p)]),
        "bnh_results_free": (None, [vp]),
        "bnh_parse_labels": (sz, [C.c_char_p, i32, C.c_char_p, sz]),
        "bnh_chunk_plan": (sz, [sz, sz, C.c_float, C.c_uint32, C.POINTER(C.c_uint64), f32p, sz]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError => the library does not export what the headers declare
        fn.restype = res
        fn.argtypes = args
    if L.bn_abi_version() != BN_ABI_VERSION:
        raise ImportError(f"{LIB_PATH} speaks ABI {L.bn_abi_version()}, this harness was written for ABI {BN_ABI_VERSION}: rebuild (make)")
    return L


lib = _load()


def last_error() -> str:
    buf = C.create_string_buffer(2048)
    lib.bn_last_error(buf, 2048)
    return buf.value.decode("utf-8", "replace")


# ------------------------------------------------------------------ boundary types
class ModelType(enum.IntEnum):
    BirdNetV24 = 0
    BirdNetV30 = 1
    PerchV2 = 2

    def sample_rate(self) -> int:
        return 48000 if self is ModelType.BirdNetV24 else 32000

    def segment_duration(self) -> float:
        return 3.0 if self is ModelType.BirdNetV24 else 5.0

    def sample_count(self) -> int:
        return 144000 if self is ModelType.BirdNetV24 else 160000

    def has_embeddings(self) -> bool:
        return self is not ModelType.BirdNetV24


@dataclass
class ModelConfig:
    model_type: ModelType
    sample_rate: int
    segment_duration: float
    sample_count: int
    num_species: int
    embedding_dim: Optional[int]

    @staticmethod
    def _from(c: BnModelConfig) -> "ModelConfig":
        return ModelConfig(ModelType(c.model_type), c.sample_rate, c.segment_duration, c.sample_count,
                           c.num_species, c.embedding_dim if c.has_embedding else None)


@dataclass
class Prediction:
    species: str
    confidence: np.float32
    index: int


@dataclass
class PredictionResult:
    model_type: ModelType
    predictions: list
    embeddings: Optional[np.ndarray]
    raw_scores: np.ndarray


class ErrorKind(enum.IntEnum):
    InputSize = 1
    BatchInputSize = 2
    ModelDetection = 3
    LabelCount = 4
    ModelPathRequired = 5
    LabelsRequired = 6
    ModelLoad = 7
    LabelLoad = 8
    LabelParse = 9
    Inference = 10
    Timeout = 11
    Cancelled = 12
    InvalidCoordinates = 13
    InvalidDate = 14
    RangeFilterInference = 15
    Other = 16


class Error(Exception):
    """reference src/error.rs: ``kind`` is the variant, ``str()`` the Display text."""

    def __init__(self, e: BnhError):
        super().__init__(e.message.decode("utf-8", "replace"))
        self.kind = ErrorKind(e.kind)
        self.index, self.expected, self.got, self.duration_ns = e.index, e.expected, e.got, e.duration_ns
        self.latitude, self.longitude, self.month, self.day = e.latitude, e.longitude, e.month, e.day


class EngineError(RuntimeError):
    def __init__(self, status: int):
        super().__init__(f"bn_status {status}: {last_error()}")
        self.status = status


def _min_args(min_confidence: Optional[float]):
    """The (has_min, min_conf) pair of arguments the C ABI takes for an optional minimum confidence."""
    return 0 if min_confidence is None else 1, C.c_float(min_confidence or 0.0)


def _step_arrays(batch: int, k: int, ix, cf, ct, lg=None, n: int = 0):
    """Copies of the pinned results of a step: (idx [batch, k], conf [batch, k], count [batch]), behind logits [batch, n] if given."""
    rows = (np.ctypeslib.as_array(ix, shape=(batch, k)).copy(), np.ctypeslib.as_array(cf, shape=(batch, k)).copy(),
            np.ctypeslib.as_array(ct, shape=(batch,)).copy())
    return rows if lg is None else (np.ctypeslib.as_array(lg, shape=(batch, n)).copy(),) + rows


class CancellationToken:
    """reference src/inference_options.rs:24-47 (an int32 flag shared with the C ABI)."""

    def __init__(self):
        self._flag = C.c_int32(0)

    def cancel(self):
        self._flag.value = 1

    def is_cancelled(self) -> bool:
        return self._flag.value != 0


class InferenceOptions:
    """reference src/inference_options.rs:73-114; timeout in seconds (float) or None."""

    def __init__(self, timeout: Optional[float] = None, cancellation_token: Optional[CancellationToken] = None):
        self.timeout = timeout
        self.cancellation_token = cancellation_token

    @staticmethod
    def with_timeout_of(seconds: float) -> "InferenceOptions":
        return InferenceOptions(timeout=seconds)

    def with_timeout(self, seconds: float) -> "InferenceOptions":
        self.timeout = seconds
        return self

    def with_cancellation_token(self, token: CancellationToken) -> "InferenceOptions":
        self.cancellation_token = token
        return self

    def needs_monitor(self) -> bool:
        return self.timeout is not None or self.cancellation_token is not None

    def _raw(self):
        t = -1 if self.timeout is None else int(round(self.timeout * 1e9))
        c = None if self.cancellation_token is None else C.byref(self.cancellation_token._flag)
        return C.c_int64(t), c


def _segments_arg(segments: Sequence[np.ndarray]):
    arrs = [np.ascontiguousarray(s, dtype=np.float32) for s in segments]
    n = len(arrs)
    f32p = C.POINTER(C.c_float)
    ptrs = (f32p * max(n, 1))(*[a.ctypes.data_as(f32p) for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.shape[0] for a in arrs])
    return arrs, ptrs, lens, n


def _collect(res: C.c_void_p) -> list:
    out = []
    try:
        for i in range(lib.bnh_results_len(res)):
            preds = [Prediction(lib.bnh_result_species(res, i, j).decode("utf-8"),
                                np.float32(lib.bnh_result_confidence(res, i, j)), lib.bnh_result_index(res, i, j))
                     for j in range(lib.bnh_result_n_predictions(res, i))]
            p = C.POINTER(C.c_float)()
            n = lib.bnh_result_raw_scores(res, i, C.byref(p))
            raw = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.float32)
            n = lib.bnh_result_embeddings(res, i, C.byref(p))
            emb = np.ctypeslib.as_array(p, shape=(n,)).copy() if n else None
            out.append(PredictionResult(ModelType(lib.bnh_result_model_type(res, i)), preds, emb, raw))
    finally:
        lib.bnh_results_free(res)
    return out


class BatchInferenceContext:
    """reference src/batch_context.rs:70-165."""

    def __init__(self, handle):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None):
            lib.bnh_context_free(self._h)
            self._h = None

    def max_batch_size(self) -> int:
        return lib.bnh_context_max_batch_size(self._h)

    def sample_count(self) -> int:
        return lib.bnh_context_sample_count(self._h)

    def input_buffer_capacity(self) -> int:
        return lib.bnh_context_input_buffer_capacity(self._h)

    def input_buffer_bytes(self) -> int:
        return lib.bnh_context_input_buffer_bytes(self._h)

    def model_type(self) -> ModelType:
        return ModelType(lib.bnh_context_model_type(self._h))

    def read_output(self, index: int, batch: int) -> np.ndarray:
        """Native extension: graph output `index` of the last batch as [batch, row_elems] (contexts made with
        create_native_batch_context(all_outputs=True) also hold the outputs the reference discards)."""
        err, row = BnhError(), C.c_size_t()
        need = lib.bnh_context_read_output(self._h, index, batch, None, 0, C.byref(row), C.byref(err))
        if err.kind:
            raise Error(err)
        out = np.zeros(need, dtype=np.float32)
        lib.bnh_context_read_output(self._h, index, batch, out.ctypes.data_as(C.POINTER(C.c_float)), need, C.byref(row), C.byref(err))
        if err.kind:
            raise Error(err)
        return out.reshape(batch, row.value)


class Classifier:
    """reference src/classifier.rs:436-867, backed by the compiled C++ mirror."""

    def __init__(self, handle):
        self._h = handle
        cfg = BnModelConfig()
        lib.bnh_classifier_config(handle, C.byref(cfg))
        self._config = ModelConfig._from(cfg)

    def __del__(self):
        if getattr(self, "_h", None):
            lib.bnh_classifier_free(self._h)
            self._h = None

    @staticmethod
    def builder() -> "ClassifierBuilder":
        return ClassifierBuilder()

    def config(self) -> ModelConfig:
        return self._config

    def labels(self) -> list:
        return [lib.bnh_classifier_label(self._h, i).decode("utf-8") for i in range(lib.bnh_classifier_label_count(self._h))]

    def requested_provider(self) -> str:
        return lib.bnh_classifier_provider(self._h).decode()

    def predict(self, segment, options: Optional[InferenceOptions] = None) -> PredictionResult:
        options = options or InferenceOptions()
        a = np.ascontiguousarray(segment, dtype=np.float32)
        t, c = options._raw()
        res, err = C.c_void_p(), BnhError()
        if lib.bnh_predict(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], t, c, C.byref(res), C.byref(err)):
            raise Error(err)
        return _collect(res)[0]

    def predict_batch(self, segments, options: Optional[InferenceOptions] = None) -> list:
        options = options or InferenceOptions()
        arrs, ptrs, lens, n = _segments_arg(segments)
        t, c = options._raw()
        res, err = C.c_void_p(), BnhError()
        if lib.bnh_predict_batch(self._h, ptrs, lens, n, t, c, C.byref(res), C.byref(err)):
            raise Error(err)
        return _collect(res)

    def create_batch_context(self, max_batch_size: int) -> BatchInferenceContext:
        h, err = C.c_void_p(), BnhError()
        if lib.bnh_create_batch_context(self._h, max_batch_size, C.byref(h), C.byref(err)):
            raise Error(err)
        return BatchInferenceContext(h)

    def create_native_batch_context(self, max_batch_size: int, all_outputs: bool = False) -> BatchInferenceContext:
        """Native extension: a batch context for every model family, Perch included (the reference refuses it)."""
        h, err = C.c_void_p(), BnhError()
        if lib.bnh_create_native_batch_context(self._h, max_batch_size, 1 if all_outputs else 0, C.byref(h), C.byref(err)):
            raise Error(err)
        return BatchInferenceContext(h)

    def predict_batch_with_context(self, context: BatchInferenceContext, segments,
                                   options: Optional[InferenceOptions] = None) -> list:
        options = options or InferenceOptions()
        arrs, ptrs, lens, n = _segments_arg(segments)
        t, c = options._raw()
        res, err = C.c_void_p(), BnhError()
        if lib.bnh_predict_batch_with_context(self._h, context._h, ptrs, lens, n, t, c, C.byref(res), C.byref(err)):
            raise Error(err)
        return _collect(res)


    def predict_recording(self, context: BatchInferenceContext, samples: np.ndarray, overlap_secs: float = 0.0, first_chunk: int = 0,
                          count: Optional[int] = None, options: Optional[InferenceOptions] = None) -> list:
        """The reference CLI's read_wav + chunk_audio + batch loop (src/bin/birdnet-analyze.rs:556-600, 683-743) on a mono
        int16 / float32 recording: uploaded once, windows cut on the device.  Returns [(start_time, PredictionResult)]."""
        options = options or InferenceOptions()
        a = np.ascontiguousarray(samples)
        if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
            raise ValueError("mono int16 or float32 samples expected")
        t, c = options._raw()
        res, err = C.c_void_p(), BnhError()
        cap = 1 << 20
        times = np.zeros(cap, dtype=np.float32)
        if lib.bnh_predict_recording(self._h, context._h, a.ctypes.data_as(C.c_void_p), a.shape[0], 0 if a.dtype == np.int16 else 1,
                                     C.c_float(overlap_secs), first_chunk, (1 << 64) - 1 if count is None else count, t, c, C.byref(res),
                                     times.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(err)):
            raise Error(err)
        results = _collect(res)
        return list(zip(times[:len(results)].tolist(), results))

    def predict_live(self, context: BatchInferenceContext, live: "LiveSources", max_windows: int,
                     options: Optional[InferenceOptions] = None) -> list:
        """Classifier::predict_live: up to max_windows ready windows of all live sources, oldest first, as one batch.
        Returns [(source, chunk, start_time, PredictionResult)]."""
        options = options or InferenceOptions()
        t, c = options._raw()
        res, err = C.c_void_p(), BnhError()
        cap = max(max_windows, 1)
        src, chunk, times = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.float32)
        if lib.bnh_predict_live(self._h, context._h, live._h, max_windows, t, c, C.byref(res), src.ctypes.data_as(C.POINTER(C.c_int32)),
                                chunk.ctypes.data_as(C.POINTER(C.c_uint64)), times.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(err)):
            raise Error(err)
        results = _collect(res)
        return [(int(src[i]), int(chunk[i]), float(times[i]), r) for i, r in enumerate(results)]

    def predict_window_list(self, context: BatchInferenceContext, refs, options: Optional[InferenceOptions] = None) -> list:
        """Classifier::predict_window_list: one batch over an explicit list of (HostRecording, start[, source[, window]]) rows;
        result i is row i."""
        options = options or InferenceOptions()
        t, c = options._raw()
        rows = [tuple(r) for r in refs]
        n = len(rows)
        recs = (C.c_void_p * max(n, 1))(*[None if r[0] is None else r[0]._h for r in rows])
        starts = np.array([int(r[1]) for r in rows], dtype=np.uint64)
        sources = np.array([int(r[2]) if len(r) > 2 else 0 for r in rows], dtype=np.int32)
        windows = np.array([int(r[3]) if len(r) > 3 else i for i, r in enumerate(rows)], dtype=np.uint64)
        res, err = C.c_void_p(), BnhError()
        if lib.bnh_predict_window_list(self._h, context._h, recs, starts.ctypes.data_as(C.POINTER(C.c_uint64)), sources.ctypes.data_as(C.POINTER(C.c_int32)),
                                       windows.ctypes.data_as(C.POINTER(C.c_uint64)), n, t, c, C.byref(res), C.byref(err)):
            raise Error(err)
        return _collect(res)


class HostRecording:
    """birdnet::Recording through the host mirror: interleaved frames in any format uploaded once (format / channels / channel are a
    bn_pcm_layout's fields), for levels() and Classifier.predict_window_list."""

    def __init__(self, pcm, fmt: int = BN_PCM_I16, channels: int = 1, channel: int = 0, device: int = 0):
        a = np.frombuffer(pcm, dtype=np.uint8) if isinstance(pcm, (bytes, bytearray, memoryview)) else np.ascontiguousarray(pcm).reshape(-1).view(np.uint8)
        fb = PCM_SAMPLE_BYTES.get(fmt, 1) * max(int(channels), 1)
        if a.shape[0] % fb:
            raise ValueError(f"{a.shape[0]} bytes are no whole number of {fb}-byte frames")
        h, err = C.c_void_p(), BnhError()
        if lib.bnh_recording_create(a.ctypes.data_as(C.c_void_p), a.shape[0] // fb, fmt, channels, channel, device, C.byref(h), C.byref(err)):
            raise Error(err)
        self._h = h
        self.n_samples = int(lib.bnh_recording_samples(h))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bnh_recording_free(self._h)
            self._h = None

    def levels(self, segment_samples: int, step_samples: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Recording::levels: a LEVEL_DTYPE array of windows [first, first + count) (count None: to the last window)."""
        want = (1 << 64) - 1 if count is None else count
        cap = max(int(lib.bn_chunk_count(self.n_samples, step_samples)) if step_samples else 0, 0 if count is None else count, 1)
        out = np.zeros(cap, dtype=LEVEL_DTYPE)
        n, err = C.c_size_t(), BnhError()
        if lib.bnh_recording_levels(self._h, segment_samples, step_samples, first, want, out.ctypes.data_as(C.POINTER(BnWindowLevel)), cap, C.byref(n),
                                    C.byref(err)):
            raise Error(err)
        return out[:n.value].copy()

    def band_levels(self, segment_samples: int, step_samples: int, frame: int, hop: int, bands, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Recording::band_levels: a BAND_DTYPE array of windows [first, first + count) (count None: to the last window); bands =
        [(bin_lo, bin_hi), ...]."""
        want = (1 << 64) - 1 if count is None else count
        cap = max(int(lib.bn_chunk_count(self.n_samples, step_samples)) if step_samples else 0, 0 if count is None else count, 1)
        out = np.zeros(cap, dtype=BAND_DTYPE)
        n, err = C.c_size_t(), BnhError()
        sp = band_spec(frame, hop, bands)
        if lib.bnh_recording_band_levels(self._h, segment_samples, step_samples, C.byref(sp), first, want, out.ctypes.data_as(C.POINTER(BnWindowBands)), cap,
                                         C.byref(n), C.byref(err)):
            raise Error(err)
        return out[:n.value].copy()


class LiveSources:
    """birdnet::LiveSources: live pools through the host mirror (windows of the classifier's segment length, chunk_audio's step
    for the given overlap; ring_samples 0 => 2 * segment + step; device < 0 => the classifier's).  source_rates (one rate in Hz
    per source, len == n_sources) makes it a resampling pool: pushes arrive at those rates and are converted on the device to the
    classifier's sample rate (bn_live_create_rates); start times stay in the classifier's rate."""

    def __init__(self, classifier: Classifier, n_sources: int, fmt: int = BN_PCM_I16, overlap_secs: float = 0.0, ring_samples: int = 0,
                 device: int = -1, source_rates=None, zero_crossings: int = 0):
        h, err = C.c_void_p(), BnhError()
        if source_rates is None:
            st = lib.bnh_live_create(classifier._h, n_sources, fmt, C.c_float(overlap_secs), ring_samples, device, C.byref(h), C.byref(err))
        else:
            rates = np.ascontiguousarray(source_rates, dtype=np.uint32).reshape(-1)
            if rates.shape[0] != n_sources:
                raise ValueError("source_rates needs one rate per source")
            st = lib.bnh_live_create_rates(classifier._h, n_sources, rates.ctypes.data_as(C.POINTER(C.c_uint32)), fmt, C.c_float(overlap_secs),
                                           ring_samples, device, zero_crossings, C.byref(h), C.byref(err))
        if st:
            raise Error(err)
        self._h, self._dtype = h, (np.int16 if fmt == BN_PCM_I16 else np.float32)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bnh_live_free(self._h)
            self._h = None

    def push(self, source: int, samples):
        a = np.ascontiguousarray(samples, dtype=self._dtype).reshape(-1)
        err = BnhError()
        if lib.bnh_live_push(self._h, source, a.ctypes.data_as(C.c_void_p), a.shape[0], C.byref(err)):
            raise Error(err)

    def close(self, source: int):
        err = BnhError()
        if lib.bnh_live_close(self._h, source, C.byref(err)):
            raise Error(err)

    def ready(self, source: int = -1) -> int:
        return int(lib.bnh_live_ready(self._h, source))


class ClassifierBuilder:
    """reference src/classifier.rs:46-383."""

    def __init__(self):
        self._model_path = None
        self._labels_path = None
        self._labels = None
        self._model_type = -1
        self._top_k = 10
        self._min_conf = None
        self._device = 0

    def model_path(self, p: str):
        self._model_path = p
        return self

    def labels_path(self, p: str):
        self._labels_path, self._labels = p, None
        return self

    def labels(self, l: Sequence[str]):
        self._labels, self._labels_path = list(l), None
        return self

    def model_type(self, t: ModelType):
        self._model_type = int(t)
        return self

    def top_k(self, k: int):
        self._top_k = k
        return self

    def min_confidence(self, c: float):
        self._min_conf = c
        return self

    def with_rocm(self, device: int = 0):
        self._device = device
        return self

    def build(self) -> Classifier:
        h, err = C.c_void_p(), BnhError()
        labs = None
        n = 0
        if self._labels is not None:
            n = len(self._labels)
            labs = (C.c_char_p * max(n, 1))(*[s.encode("utf-8") for s in self._labels])
        top_k = self._top_k if self._top_k < 2 ** 63 else -1
        rc = lib.bnh_classifier_build(None if self._model_path is None else self._model_path.encode(),
                                      None if self._labels_path is None else self._labels_path.encode(), labs, n,
                                      self._model_type, top_k, 0 if self._min_conf is None else 1,
                                      C.c_float(self._min_conf or 0.0), self._device, C.byref(h), C.byref(err))
        if rc:
            raise Error(err)
        return Classifier(h)


# ------------------------------------------------------------------ engine-level wrappers (bench / tests)
class Model:
    """bn_model: what the Rust shim would hold in place of ort::Session."""

    def __init__(self, path: str, device: int = 0, model_type: int = -1):
        h = C.c_void_p()
        st = lib.bn_model_load(path.encode(), device, model_type, C.byref(h))
        if st:
            raise EngineError(st)
        self._h = h
        cfg = BnModelConfig()
        lib.bn_model_get_config(h, C.byref(cfg))
        self.config = cfg
        self.device = device

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # lib is gone at interpreter shutdown
            lib.bn_model_free(self._h)
            self._h = None

    def io_info(self) -> BnIoInfo:
        io = BnIoInfo()
        lib.bn_model_io_info(self._h, C.byref(io))
        return io

    def cost(self) -> BnModelCost:
        c = BnModelCost()
        lib.bn_model_get_cost(self._h, C.byref(c), C.sizeof(c))
        return c


class Context:
    """bn_ctx: buffers + stream for one in-flight batch."""

    def __init__(self, model: Model, max_batch: int, flags: int = BN_CTX_DEFAULT):
        h = C.c_void_p()
        st = lib.bn_ctx_create(model._h, max_batch, flags, C.byref(h))
        if st:
            raise EngineError(st)
        self._h, self.model, self.max_batch = h, model, max_batch

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_ctx_destroy(self._h)
            self._h = None

    def close(self):
        """Drain the context's stream and destroy it now (instead of whenever the object is collected).  Anything that wraps
        `stream()` -- torch.cuda.ExternalStream, events recorded on it, tensors copied on it -- must be released first; never
        `tensor.record_stream()` a context's stream: the allocator would record an event on it when the tensor is freed, possibly
        after bn_ctx_destroy has destroyed the hipStream_t (round 3's SIGSEGV)."""
        self.__del__()

    def input_device(self):
        """(device pointer, capacity in floats) of the context's own input buffer: a batch written here runs without a copy."""
        p, n = C.c_void_p(), C.c_size_t()
        st = lib.bn_ctx_input_device(self._h, C.byref(p), C.byref(n))
        if st:
            raise EngineError(st)
        return p.value, n.value

    def stats(self) -> dict:
        """bn_ctx_get_stats: captures / instantiates / replays / eager runs / capture fallbacks (must be 0) of this context."""
        st = BnCtxStats()
        r = lib.bn_ctx_get_stats(self._h, C.byref(st), C.sizeof(st))
        if r:
            raise EngineError(r)
        d = {k: int(getattr(st, k)) for k, _ in BnCtxStats._fields_ if k != "last_fallback"}
        d["last_fallback"] = st.last_fallback.decode(errors="replace")
        return d

    def infer(self, segments: np.ndarray, want_embeddings: bool = True, timeout_ns: int = 0, cancel=None):
        x = np.ascontiguousarray(segments, dtype=np.float32)
        b = x.shape[0]
        cfg = self.model.config
        f32p = C.POINTER(C.c_float)
        ptrs = (f32p * max(b, 1))(*[x[i].ctypes.data_as(f32p) for i in range(b)])
        logits = np.empty((b, self.output_device(cfg.logits_output)[1]), dtype=np.float32)
        emb = None
        if cfg.has_embedding and want_embeddings:
            emb = np.empty((b, self.output_device(cfg.embedding_output)[1]), dtype=np.float32)
        st = lib.bn_infer(self._h, ptrs, b, logits.ctypes.data_as(f32p),
                          None if emb is None else emb.ctypes.data_as(f32p), cancel, timeout_ns)
        if st:
            raise EngineError(st)
        return logits, emb

    def submit(self, segments, top_k: int = 0, min_confidence: Optional[float] = None) -> int:
        """bn_infer_submit: stage + upload + enqueue one batch of host segments ([b, S] array or a list of 1-D
        arrays); returns a ticket for collect().  At most two tickets may be outstanding per context."""
        f32p = C.POINTER(C.c_float)
        if isinstance(segments, np.ndarray):
            x = np.ascontiguousarray(segments, dtype=np.float32)
            rows = [x[i] for i in range(x.shape[0])]
        else:
            rows = [np.ascontiguousarray(r, dtype=np.float32) for r in segments]
        b = len(rows)
        ptrs = (f32p * max(b, 1))(*[r.ctypes.data_as(f32p) for r in rows])
        t = C.c_uint64(0)
        st = lib.bn_infer_submit(self._h, ptrs, b, top_k, *_min_args(min_confidence), C.byref(t))
        if st:
            raise EngineError(st)
        self._tickets = getattr(self, "_tickets", {})
        self._tickets[t.value] = (b, min(top_k, self.output_device(self.model.config.logits_output)[1]))
        return t.value

    def collect(self, ticket: int, want_embeddings: bool = True, timeout_ns: int = 0, cancel=None):
        """bn_infer_collect: (logits, embeddings or None, idx, conf, count) of a submitted batch (the top-K arrays
        are None when it was submitted with top_k = 0)."""
        f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        b, k = self._tickets.pop(ticket, (0, 0))
        cfg = self.model.config
        logits = np.empty((b, self.output_device(cfg.logits_output)[1]), dtype=np.float32)
        emb = None
        if cfg.has_embedding and want_embeddings:
            emb = np.empty((b, self.output_device(cfg.embedding_output)[1]), dtype=np.float32)
        idx = conf = cnt = None
        if k:
            idx, conf, cnt = np.zeros((b, k), dtype=np.uint32), np.zeros((b, k), dtype=np.float32), np.zeros(b, dtype=np.uint32)
        st = lib.bn_infer_collect(self._h, ticket, logits.ctypes.data_as(f32p), None if emb is None else emb.ctypes.data_as(f32p), k,
                                  None if idx is None else idx.ctypes.data_as(u32p), None if conf is None else conf.ctypes.data_as(f32p),
                                  None if cnt is None else cnt.ctypes.data_as(u32p), cancel, timeout_ns)
        if st:
            raise EngineError(st)
        return logits, emb, idx, conf, cnt

    def infer_device(self, d_ptr: int, batch: int, sync: bool = False):
        st = lib.bn_infer_device(self._h, C.c_void_p(d_ptr), batch, 1 if sync else 0)
        if st:
            raise EngineError(st)

    def step_device(self, d_ptr: int, batch: int, top_k: int = 10, min_confidence: Optional[float] = None,
                    sync: bool = False):
        """One whole hot-path pass (plan + top-K + D2H of logits / top-K) on a device-resident batch."""
        st = lib.bn_step_device(self._h, C.c_void_p(d_ptr), batch, top_k, *_min_args(min_confidence), 1 if sync else 0)
        if st:
            raise EngineError(st)

    def step_results(self, batch: int):
        lg, ix, cf, ct = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
        ks = C.c_size_t()
        st = lib.bn_step_results(self._h, C.byref(lg), C.byref(ix), C.byref(cf), C.byref(ct), C.byref(ks))
        if st:
            raise EngineError(st)
        return _step_arrays(batch, ks.value, ix, cf, ct, lg, self.output_device(self.model.config.logits_output)[1])

    def synchronize(self):
        st = lib.bn_ctx_synchronize(self._h)
        if st:
            raise EngineError(st)

    def output_device(self, index: int):
        p, n = C.c_void_p(), C.c_size_t()
        st = lib.bn_ctx_output_device(self._h, index, C.byref(p), C.byref(n))
        if st:
            raise EngineError(st)
        return p.value, n.value

    def read_output(self, index: int, batch: int) -> np.ndarray:
        _, n = self.output_device(index)
        out = np.empty((batch, n), dtype=np.float32)
        st = lib.bn_ctx_read_output(self._h, index, batch, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out

    def topk(self, batch: int, top_k: int, min_confidence: Optional[float] = None):
        n = self.model.config.num_species
        k = max(min(top_k, n), 1)
        idx = np.zeros((batch, k), dtype=np.uint32)
        conf = np.zeros((batch, k), dtype=np.float32)
        cnt = np.zeros(batch, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        st = lib.bn_topk(self._h, batch, top_k, *_min_args(min_confidence), k, idx.ctypes.data_as(u32p),
                         conf.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(u32p))
        if st:
            raise EngineError(st)
        return idx, conf, cnt

    def infer_windows(self, rec: "Recording", step_samples: int, first: int, count: int, want_embeddings: bool = True,
                      timeout_ns: int = 0, cancel=None):
        """bn_infer_windows: windows [first, first+count) of an uploaded recording -> (logits, embeddings)."""
        cfg = self.model.config
        f32p = C.POINTER(C.c_float)
        logits = np.empty((count, self.output_device(cfg.logits_output)[1]), dtype=np.float32)
        emb = None
        if cfg.has_embedding and want_embeddings:
            emb = np.empty((count, self.output_device(cfg.embedding_output)[1]), dtype=np.float32)
        st = lib.bn_infer_windows(self._h, rec._h, step_samples, first, count, logits.ctypes.data_as(f32p),
                                  None if emb is None else emb.ctypes.data_as(f32p), cancel, timeout_ns)
        if st:
            raise EngineError(st)
        return logits, emb

    def step_windows(self, rec: "Recording", step_samples: int, first: int, count: int, top_k: int = 10,
                     min_confidence: Optional[float] = None, sync: bool = False):
        """bn_step_windows: one asynchronous hot-path pass over windows of an uploaded recording."""
        st = lib.bn_step_windows(self._h, rec._h, step_samples, first, count, top_k, *_min_args(min_confidence), 1 if sync else 0)
        if st:
            raise EngineError(st)

    def step_window_list(self, refs, top_k: int = 10, min_confidence: Optional[float] = None, sync: bool = False):
        """bn_step_window_list: one hot-path pass over an explicit list of windows.  refs: (recording, start[, source[, window]]) per
        row -- the S frames of `recording` from frame `start`, reported to an attached prior / tracker as window `window` of `source`
        (defaults 0 and the row's position).  Results through step_results(len(refs)) and the other step_*_results."""
        arr, keep = window_refs(refs)
        st = lib.bn_step_window_list(self._h, arr, len(keep), C.sizeof(BnWindowRef), top_k, *_min_args(min_confidence), 1 if sync else 0)
        if st:
            raise EngineError(st)

    def step_live(self, live: "Live", max_windows: int, top_k: int = 10, min_confidence: Optional[float] = None,
                  sync: bool = False):
        """bn_step_live: up to max_windows ready windows of a live pool through the hot path; returns (sources, windows) of the
        rows taken (empty: nothing ran).  Results through step_results(len(sources))."""
        src = np.zeros(max(max_windows, 1), dtype=np.int32)
        win = np.zeros(max(max_windows, 1), dtype=np.uint64)
        n = C.c_size_t()
        st = lib.bn_step_live(self._h, live._h, max_windows, top_k, *_min_args(min_confidence),
                              src.ctypes.data_as(C.POINTER(C.c_int32)), win.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n), 1 if sync else 0)
        if st:
            raise EngineError(st)
        return src[:n.value].copy(), win[:n.value].copy()

    def attach_prior(self, prior: Optional["Prior"], source_sites=None, top_k: int = 10, min_confidence: Optional[float] = None):
        """bn_ctx_attach_prior: every later step of this context also produces that step's prior-filtered top-K rows (None
        detaches).  source_sites: the site of every source of the live pools this context steps; without it, and in step_device /
        step_windows, every row is at the context's site (set_prior_site, 0 after every attach)."""
        m = None if source_sites is None else np.ascontiguousarray(source_sites, dtype=np.int32).reshape(-1)
        st = lib.bn_ctx_attach_prior(self._h, None if prior is None else prior._h, None if m is None else m.ctypes.data_as(C.POINTER(C.c_int32)),
                                     0 if m is None else m.shape[0], top_k, *_min_args(min_confidence))
        if st:
            raise EngineError(st)
        self._prior = prior

    def set_prior_site(self, site: int):
        """bn_ctx_prior_site: the site of every row of step_device / step_windows."""
        st = lib.bn_ctx_prior_site(self._h, site)
        if st:
            raise EngineError(st)

    def step_prior_results(self, batch: int):
        """(idx [batch, k], conf [batch, k], count [batch]) of the last step's prior-filtered rows, after synchronize()."""
        ix, cf, ct, ks = C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.c_size_t()
        st = lib.bn_step_prior_results(self._h, C.byref(ix), C.byref(cf), C.byref(ct), C.byref(ks))
        if st:
            raise EngineError(st)
        return _step_arrays(batch, ks.value, ix, cf, ct)

    def attach_track(self, tracker: Optional["Tracker"]):
        """bn_ctx_attach_track: every later step_windows / step_live of this context also updates the tracker with that step's rows
        (None detaches).  Rows of step_windows are windows first + i of the context's source (set_track_source, 0 after every attach);
        rows of step_live carry their own source and window."""
        st = lib.bn_ctx_attach_track(self._h, None if tracker is None else tracker._h)
        if st:
            raise EngineError(st)
        self._track = tracker

    def set_track_source(self, source: int):
        """bn_ctx_track_source: the source of every row of step_windows."""
        st = lib.bn_ctx_track_source(self._h, source)
        if st:
            raise EngineError(st)

    def step_track_results(self):
        """(events, dropped, stale_rows) of the last tracked step, after synchronize(): the events that step closed as an EVENT_DTYPE
        array sorted by (source, species, first_window), the number lost to the tracker's max_events, and the live rows skipped
        because their window did not exceed their source's last."""
        ev, n, dr, stale = C.POINTER(BnEvent)(), C.c_size_t(), C.c_size_t(), C.c_size_t()
        st = lib.bn_step_track_results(self._h, C.byref(ev), C.byref(n), C.byref(dr), C.byref(stale))
        if st:
            raise EngineError(st)
        out = np.empty(n.value, dtype=EVENT_DTYPE)
        if n.value:
            C.memmove(out.ctypes.data, ev, n.value * C.sizeof(BnEvent))
        return out, int(dr.value), int(stale.value)

    def attach_head(self, head: Optional["Head"], top_k: int = 10, min_confidence: Optional[float] = None):
        """bn_ctx_attach_head: every later step of this context also runs `head` on the step's embedding rows (None detaches)."""
        st = lib.bn_ctx_attach_head(self._h, None if head is None else head._h, top_k, *_min_args(min_confidence))
        if st:
            raise EngineError(st)
        self._head = head

    def step_head_results(self, batch: int):
        """(head logits [batch, n_classes], idx, conf, count) of the last step, after synchronize()."""
        lg, ix, cf, ct = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)()
        ks, nc = C.c_size_t(), C.c_size_t()
        st = lib.bn_step_head_results(self._h, C.byref(lg), C.byref(ix), C.byref(cf), C.byref(ct), C.byref(ks), C.byref(nc))
        if st:
            raise EngineError(st)
        return _step_arrays(batch, ks.value, ix, cf, ct, lg, nc.value)

    def attach_index(self, index: Optional["Index"], top_m: int = 10, min_score: Optional[float] = None):
        """bn_ctx_attach_index: every later step of this context also matches the step's embedding rows against the rows `index`
        holds now (None detaches); with min_score only rows scoring at least that much are returned."""
        st = lib.bn_ctx_attach_index(self._h, None if index is None else index._h, top_m, *_min_args(min_score))
        if st:
            raise EngineError(st)
        self._index = index

    def step_index_results(self, batch: int):
        """(ids [batch, top_m] uint64, scores [batch, top_m] float32, tags [batch, top_m] uint32, counts [batch] uint32,
        rows_searched) of the last step's match, after synchronize(); entries past counts[i] are as Index.search leaves them (id 0,
        score NaN, tag 0)."""
        ip, sp, tp, cp = C.POINTER(C.c_uint64)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        ms, ns = C.c_size_t(), C.c_size_t()
        st = lib.bn_step_index_results(self._h, C.byref(ip), C.byref(sp), C.byref(tp), C.byref(cp), C.byref(ms), C.byref(ns))
        if st:
            raise EngineError(st)
        m = ms.value
        counts = np.ctypeslib.as_array(cp, (batch,)).copy()
        ids = np.ctypeslib.as_array(ip, (batch, m)).copy()
        scores = np.ctypeslib.as_array(sp, (batch, m)).copy()
        tags = np.ctypeslib.as_array(tp, (batch, m)).copy()
        past = np.arange(m)[None, :] >= counts[:, None]
        ids[past], scores[past], tags[past] = 0, np.nan, 0
        return ids, scores, tags, counts, int(ns.value)

    def time_kernels(self, batch: int):
        cap = 1024
        names = C.create_string_buffer(cap * BN_NAME_LEN)
        usec = (C.c_float * cap)()
        macs = (C.c_double * cap)()
        byts = (C.c_double * cap)()
        n = lib.bn_ctx_time_kernels(self._h, batch, C.cast(names, C.c_void_p), usec, macs, byts, cap)
        out = []
        for i in range(min(n, cap)):
            nm = names.raw[i * BN_NAME_LEN:(i + 1) * BN_NAME_LEN].split(b"\0", 1)[0].decode()
            out.append((nm, float(usec[i]), float(macs[i]), float(byts[i])))
        return out

    def launch_costs(self, batch: int):
        """Per launch: (macs on the matrix cores, macs on the vector ALU, recompute share of the first, algorithmic bytes)."""
        cap = 1024
        a, b, r, by = ((C.c_double * cap)() for _ in range(4))
        n = lib.bn_ctx_launch_costs(self._h, batch, a, b, r, by, cap)
        return [(float(a[i]), float(b[i]), float(r[i]), float(by[i])) for i in range(min(n, cap))]

    def stream(self) -> int:
        return lib.bn_ctx_stream(self._h) or 0


_pending_uploads = weakref.WeakSet()


def _join_uploads():
    for r in list(_pending_uploads):
        try:
            if getattr(r, "_h", None):
                lib.bn_recording_wait(r._h)
        except Exception:  # noqa: BLE001 -- exit path
            pass


atexit.register(_join_uploads)


def window_refs(refs):
    """A bn_window_ref array of (recording, start[, source[, window]]) rows, and the recordings it points at (keep them alive as long
    as the array is used)."""
    rows = [tuple(r) for r in refs]
    arr = (BnWindowRef * max(len(rows), 1))()
    for i, r in enumerate(rows):
        arr[i].recording = None if r[0] is None else r[0]._h
        arr[i].start = int(r[1])
        arr[i].source = int(r[2]) if len(r) > 2 else 0
        arr[i].window = int(r[3]) if len(r) > 3 else i
    return arr, rows


def recording_window_list(refs, segment_samples: int) -> np.ndarray:
    """bn_recording_window_list: the rows a list step would gather, copied back: f32 [len(refs), segment_samples]."""
    arr, keep = window_refs(refs)
    out = np.zeros((len(keep), segment_samples), dtype=np.float32)
    st = lib.bn_recording_window_list(arr, len(keep), C.sizeof(BnWindowRef), segment_samples, out.ctypes.data_as(C.POINTER(C.c_float)))
    if st:
        raise EngineError(st)
    return out


class Recording:
    """bn_recording: a mono recording uploaded once in its storage format (int16 or float32)."""

    def __init__(self, samples: np.ndarray, device: int = 0, src_rate: Optional[int] = None, dst_rate: Optional[int] = None,
                 zero_crossings: int = 0, async_upload: bool = False):
        """src_rate / dst_rate given and different: converted on the device by the polyphase resampler
        (bn_recording_create_resampled); the recording then holds f32 samples at dst_rate.
        async_upload: bn_recording_create_async -- returns at once, the windows' calls wait for the samples they read (this object
        keeps the array alive until the upload is done)."""
        a = np.ascontiguousarray(samples)
        if a.ndim != 1 or a.dtype not in (np.int16, np.float32):
            raise ValueError("mono int16 or float32 samples expected")
        h = C.c_void_p()
        fmt = 0 if a.dtype == np.int16 else 1
        if async_upload and src_rate and dst_rate:
            raise ValueError("async_upload cannot be combined with resampling: bn_recording_create_resampled converts during its own (synchronous) upload")
        if src_rate and dst_rate:
            st = lib.bn_recording_create_resampled(device, a.ctypes.data_as(C.c_void_p), a.shape[0], fmt, src_rate, dst_rate, zero_crossings, C.byref(h))
        elif async_upload:
            self._keep = a  # the uploader thread reads it until wait() / free
            st = lib.bn_recording_create_async(device, a.ctypes.data_as(C.c_void_p), a.shape[0], fmt, C.byref(h))
        else:
            st = lib.bn_recording_create(device, a.ctypes.data_as(C.c_void_p), a.shape[0], fmt, C.byref(h))
        if st:
            raise EngineError(st)
        self._h = h
        self.n_samples = int(lib.bn_recording_samples(h))
        if async_upload:
            _pending_uploads.add(self)  # joined at interpreter exit: the uploader thread must not outlive the array it reads

    @classmethod
    def _adopt(cls, h, keep=None, pending=False):
        r = cls.__new__(cls)
        r._h, r._keep = h, keep
        r.n_samples = int(lib.bn_recording_samples(h))
        if pending:
            _pending_uploads.add(r)
        return r

    @classmethod
    def from_layout(cls, pcm, fmt: int, channels: int = 1, channel: int = 0, device: int = 0, async_upload: bool = False,
                    src_rate: Optional[int] = None, dst_rate: Optional[int] = None, zero_crossings: int = 0) -> "Recording":
        """bn_recording_create_layout[_async | _resampled]: `pcm` holds interleaved frames of `channels` samples in format `fmt`
        (BN_PCM_*; bytes or any contiguous array -- packed 24-bit has no dtype of its own), read on the device as channel
        `channel` or, at BN_PCM_MIX, mixed down.  n_samples counts frames."""
        a = np.frombuffer(pcm, dtype=np.uint8) if isinstance(pcm, (bytes, bytearray, memoryview)) else np.ascontiguousarray(pcm).reshape(-1).view(np.uint8)
        fb = PCM_SAMPLE_BYTES.get(fmt, 1) * max(int(channels), 1)
        if a.shape[0] % fb:
            raise ValueError(f"{a.shape[0]} bytes are no whole number of {fb}-byte frames")
        n = a.shape[0] // fb
        lay = BnPcmLayout(fmt, channels, channel)
        h = C.c_void_p()
        if async_upload and src_rate and dst_rate:
            raise ValueError("async_upload cannot be combined with resampling")
        if src_rate and dst_rate:
            st = lib.bn_recording_create_layout_resampled(device, a.ctypes.data_as(C.c_void_p), n, C.byref(lay), C.sizeof(lay), src_rate, dst_rate, zero_crossings, C.byref(h))
        elif async_upload:
            st = lib.bn_recording_create_layout_async(device, a.ctypes.data_as(C.c_void_p), n, C.byref(lay), C.sizeof(lay), C.byref(h))
        else:
            st = lib.bn_recording_create_layout(device, a.ctypes.data_as(C.c_void_p), n, C.byref(lay), C.sizeof(lay), C.byref(h))
        if st:
            raise EngineError(st)
        return cls._adopt(h, a if async_upload else None, async_upload)

    def view_channel(self, channel: int) -> "Recording":
        """bn_recording_view_channel: the same device bytes read with another channel op; no second upload.  Either may go first."""
        h = C.c_void_p()
        st = lib.bn_recording_view_channel(self._h, channel, C.byref(h))
        if st:
            raise EngineError(st)
        keep = getattr(self, "_keep", None)
        return Recording._adopt(h, keep, keep is not None)  # a view shares the upload: it keeps the source array alive as well

    def wait(self):
        """The whole recording is on the device (no-op for a synchronous upload)."""
        st = lib.bn_recording_wait(self._h)
        if st:
            raise EngineError(st)
        self._keep = None

    def read_f32(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        count = self.n_samples - first if count is None else count
        out = np.zeros(max(count, 0), dtype=np.float32)
        st = lib.bn_recording_read_f32(self._h, first, count, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # lib is gone at interpreter shutdown
            lib.bn_recording_free(self._h)
            self._h = None

    def n_windows(self, step_samples: int) -> int:
        return int(lib.bn_chunk_count(self.n_samples, step_samples))

    def windows(self, segment_samples: int, step_samples: int, first: int, count: int) -> np.ndarray:
        """chunk_audio on the device, copied back: f32 [count, segment_samples]."""
        out = np.zeros((count, segment_samples), dtype=np.float32)
        st = lib.bn_recording_windows(self._h, segment_samples, step_samples, first, count, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out

    def levels(self, segment_samples: int, step_samples: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bn_recording_levels: peak, mean, mean_square and flags of windows [first, first + count) as a LEVEL_DTYPE array, computed on
        the device over exactly the samples windows() returns (count None: to the last window)."""
        count = self.n_windows(step_samples) - first if count is None else count
        out = np.zeros(max(count, 0), dtype=LEVEL_DTYPE)
        st = lib.bn_recording_levels(self._h, segment_samples, step_samples, first, count, out.ctypes.data_as(C.POINTER(BnWindowLevel)),
                                     C.sizeof(BnWindowLevel))
        if st:
            raise EngineError(st)
        return out

    def band_levels(self, segment_samples: int, step_samples: int, frame: int, hop: int, bands, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bn_recording_band_levels: per window the power inside bands = [(bin_lo, bin_hi), ...] of frames of `frame` samples every `hop`,
        mean and maximum over the window's frames, as a BAND_DTYPE array (count None: to the last window).  band_bins() gives the bins
        of a band in hertz."""
        count = self.n_windows(step_samples) - first if count is None else count
        out = np.zeros(max(count, 0), dtype=BAND_DTYPE)
        sp = band_spec(frame, hop, bands)
        st = lib.bn_recording_band_levels(self._h, segment_samples, step_samples, first, count, C.byref(sp), C.sizeof(BnBandSpec),
                                          out.ctypes.data_as(C.POINTER(BnWindowBands)), C.sizeof(BnWindowBands))
        if st:
            raise EngineError(st)
        return out



class Index:
    """bn_index: a device-resident store of L2-normalised embedding rows with exact top-M cosine search.  Row ids are the
    append order.  search / search_ids return (ids [n, top_m] uint64, scores [n, top_m] float32, counts [n] uint32); entries
    past counts[i] are left as written here (ids 0, scores NaN)."""

    def __init__(self, device: int, dim: int, capacity: int):
        h = C.c_void_p()
        st = lib.bn_index_create(device, dim, capacity, C.byref(h))
        if st:
            raise EngineError(st)
        self._h, self.device, self.dim, self.capacity = h, device, dim, capacity

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_index_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    def __len__(self) -> int:
        return int(lib.bn_index_size(self._h))

    def add(self, rows) -> int:
        """Append host rows [n, dim]; returns the id of the first."""
        a = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        first = C.c_uint64()
        st = lib.bn_index_add_host(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], C.byref(first))
        if st:
            raise EngineError(st)
        return int(first.value)

    def add_context(self, ctx: "Context", batch: int) -> int:
        """Append rows 0 .. batch-1 of the embedding output of ctx's last run, device to device; returns the id of the first."""
        first = C.c_uint64()
        st = lib.bn_index_add_ctx(self._h, ctx._h, batch, C.byref(first))
        if st:
            raise EngineError(st)
        return int(first.value)

    def read(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Stored (normalised) rows [first, first + count) as f32 [count, dim]."""
        count = len(self) - first if count is None else count
        out = np.zeros((max(count, 0), self.dim), dtype=np.float32)
        st = lib.bn_index_read(self._h, first, count, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out

    @staticmethod
    def _outputs(n: int, m_stride: int):
        return (np.zeros((n, m_stride), dtype=np.uint64), np.full((n, m_stride), np.nan, dtype=np.float32), np.zeros(n, dtype=np.uint32))

    def search(self, queries, top_m: int, m_stride: Optional[int] = None):
        """Top-M rows by cosine for host queries [n, dim]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts = self._outputs(q.shape[0], max(m_stride, 0))
        st = lib.bn_index_search(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], top_m, m_stride,
                                 ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                 counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, counts

    def match(self, rows, top_m: int, min_score: Optional[float] = None, m_stride: Optional[int] = None):
        """bn_index_match: what a step of a context with this index attached computes for its embedding rows, on host rows [n, dim]:
        (ids, scores, tags [n, top_m], counts [n]), the prefix of search()'s lists scoring at least min_score, with the tags of the hits."""
        q = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts = self._outputs(q.shape[0], max(m_stride, 0))
        tags = np.zeros(ids.shape, dtype=np.uint32)
        st = lib.bn_index_match(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], top_m, *_min_args(min_score), m_stride,
                                ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                tags.ctypes.data_as(C.POINTER(C.c_uint32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, tags, counts

    def search_head(self, head: "Head", top_m: int):
        """Per class, the top_m stored rows by head logit: bn_index_search with W_c as the query.  For a stored (unit) row
        logit = cosine * |W_c| + b_c, so the ranking does not depend on the query's positive scale or on the bias; returns
        (ids, logits, counts) with the cosine converted back to that logit in float64 (a class whose W_c is zero has count 0)."""
        w, b = head.read()
        ids, cos, counts = self.search(w, top_m)
        norm = np.sqrt((w.astype(np.float64) ** 2).sum(axis=1))
        return ids, cos.astype(np.float64) * norm[:, None] + b.astype(np.float64)[:, None], counts

    def search_ids(self, ids, top_m: int, exclude_radius: int = -1, m_stride: Optional[int] = None):
        """Query by example: the stored rows `ids` are the queries; rows within exclude_radius of a query's id are skipped."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        m_stride = top_m if m_stride is None else m_stride
        out_ids, scores, counts = self._outputs(qi.shape[0], max(m_stride, 0))
        st = lib.bn_index_search_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius, top_m, m_stride,
                                     out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                     counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out_ids, scores, counts

    def search_peaks(self, queries, top_m: int, peak_radius: int, m_stride: Optional[int] = None):
        """bn_index_search_peaks: search(), but only rows that no eligible row within peak_radius ids of them beats are returned: one hit
        per local peak of the score over row ids.  peak_radius 0 is search()."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts = self._outputs(q.shape[0], max(m_stride, 0))
        st = lib.bn_index_search_peaks(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], peak_radius, top_m, m_stride,
                                       ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                       counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, counts

    def search_peaks_ids(self, ids, top_m: int, peak_radius: int, exclude_radius: int = -1, m_stride: Optional[int] = None):
        """bn_index_search_peaks_ids: search_ids(), restricted to the local peaks as search_peaks() is; rows within exclude_radius of a
        query's id are neither returned nor do they suppress a neighbour."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        m_stride = top_m if m_stride is None else m_stride
        out_ids, scores, counts = self._outputs(qi.shape[0], max(m_stride, 0))
        st = lib.bn_index_search_peaks_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius, peak_radius, top_m,
                                           m_stride, out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                           counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out_ids, scores, counts

    def search_seq(self, queries, seq_len: int, top_m: int, peak_radius: int = 0, m_stride: Optional[int] = None):
        """bn_index_search_seq: each query is a run of seq_len consecutive windows, host rows [n_seq * seq_len, dim]; start row i of the
        index scores the mean of the window scores along the diagonal, mean_j dot(query_j, row[i + j]).  Returns the best top_m starts
        per sequence (ids [n_seq, top_m] are START rows); with peak_radius >= 1 only local peaks over start ids, by search_peaks()' rule."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        n_seq = q.shape[0] // max(seq_len, 1)
        if seq_len >= 1 and q.shape[0] != n_seq * seq_len:
            raise ValueError(f"{q.shape[0]} query rows are not a whole number of sequences of {seq_len}")
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts = self._outputs(n_seq, max(m_stride, 0))
        st = lib.bn_index_search_seq(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), n_seq, seq_len, peak_radius, top_m, m_stride,
                                     ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                     counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, counts

    def search_seq_ids(self, first_ids, seq_len: int, exclude_radius: int, top_m: int, peak_radius: int = 0, m_stride: Optional[int] = None):
        """bn_index_search_seq_ids: search_seq() with the stored rows [first_ids[i], first_ids[i] + seq_len) as sequence i; starts within
        exclude_radius of first_ids[i] are neither returned nor do they suppress a neighbour (< 0: none; 0: the query's own start)."""
        qi = np.ascontiguousarray(first_ids, dtype=np.uint64).reshape(-1)
        m_stride = top_m if m_stride is None else m_stride
        out_ids, scores, counts = self._outputs(qi.shape[0], max(m_stride, 0))
        st = lib.bn_index_search_seq_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], seq_len, exclude_radius, peak_radius, top_m,
                                         m_stride, out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                         counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out_ids, scores, counts

    @staticmethod
    def _thresholds(min_score, n: int) -> np.ndarray:
        """a scalar or an array [n] -> f32 [n]"""
        return np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, dtype=np.float32).reshape(-1), (n,)))

    def search_above(self, queries, min_score, max_hits: int, first_id: int = 0, n_ids: int = 0, h_stride: Optional[int] = None):
        """bn_index_search_above: EVERY row of [first_id, first_id + n_ids) (n_ids 0: to the end) scoring at least min_score (a scalar or
        one value per query) for host queries [n, dim], in id order: (ids, scores, tags [n, h_stride], counts [n]).  counts[i] is the
        total number of hits, also beyond max_hits; the first min(counts[i], max_hits) are returned, the entries past them stay as
        written here (id 0, score NaN, tag 0)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        thr = self._thresholds(min_score, q.shape[0])
        h_stride = max_hits if h_stride is None else h_stride
        ids, scores, counts = self._outputs(q.shape[0], max(h_stride, 0))
        tags = np.zeros(ids.shape, dtype=np.uint32)
        st = lib.bn_index_search_above(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], thr.ctypes.data_as(C.POINTER(C.c_float)), first_id,
                                       n_ids, max_hits, h_stride, ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                       tags.ctypes.data_as(C.POINTER(C.c_uint32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, tags, counts

    def search_above_ids(self, ids, min_score, max_hits: int, exclude_radius: int = -1, first_id: int = 0, n_ids: int = 0,
                         h_stride: Optional[int] = None):
        """bn_index_search_above_ids: search_above() with the stored rows `ids` as the queries; rows within exclude_radius of a query's id
        are no hits."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        thr = self._thresholds(min_score, qi.shape[0])
        h_stride = max_hits if h_stride is None else h_stride
        out_ids, scores, counts = self._outputs(qi.shape[0], max(h_stride, 0))
        tags = np.zeros(out_ids.shape, dtype=np.uint32)
        st = lib.bn_index_search_above_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius,
                                           thr.ctypes.data_as(C.POINTER(C.c_float)), first_id, n_ids, max_hits, h_stride,
                                           out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                           tags.ctypes.data_as(C.POINTER(C.c_uint32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out_ids, scores, tags, counts

    def count_above(self, queries, min_score, first_id: int = 0, n_ids: int = 0) -> np.ndarray:
        """bn_index_search_above with max_hits 0: the number of rows of the range scoring at least min_score, per query [n] uint32."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        thr = self._thresholds(min_score, q.shape[0])
        counts = np.zeros(q.shape[0], dtype=np.uint32)
        st = lib.bn_index_search_above(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], thr.ctypes.data_as(C.POINTER(C.c_float)), first_id,
                                       n_ids, 0, 0, None, None, None, counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return counts

    @staticmethod
    def _group_outputs(n: int, g_stride: int):
        """the seven output arrays of group_above, as the binding fills them before the call: what lies past n_groups stays like this
        (count 0, ids BN_GROUP_NO_ROW, score NaN)"""
        none = np.uint64(BN_GROUP_NO_ROW)
        return (np.zeros((n, g_stride), dtype=np.uint32), np.full((n, g_stride), none, dtype=np.uint64), np.full((n, g_stride), np.nan, dtype=np.float32),
                np.full((n, g_stride), none, dtype=np.uint64), np.full((n, g_stride), none, dtype=np.uint64), np.zeros(n, dtype=np.uint32),
                np.zeros(n, dtype=np.uint32))

    @staticmethod
    def _group_pointers(out):
        u64p = C.POINTER(C.c_uint64)
        u32p = C.POINTER(C.c_uint32)
        return (out[0].ctypes.data_as(u32p), out[1].ctypes.data_as(u64p), out[2].ctypes.data_as(C.POINTER(C.c_float)), out[3].ctypes.data_as(u64p),
                out[4].ctypes.data_as(u64p), out[5].ctypes.data_as(u32p), out[6].ctypes.data_as(u32p))

    def group_above(self, queries, min_score, n_groups: int, first_id: int = 0, n_ids: int = 0, g_stride: Optional[int] = None):
        """bn_index_group_above: the rows of [first_id, first_id + n_ids) (n_ids 0: to the end) scoring at least min_score (a scalar or one
        value per query) for host queries [n, dim], grouped by row tag: (counts, best_ids, best_scores, first_ids, last_ids [n, g_stride],
        other, total [n]).  Group g of query i is entry [i, g]; a group without hits has count 0, ids BN_GROUP_NO_ROW and score 0.0; hits
        whose tag is >= n_groups are counted in other[i] only; total[i] = counts[i, :n_groups].sum() + other[i]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        thr = self._thresholds(min_score, q.shape[0])
        g_stride = n_groups if g_stride is None else g_stride
        out = self._group_outputs(q.shape[0], max(g_stride, 0))
        st = lib.bn_index_group_above(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], thr.ctypes.data_as(C.POINTER(C.c_float)), first_id,
                                      n_ids, n_groups, g_stride, *self._group_pointers(out))
        if st:
            raise EngineError(st)
        return out

    def group_above_ids(self, ids, min_score, n_groups: int, exclude_radius: int = -1, first_id: int = 0, n_ids: int = 0,
                        g_stride: Optional[int] = None):
        """bn_index_group_above_ids: group_above() with the stored rows `ids` as the queries; rows within exclude_radius of a query's id
        are no hits."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        thr = self._thresholds(min_score, qi.shape[0])
        g_stride = n_groups if g_stride is None else g_stride
        out = self._group_outputs(qi.shape[0], max(g_stride, 0))
        st = lib.bn_index_group_above_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius,
                                          thr.ctypes.data_as(C.POINTER(C.c_float)), first_id, n_ids, n_groups, g_stride, *self._group_pointers(out))
        if st:
            raise EngineError(st)
        return out

    def set_tags(self, first_id: int, tags) -> None:
        """bn_index_set_tags: rows [first_id, first_id + len(tags)) get the tags given (each below BN_INDEX_TAG_LIMIT)."""
        t = np.ascontiguousarray(tags, dtype=np.uint32).reshape(-1)
        st = lib.bn_index_set_tags(self._h, first_id, t.shape[0], t.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)

    def fill_tags(self, first_id: int, n: int, tag: int) -> None:
        """bn_index_fill_tags: rows [first_id, first_id + n) all get `tag`, e.g. the batch add_context just appended."""
        st = lib.bn_index_fill_tags(self._h, first_id, n, tag)
        if st:
            raise EngineError(st)

    def tags(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bn_index_read_tags: the tags of rows [first, first + count) as uint32; count None: to the last row.  A row never tagged has 0."""
        count = max(len(self) - first, 0) if count is None else count
        out = np.zeros(max(count, 0), dtype=np.uint32)
        st = lib.bn_index_read_tags(self._h, first, count, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out

    def append_rows(self, src: "Index", first_id: int = 0, n_ids: int = 0) -> int:
        """bn_index_append_rows: rows [first_id, first_id + n_ids) of `src` (n_ids 0: to its end) appended with their stored bits, valid
        bytes and tags, device to device; returns the id of the first new row."""
        first = C.c_uint64()
        st = lib.bn_index_append_rows(self._h, src._h, first_id, n_ids, C.byref(first))
        if st:
            raise EngineError(st)
        return int(first.value)

    def append_subset(self, subset: "Subset") -> int:
        """bn_index_append_subset: the members of `subset` (of another index), in its order, appended as append_rows appends a range;
        returns the id of the first new row.  New row j is the subset's j-th member."""
        first = C.c_uint64()
        st = lib.bn_index_append_subset(self._h, subset._h, C.byref(first))
        if st:
            raise EngineError(st)
        return int(first.value)

    def save(self, path, chunk_rows: int = 0) -> None:
        """bn_index_save: the stored bits of every row to `path` (written under a temporary name, renamed when complete); chunk_rows
        0 takes the default.  Index.load(path) gives an index that answers every call as this one does now."""
        st = lib.bn_index_save(self._h, os.fsencode(path), chunk_rows)
        if st:
            raise EngineError(st)

    @classmethod
    def load(cls, path, device: int = 0, capacity_rows: int = 0) -> "Index":
        """bn_index_load: an index holding the rows of a file Index.save wrote, with room for capacity_rows rows (0: the file's)."""
        h = C.c_void_p()
        st = lib.bn_index_load(device, os.fsencode(path), capacity_rows, C.byref(h))
        if st:
            raise EngineError(st)
        x = cls.__new__(cls)
        x._h, x.device, x.dim = h, device, int(lib.bn_index_dim(h))
        x.capacity = capacity_rows if capacity_rows else max(int(lib.bn_index_size(h)), 1)
        return x

    def _range(self, first_id: int, n_ids: int) -> int:
        return max((n_ids if n_ids else len(self) - first_id), 0)

    def assign(self, centroids, first_id: int = 0, n_ids: int = 0):
        """bn_index_assign: the nearest of `centroids` [k, dim] (used as given) for rows [first_id, first_id + n_ids) (n_ids 0: to
        the end).  Returns (assign [rows] uint32, scores [rows] float32); a row without a cluster has BN_CLUSTER_NONE and NaN."""
        c = np.ascontiguousarray(centroids, dtype=np.float32).reshape(-1, self.dim)
        n = self._range(first_id, n_ids)
        assign = np.full(n, BN_CLUSTER_NONE, dtype=np.uint32)
        scores = np.full(n, np.nan, dtype=np.float32)
        st = lib.bn_index_assign(self._h, c.ctypes.data_as(C.POINTER(C.c_float)), c.shape[0], first_id, n_ids,
                                 assign.ctypes.data_as(C.POINTER(C.c_uint32)), scores.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return assign, scores

    def cluster(self, k: int, first_id: int = 0, n_ids: int = 0, max_iters: int = 0, init_ids=None, init_centroids=None, history: int = 0):
        """bn_index_cluster: spherical k-means of rows [first_id, first_id + n_ids) into k clusters, started from the stored rows
        `init_ids`, from `init_centroids` [k, dim], or from the built-in max-min start.  Returns (centroids [k, dim] float32,
        assign [rows] uint32, scores [rows] float32, counts [k] uint32, report); report = {iters, converged, empty_clusters,
        moved_last, objective, start_ids (None under init_centroids), objective_history (the first `history` passes)}."""
        n = self._range(first_id, n_ids)
        cent = np.zeros((k, self.dim), dtype=np.float32)
        assign = np.full(n, BN_CLUSTER_NONE, dtype=np.uint32)
        scores = np.full(n, np.nan, dtype=np.float32)
        counts = np.zeros(k, dtype=np.uint32)
        ids = None if init_ids is None else np.ascontiguousarray(init_ids, dtype=np.uint64).reshape(-1)
        ic = None if init_centroids is None else np.ascontiguousarray(init_centroids, dtype=np.float32).reshape(-1, self.dim)
        if (ids is not None and ids.shape[0] != k) or (ic is not None and ic.shape[0] != k):
            raise ValueError("init_ids / init_centroids must hold k entries")
        start = np.zeros(k, dtype=np.uint64)
        hist = np.full(max(history, 1), np.nan, dtype=np.float64)
        o = BnClusterOpts(max_iters, None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                          None if ic is None else ic.ctypes.data_as(C.POINTER(C.c_float)), start.ctypes.data_as(C.POINTER(C.c_uint64)),
                          hist.ctypes.data_as(C.POINTER(C.c_double)) if history else None, history)
        rep = BnClusterReport()
        st = lib.bn_index_cluster(self._h, k, first_id, n_ids, C.byref(o), C.sizeof(o), cent.ctypes.data_as(C.POINTER(C.c_float)),
                                  assign.ctypes.data_as(C.POINTER(C.c_uint32)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                  counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(rep), C.sizeof(rep))
        if st:
            raise EngineError(st)
        report = {"iters": int(rep.iters), "converged": bool(rep.converged), "empty_clusters": int(rep.empty_clusters),
                  "moved_last": int(rep.moved_last), "objective": float(rep.objective), "start_ids": None if ic is not None else start,
                  "objective_history": hist[:int(rep.history_len)].copy()}
        return cent, assign, scores, counts, report


def index_file_info(path) -> dict:
    """bn_index_file_info: the header fields of an index file (host only): dim, rows, valid_rows, chunk_rows, n_chunks, version."""
    info = BnIndexFileInfo()
    st = lib.bn_index_file_info(os.fsencode(path), C.byref(info), C.sizeof(info))
    if st:
        raise EngineError(st)
    return {k: int(getattr(info, k)) for k in ("dim", "rows", "valid_rows", "chunk_rows", "n_chunks", "version")}


def index_file_verify(path) -> None:
    """bn_index_file_verify: every digest of an index file recomputed on the CPU, the finite and valid_rows rules applied (host only).
    Raises EngineError; its first_bad_chunk is the first chunk with a digest mismatch or a non-finite element, else None."""
    bad = C.c_uint64()
    st = lib.bn_index_file_verify(os.fsencode(path), C.byref(bad))
    if st:
        e = EngineError(st)
        e.first_bad_chunk = None if bad.value == 0xFFFFFFFFFFFFFFFF else int(bad.value)
        raise e


class Ivf:
    """bn_ivf: an inverted-file view of an Index under `centroids` [k, dim] (used as given): the exact assignment of its rows and one
    member list per centroid.  search / search_ids scan only the nprobe best lists of each query and return (ids [n, top_m] uint64,
    scores [n, top_m] float32, counts [n] uint32, probes [n, nprobe] uint32, scanned [n] uint64): what Index.search would return if
    only the probed lists' rows existed.  Rows appended to the index are searched after extend().  The view keeps the Index alive."""

    def __init__(self, index: "Index", centroids):
        c = np.ascontiguousarray(centroids, dtype=np.float32).reshape(-1, index.dim)
        h = C.c_void_p()
        st = lib.bn_ivf_build(index._h, c.ctypes.data_as(C.POINTER(C.c_float)), c.shape[0], C.byref(h))
        if st:
            raise EngineError(st)
        self._h, self.index = h, index

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_ivf_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    def __len__(self) -> int:
        """the number of lists, k"""
        return int(lib.bn_ivf_lists(self._h))

    @property
    def rows(self) -> int:
        """the covered rows: ids [0, rows)"""
        return int(lib.bn_ivf_rows(self._h))

    def extend(self) -> None:
        st = lib.bn_ivf_extend(self._h)
        if st:
            raise EngineError(st)

    def list_sizes(self) -> np.ndarray:
        out = np.zeros(len(self), dtype=np.uint32)
        st = lib.bn_ivf_list_sizes(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out

    def read_list(self, c: int) -> np.ndarray:
        """the ids of list c, ascending"""
        n = C.c_size_t()
        out = np.zeros(int(self.list_sizes()[c]) if 0 <= c < len(self) else 0, dtype=np.uint64)
        st = lib.bn_ivf_read_list(self._h, c, out.ctypes.data_as(C.POINTER(C.c_uint64)), out.shape[0], C.byref(n))
        if st:
            raise EngineError(st)
        return out[:int(n.value)]

    @staticmethod
    def _outputs(n: int, m_stride: int, nprobe: int):
        return Index._outputs(n, m_stride) + (np.full((n, max(nprobe, 0)), BN_CLUSTER_NONE, dtype=np.uint32), np.zeros(n, dtype=np.uint64))

    def search(self, queries, nprobe: int, top_m: int, m_stride: Optional[int] = None):
        """Top-M rows by cosine among the nprobe best lists of each host query [n, dim]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.index.dim)
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts, probes, scanned = self._outputs(q.shape[0], max(m_stride, 0), nprobe)
        st = lib.bn_ivf_search(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], nprobe, top_m, m_stride,
                               ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                               counts.ctypes.data_as(C.POINTER(C.c_uint32)), probes.ctypes.data_as(C.POINTER(C.c_uint32)),
                               scanned.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st:
            raise EngineError(st)
        return ids, scores, counts, probes, scanned

    def search_ids(self, ids, nprobe: int, top_m: int, exclude_radius: int = -1, m_stride: Optional[int] = None):
        """Query by example among the nprobe best lists of each stored row `ids`; rows within exclude_radius of a query's id are skipped."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        m_stride = top_m if m_stride is None else m_stride
        out_ids, scores, counts, probes, scanned = self._outputs(qi.shape[0], max(m_stride, 0), nprobe)
        st = lib.bn_ivf_search_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius, nprobe, top_m, m_stride,
                                   out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                   counts.ctypes.data_as(C.POINTER(C.c_uint32)), probes.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   scanned.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st:
            raise EngineError(st)
        return out_ids, scores, counts, probes, scanned


class Sq8:
    """bn_sq8: an int8 view of an Index: one code byte per element and one f32 scale per row.  search / search_ids rank every covered
    row by an exact integer key, keep the `refine` best as candidates and re-score those exactly; they return (ids [n, top_m] uint64,
    scores [n, top_m] float32, counts [n] uint32, cands [n, refine] uint64, cand_counts [n] uint32): what Index.search would return if
    only the candidates existed.  Rows appended to the index are searched after extend().  The view keeps the Index alive."""

    def __init__(self, index: "Index"):
        h = C.c_void_p()
        st = lib.bn_sq8_build(index._h, C.byref(h))
        if st:
            raise EngineError(st)
        self._h, self.index = h, index

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_sq8_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    @property
    def rows(self) -> int:
        """the covered rows: ids [0, rows)"""
        return int(lib.bn_sq8_rows(self._h))

    def extend(self) -> None:
        st = lib.bn_sq8_extend(self._h)
        if st:
            raise EngineError(st)

    def read(self, first: int = 0, count: Optional[int] = None):
        """(codes [count, dim] int8, scales [count] float32) of rows [first, first + count); count None: to the last covered row"""
        count = max(self.rows - first, 0) if count is None else count
        codes = np.zeros((max(count, 0), self.index.dim), dtype=np.int8)
        scales = np.zeros(max(count, 0), dtype=np.float32)
        st = lib.bn_sq8_read(self._h, first, count, codes.ctypes.data_as(C.POINTER(C.c_int8)), scales.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return codes, scales

    @staticmethod
    def _outputs(n: int, m_stride: int, refine: int):
        return Index._outputs(n, m_stride) + (np.zeros((n, max(refine, 0)), dtype=np.uint64), np.zeros(n, dtype=np.uint32))

    def search(self, queries, refine: int, top_m: int, m_stride: Optional[int] = None):
        """Top-M rows by cosine among the `refine` coarse candidates of each host query [n, dim]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.index.dim)
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts, cands, cand_counts = self._outputs(q.shape[0], max(m_stride, 0), refine)
        st = lib.bn_sq8_search(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], refine, top_m, m_stride,
                               ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                               counts.ctypes.data_as(C.POINTER(C.c_uint32)), cands.ctypes.data_as(C.POINTER(C.c_uint64)),
                               cand_counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, counts, cands, cand_counts

    def search_ids(self, ids, refine: int, top_m: int, exclude_radius: int = -1, m_stride: Optional[int] = None):
        """Query by example among the `refine` coarse candidates of each stored row `ids`; rows within exclude_radius of a query's id
        are neither candidates nor results."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        m_stride = top_m if m_stride is None else m_stride
        out_ids, scores, counts, cands, cand_counts = self._outputs(qi.shape[0], max(m_stride, 0), refine)
        st = lib.bn_sq8_search_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius, refine, top_m, m_stride,
                                   out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                   counts.ctypes.data_as(C.POINTER(C.c_uint32)), cands.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   cand_counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out_ids, scores, counts, cands, cand_counts


class Subset:
    """bn_subset: a fixed, ascending list of row ids of an Index.  search / search_ids return (ids [n, top_m] uint64, scores [n, top_m]
    float32, counts [n] uint32): what Index.search / Index.search_ids would return if only the subset's rows existed, from one read of
    those rows for all queries of a pass.  Rows appended and tags changed afterwards do not alter the list.  The subset keeps the Index
    alive.  Make one with Subset.select or Subset.from_ids."""

    def __init__(self, index: "Index", handle):
        self._h, self.index = handle, index

    @classmethod
    def select(cls, index: "Index", first_id: int = 0, n_ids: int = 0, tags=None, exclude: bool = False) -> "Subset":
        """bn_subset_select: the rows of [first_id, first_id + n_ids) (n_ids 0: to the end) whose tag is in `tags`, or, with exclude,
        is not in it; tags None or empty: every row of the range."""
        t = None if tags is None else np.ascontiguousarray(tags, dtype=np.uint32).reshape(-1)
        f = BnIndexFilter(first_id, n_ids, None if t is None else t.ctypes.data_as(C.POINTER(C.c_uint32)), 0 if t is None else t.shape[0],
                          BN_FILTER_EXCLUDE_TAGS if exclude else 0)
        h = C.c_void_p()
        st = lib.bn_subset_select(index._h, C.byref(f), C.sizeof(f), C.byref(h))
        if st:
            raise EngineError(st)
        return cls(index, h)

    @classmethod
    def from_ids(cls, index: "Index", ids) -> "Subset":
        """bn_subset_from_ids: the rows `ids`, strictly ascending."""
        a = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        h = C.c_void_p()
        st = lib.bn_subset_from_ids(index._h, a.ctypes.data_as(C.POINTER(C.c_uint64)), a.shape[0], C.byref(h))
        if st:
            raise EngineError(st)
        return cls(index, h)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_subset_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    def __len__(self) -> int:
        return int(lib.bn_subset_size(self._h))

    @property
    def ids(self) -> np.ndarray:
        """the members, ascending, as uint64"""
        out = np.zeros(len(self), dtype=np.uint64)
        st = lib.bn_subset_read(self._h, 0, out.shape[0], out.ctypes.data_as(C.POINTER(C.c_uint64)))
        if st:
            raise EngineError(st)
        return out

    def search(self, queries, top_m: int, m_stride: Optional[int] = None):
        """Top-M members by cosine for host queries [n, dim]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.index.dim)
        m_stride = top_m if m_stride is None else m_stride
        ids, scores, counts = Index._outputs(q.shape[0], max(m_stride, 0))
        st = lib.bn_subset_search(self._h, q.ctypes.data_as(C.POINTER(C.c_float)), q.shape[0], top_m, m_stride,
                                  ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                  counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, scores, counts

    def search_ids(self, ids, top_m: int, exclude_radius: int = -1, m_stride: Optional[int] = None):
        """Query by example: the stored rows `ids` of the index (members or not) are the queries; members within exclude_radius of a
        query's id are skipped."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        m_stride = top_m if m_stride is None else m_stride
        out_ids, scores, counts = Index._outputs(qi.shape[0], max(m_stride, 0))
        st = lib.bn_subset_search_ids(self._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), qi.shape[0], exclude_radius, top_m, m_stride,
                                      out_ids.ctypes.data_as(C.POINTER(C.c_uint64)), scores.ctypes.data_as(C.POINTER(C.c_float)),
                                      counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return out_ids, scores, counts


def _fit_opts(n_classes: int, l2: float, tol: float, max_iters: int, l2norm: bool, pos_weight):
    pw = None
    if pos_weight is not None:
        pw = np.ascontiguousarray(pos_weight, dtype=np.float32).reshape(n_classes)
    o = BnHeadFitOpts(l2, tol, max_iters, BN_HEAD_L2NORM if l2norm else 0, None if pw is None else pw.ctypes.data_as(C.POINTER(C.c_float)))
    return o, pw  # pw must outlive the call


class Head:
    """bn_head: an immutable linear classifier head over embeddings, resident on one device.  `Head(device, W, bias)` from host
    weights, `Head.fit(...)` / `Head.fit_index(...)` fitted on the device; `apply(rows)` on host rows, `Context.attach_head` for
    every step of a context.  A fitted head carries `report` = {iters, converged, loss, certificate}."""

    def __init__(self, device: int, W, bias=None, l2norm: bool = False, _handle=None):
        self.report = None
        if _handle is not None:
            self._h = _handle
            return
        w = np.ascontiguousarray(W, dtype=np.float32)
        if w.ndim != 2:
            raise ValueError("W must be [n_classes, dim]")
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32).reshape(w.shape[0])
        f32p = C.POINTER(C.c_float)
        h = C.c_void_p()
        st = lib.bn_head_create(device, w.shape[1], w.shape[0], w.ctypes.data_as(f32p), None if b is None else b.ctypes.data_as(f32p),
                                BN_HEAD_L2NORM if l2norm else 0, C.byref(h))
        if st:
            raise EngineError(st)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_head_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    @staticmethod
    def _fitted(h, rep: BnHeadFitReport) -> "Head":
        out = Head(0, None, _handle=h)
        out.report = {"iters": int(rep.iters), "converged": bool(rep.converged), "loss": float(rep.loss), "certificate": float(rep.certificate)}
        return out

    @staticmethod
    def fit(device: int, rows, labels, l2: float = 0.0, tol: float = 0.0, max_iters: int = 0, l2norm: bool = False, pos_weight=None) -> "Head":
        """bn_head_fit: L2-regularised logistic regression of labels [n, n_classes] (0 / 1) on rows [n, dim]; zero options take
        the library's defaults (l2 1e-3, tol 1e-6, max_iters 2000)."""
        x = np.ascontiguousarray(rows, dtype=np.float32)
        y = np.ascontiguousarray(labels, dtype=np.uint8)
        if x.ndim != 2 or y.ndim != 2 or y.shape[0] != x.shape[0]:
            raise ValueError("rows must be [n, dim] and labels [n, n_classes]")
        o, pw = _fit_opts(y.shape[1], l2, tol, max_iters, l2norm, pos_weight)
        h, rep = C.c_void_p(), BnHeadFitReport()
        st = lib.bn_head_fit(device, x.shape[1], y.shape[1], x.ctypes.data_as(C.POINTER(C.c_float)), y.ctypes.data_as(C.POINTER(C.c_uint8)),
                             x.shape[0], C.byref(o), C.sizeof(o), C.byref(h), C.byref(rep), C.sizeof(rep))
        if st:
            raise EngineError(st)
        return Head._fitted(h, rep)

    @staticmethod
    def fit_index(index: "Index", ids, labels, l2: float = 0.0, tol: float = 0.0, max_iters: int = 0, pos_weight=None) -> "Head":
        """bn_head_fit_index: the training rows are stored rows of `index`, taken by id on the device."""
        qi = np.ascontiguousarray(ids, dtype=np.uint64).reshape(-1)
        y = np.ascontiguousarray(labels, dtype=np.uint8)
        if y.ndim != 2 or y.shape[0] != qi.shape[0]:
            raise ValueError("labels must be [len(ids), n_classes]")
        o, pw = _fit_opts(y.shape[1], l2, tol, max_iters, True, pos_weight)
        h, rep = C.c_void_p(), BnHeadFitReport()
        st = lib.bn_head_fit_index(index._h, qi.ctypes.data_as(C.POINTER(C.c_uint64)), y.ctypes.data_as(C.POINTER(C.c_uint8)), qi.shape[0], y.shape[1],
                                   C.byref(o), C.sizeof(o), C.byref(h), C.byref(rep), C.sizeof(rep))
        if st:
            raise EngineError(st)
        return Head._fitted(h, rep)

    @property
    def dim(self) -> int:
        return int(lib.bn_head_dim(self._h))

    @property
    def n_classes(self) -> int:
        return int(lib.bn_head_classes(self._h))

    @property
    def l2norm(self) -> bool:
        return bool(lib.bn_head_flags(self._h) & BN_HEAD_L2NORM)

    def read(self):
        """(W [n_classes, dim], bias [n_classes]) as stored on the device."""
        w = np.empty((self.n_classes, self.dim), dtype=np.float32)
        b = np.empty(self.n_classes, dtype=np.float32)
        st = lib.bn_head_read(self._h, w.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return w, b

    def rank_index(self, index: "Index", top_m: int, mode="top", first_id: int = 0, n_ids: int = 0, exclude=None, m_stride: Optional[int] = None):
        """bn_head_rank_index: per class, the top_m stored rows of `index` by this head's logit ("top": logit descending) or by
        nearness to the decision boundary ("uncertain": |logit| ascending), among rows [first_id, first_id + n_ids) (n_ids 0: to
        the end) that are not in `exclude`.  Returns (ids [n_classes, m_stride] uint64, logits [n_classes, m_stride] float32,
        counts [n_classes] uint32); entries past counts[c] are left as written here (ids 0, logits NaN)."""
        if isinstance(mode, str):
            modes = {"top": BN_RANK_TOP, "uncertain": BN_RANK_UNCERTAIN}
            if mode not in modes:
                raise ValueError("mode must be 'top' or 'uncertain'")
            mode = modes[mode]
        m_stride = top_m if m_stride is None else m_stride
        ex = None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint64).reshape(-1)
        ids, logits, counts = Index._outputs(self.n_classes, max(m_stride, 0))
        st = lib.bn_head_rank_index(self._h, index._h, mode, first_id, n_ids, None if ex is None else ex.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    0 if ex is None else ex.shape[0], top_m, m_stride, ids.ctypes.data_as(C.POINTER(C.c_uint64)),
                                    logits.ctypes.data_as(C.POINTER(C.c_float)), counts.ctypes.data_as(C.POINTER(C.c_uint32)))
        if st:
            raise EngineError(st)
        return ids, logits, counts

    def apply(self, rows) -> np.ndarray:
        """bn_head_apply_host: logits [n, n_classes] of host rows [n, dim]."""
        x = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        out = np.empty((x.shape[0], self.n_classes), dtype=np.float32)
        st = lib.bn_head_apply_host(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out


class Prior:
    """bn_prior: an immutable table of species priors per site, [n_sites, n_species] f32, resident on one device (rows as
    RangeFilter.prior_row returns them; BN_PRIOR_UNKNOWN for species the meta model does not know).  `apply(logits, sites, ...)`
    on host rows, `Context.attach_prior` for every step of a context.  after_topk=False: the K best admitted species of all
    (BN_PRIOR_SELECT); True: filter_predictions over the step's own top-K row."""

    def __init__(self, device: int, table, threshold: float = 0.01, after_topk: bool = False, rerank: bool = False, flags: Optional[int] = None):
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 2:
            raise ValueError("table must be [n_sites, n_species]")
        if flags is None:
            flags = (BN_PRIOR_AFTER_TOPK if after_topk else 0) | (BN_PRIOR_RERANK if rerank else 0)
        h = C.c_void_p()
        st = lib.bn_prior_create(device, t.shape[0], t.shape[1], t.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(threshold), flags, C.byref(h))
        if st:
            raise EngineError(st)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_prior_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    @property
    def n_sites(self) -> int:
        return int(lib.bn_prior_sites(self._h))

    @property
    def n_species(self) -> int:
        return int(lib.bn_prior_species(self._h))

    @property
    def threshold(self) -> float:
        return float(lib.bn_prior_threshold(self._h))

    @property
    def flags(self) -> int:
        return int(lib.bn_prior_flags(self._h))

    def read(self, first_site: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Table rows [count, n_species] as stored on the device."""
        count = self.n_sites - first_site if count is None else count
        out = np.empty((max(count, 0), self.n_species), dtype=np.float32)
        st = lib.bn_prior_read(self._h, first_site, count, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out

    def apply(self, logits, sites, top_k: int = 10, min_confidence: Optional[float] = None, k_stride: Optional[int] = None):
        """bn_prior_apply_host: (idx [rows, k_stride], conf [rows, k_stride], count [rows]) of host logits [rows, n_species], row r at
        sites[r]; the kernels a step runs."""
        x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, self.n_species)
        sv = np.ascontiguousarray(sites, dtype=np.int32).reshape(-1)
        if sv.shape[0] != x.shape[0]:
            raise ValueError("one site per row")
        ks = max(min(top_k, self.n_species), 1) if k_stride is None else k_stride
        idx = np.zeros((x.shape[0], ks), dtype=np.uint32)
        conf = np.zeros((x.shape[0], ks), dtype=np.float32)
        cnt = np.zeros(x.shape[0], dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        st = lib.bn_prior_apply_host(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], sv.ctypes.data_as(C.POINTER(C.c_int32)), top_k,
                                     *_min_args(min_confidence), ks, idx.ctypes.data_as(u32p),
                                     conf.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(u32p))
        if st:
            raise EngineError(st)
        return idx, conf, cnt


class Tracker:
    """bn_track: detection events on the device -- one record per (source, species), updated with the logits row of every window of
    every source, emitting finished events only: species j was heard at source s from first_window to last_window, `hits` times,
    with a peak and a mean confidence.  A window is a hit when its confidence is at least enter_conf; an event closes after more
    than max_gap missed windows and is emitted with at least min_hits hits.  `update(logits, sources, windows)` on host rows,
    `Context.attach_track` for every step of a context; `flush` at end of stream.  use_prior: hits are those of the species a Prior
    admits, on its (reranked) confidence.  Events come back as EVENT_DTYPE arrays sorted by (source, species, first_window)."""

    def __init__(self, device: int, n_sources: int, n_species: int, enter_conf: float, min_hits: int = 1, max_gap: int = 0, max_events: int = 4096,
                 use_prior: bool = False, flags: Optional[int] = None):
        if flags is None:
            flags = BN_TRACK_PRIOR if use_prior else 0
        h = C.c_void_p()
        st = lib.bn_track_create(device, n_sources, n_species, C.c_float(enter_conf), min_hits, max_gap, max_events, flags, C.byref(h))
        if st:
            raise EngineError(st)
        self._h, self.max_events = h, max_events

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_track_free(self._h)
            self._h = None

    def close(self):
        self.__del__()

    @property
    def n_sources(self) -> int:
        return int(lib.bn_track_sources(self._h))

    @property
    def n_species(self) -> int:
        return int(lib.bn_track_species(self._h))

    def open_events(self, source: int = -1) -> int:
        """bn_track_open_events: (source, species) records with an open event, of one source or of all."""
        return int(lib.bn_track_open_events(self._h, source))

    def update(self, logits, sources, windows, prior: Optional["Prior"] = None, sites=None, cap: Optional[int] = None):
        """bn_track_update_host: one update with host logits [rows, n_species], row r being window windows[r] of source sources[r] (at
        site sites[r] of `prior` under use_prior).  Returns (events, dropped)."""
        x = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1, self.n_species)
        sv = np.ascontiguousarray(sources, dtype=np.int32).reshape(-1)
        wv = np.ascontiguousarray(windows, dtype=np.uint64).reshape(-1)
        if sv.shape[0] != x.shape[0] or wv.shape[0] != x.shape[0]:
            raise ValueError("one source and one window per row")
        tv = None if sites is None else np.ascontiguousarray(sites, dtype=np.int32).reshape(-1)
        if tv is not None and tv.shape[0] != x.shape[0]:
            raise ValueError("one site per row")
        cap = self.max_events if cap is None else cap
        out = np.empty(max(cap, 1), dtype=EVENT_DTYPE)
        n, dr = C.c_size_t(), C.c_size_t()
        st = lib.bn_track_update_host(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0], sv.ctypes.data_as(C.POINTER(C.c_int32)),
                                      wv.ctypes.data_as(C.POINTER(C.c_uint64)), None if prior is None else prior._h,
                                      None if tv is None else tv.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(C.POINTER(BnEvent)), cap,
                                      C.byref(n), C.byref(dr))
        if st:
            raise EngineError(st)
        return out[:n.value].copy(), int(dr.value)

    def flush(self, source: int = -1, cap: Optional[int] = None):
        """bn_track_flush: close every open event of a source (-1: of all sources).  Returns (events, dropped)."""
        cap = self.max_events if cap is None else cap
        out = np.empty(max(cap, 1), dtype=EVENT_DTYPE)
        n, dr = C.c_size_t(), C.c_size_t()
        st = lib.bn_track_flush(self._h, source, out.ctypes.data_as(C.POINTER(BnEvent)), cap, C.byref(n), C.byref(dr))
        if st:
            raise EngineError(st)
        return out[:n.value].copy(), int(dr.value)

    def reset(self, source: int):
        """bn_track_reset: forget the source's open events and its last window."""
        st = lib.bn_track_reset(self._h, source)
        if st:
            raise EngineError(st)


class Live:
    """bn_live: a device-resident pool of per-source ring buffers for continuous audio.  Push int16 / float32 PCM as it arrives;
    Context.step_live batches the ready windows of all sources, cut on the device (chunk_audio per source)."""

    def __init__(self, device: int, n_sources: int, segment_samples: int, step_samples: int, ring_samples: int, fmt: int = BN_PCM_I16,
                 dst_rate: Optional[int] = None, src_rates=None, zero_crossings: int = 0, layout=None):
        """dst_rate and src_rates (one rate in Hz per source) given: a resampling pool (bn_live_create_rates) -- pushes arrive at
        the sources' own rates and are converted to dst_rate on the device; segment / step / ring stay in dst_rate samples.
        layout = (format, channels, channel): bn_live_create_layout -- pushes are interleaved frames (bytes or any contiguous
        array) and count frames; with or without src_rates."""
        h = C.c_void_p()
        self._frame_bytes = 0
        if layout is not None:
            if (src_rates is None) != (dst_rate is None):
                raise ValueError("a resampling pool needs both dst_rate and src_rates")
            lay = BnPcmLayout(*layout)
            fmt = lay.format
            self._frame_bytes = PCM_SAMPLE_BYTES.get(lay.format, 1) * max(int(lay.channels), 1)
            rates = None if src_rates is None else np.ascontiguousarray(src_rates, dtype=np.uint32).reshape(-1)
            if rates is not None and rates.shape[0] != n_sources:
                raise ValueError("src_rates needs one rate per source")
            st = lib.bn_live_create_layout(device, n_sources, C.byref(lay), C.sizeof(lay), segment_samples, step_samples, ring_samples, dst_rate or 0,
                                           None if rates is None else rates.ctypes.data_as(C.POINTER(C.c_uint32)), zero_crossings, C.byref(h))
        elif src_rates is None and dst_rate is None:
            st = lib.bn_live_create(device, n_sources, fmt, segment_samples, step_samples, ring_samples, C.byref(h))
        else:
            if src_rates is None or dst_rate is None:
                raise ValueError("a resampling pool needs both dst_rate and src_rates")
            rates = np.ascontiguousarray(src_rates, dtype=np.uint32).reshape(-1)
            if rates.shape[0] != n_sources:
                raise ValueError("src_rates needs one rate per source")
            st = lib.bn_live_create_rates(device, n_sources, fmt, segment_samples, step_samples, ring_samples, dst_rate,
                                          rates.ctypes.data_as(C.POINTER(C.c_uint32)), zero_crossings, C.byref(h))
        if st:
            raise EngineError(st)
        self._h, self.device, self.n_sources, self.format = h, device, n_sources, fmt
        self.segment_samples, self.step_samples, self.ring_samples = segment_samples, step_samples, ring_samples
        self._dtype = np.int16 if fmt == BN_PCM_I16 else np.float32

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bn_live_free(self._h)
            self._h = None

    def free(self):
        self.__del__()

    def _pcm(self, samples):
        """the array a push hands over and the count it names: samples, or frames of a layout pool"""
        if self._frame_bytes:
            a = np.frombuffer(samples, dtype=np.uint8) if isinstance(samples, (bytes, bytearray, memoryview)) else np.ascontiguousarray(samples).reshape(-1).view(np.uint8)
            if a.shape[0] % self._frame_bytes:
                raise ValueError(f"{a.shape[0]} bytes are no whole number of {self._frame_bytes}-byte frames")
            return a, a.shape[0] // self._frame_bytes
        a = np.ascontiguousarray(samples, dtype=self._dtype).reshape(-1)
        return a, a.shape[0]

    def push(self, source: int, samples):
        a, n = self._pcm(samples)
        st = lib.bn_live_push(self._h, source, a.ctypes.data_as(C.c_void_p), n)
        if st:
            raise EngineError(st)

    def push_many(self, sources, chunks):
        """One call for many chunks: chunk i goes to sources[i]; refused whole if any chunk exceeds its source's room."""
        pairs = [self._pcm(c) for c in chunks]
        arrs = [a for a, _ in pairs]
        n = len(arrs)
        src = (C.c_int32 * max(n, 1))(*[int(s) for s in sources])
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[k for _, k in pairs])
        st = lib.bn_live_push_many(self._h, n, src, ptrs, lens)
        if st:
            raise EngineError(st)

    def close(self, source: int):
        st = lib.bn_live_close(self._h, source)
        if st:
            raise EngineError(st)

    def reset(self, source: int):
        st = lib.bn_live_reset(self._h, source)
        if st:
            raise EngineError(st)

    def ready(self, source: int = -1) -> int:
        return int(lib.bn_live_ready(self._h, source))

    def source_rate(self, source: int) -> int:
        """bn_live_source_rate: the rate a source of a resampling pool was created with (0 for a plain pool)."""
        return int(lib.bn_live_source_rate(self._h, source))

    def room(self, source: int) -> int:
        return int(lib.bn_live_room(self._h, source))

    def event_count(self) -> int:
        """bn_live_event_count: HIP events held for scatter / gather ordering (bounded by the steps in flight)."""
        return int(lib.bn_live_event_count(self._h))

    def read_window(self, source: int, window: int) -> np.ndarray:
        out = np.empty(self.segment_samples, dtype=np.float32)
        st = lib.bn_live_read_window(self._h, source, window, out.ctypes.data_as(C.POINTER(C.c_float)))
        if st:
            raise EngineError(st)
        return out


# ---- range filter (reference src/rangefilter.rs) ----
@dataclass
class LocationScore:
    species: str
    score: float
    index: int


def calculate_week(month: int, day: int) -> float:
    return float(lib.bnh_calculate_week(month, day))


def validate_coordinates(latitude: float, longitude: float) -> None:
    err = BnhError()
    if lib.bnh_validate_coordinates(C.c_float(latitude), C.c_float(longitude), C.byref(err)):
        raise Error(err)


def validate_date(month: int, day: int) -> None:
    err = BnhError()
    if lib.bnh_validate_date(month, day, C.byref(err)):
        raise Error(err)


def filter_predictions(predictions: list, location_scores: list, threshold: float, rerank: bool) -> list:
    """filter_predictions_impl (rangefilter.rs:333-386) through the compiled C++ mirror."""
    n, m = len(predictions), len(location_scores)
    ps = (C.c_char_p * max(n, 1))(*[p.species.encode() for p in predictions])
    pc = (C.c_float * max(n, 1))(*[p.confidence for p in predictions])
    ls = (C.c_char_p * max(m, 1))(*[s.species.encode() for s in location_scores])
    lc = (C.c_float * max(m, 1))(*[s.score for s in location_scores])
    pos = (C.c_uint32 * max(n, 1))()
    conf = (C.c_float * max(n, 1))()
    k = lib.bnh_filter_predictions(ps, pc, n, ls, lc, m, C.c_float(threshold), 1 if rerank else 0, pos, conf)
    return [Prediction(predictions[pos[i]].species, float(conf[i]), predictions[pos[i]].index) for i in range(k)]


class RangeFilter:
    """reference src/rangefilter.rs:395-580; the meta model runs on the MI355X (BN_MODEL_GENERIC)."""

    def __init__(self, handle, threshold: float):
        self._h = handle
        self.threshold = threshold

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib.bnh_range_filter_free(self._h)
            self._h = None

    @staticmethod
    def builder() -> "RangeFilterBuilder":
        return RangeFilterBuilder()

    def predict(self, latitude: float, longitude: float, month: int, day: int) -> list:
        err, n = BnhError(), C.c_size_t()
        cap = 1 << 16
        idx = (C.c_uint32 * cap)()
        sc = (C.c_float * cap)()
        if lib.bnh_range_filter_predict(self._h, C.c_float(latitude), C.c_float(longitude), month, day, idx, sc, cap, C.byref(n), C.byref(err)):
            raise Error(err)
        return [LocationScore(lib.bnh_range_filter_label(self._h, idx[i]).decode(), float(sc[i]), int(idx[i])) for i in range(min(n.value, cap))]

    def scores(self, latitude: float, longitude: float, month: int, day: int) -> np.ndarray:
        """The meta model's raw output row for (lat, lon, week), in meta-model order: predict's validation and week rule, no threshold."""
        err, n = BnhError(), C.c_size_t()
        cap = 1 << 16
        sc = np.zeros(cap, dtype=np.float32)
        if lib.bnh_range_filter_scores(self._h, C.c_float(latitude), C.c_float(longitude), month, day, sc.ctypes.data_as(C.POINTER(C.c_float)), cap,
                                       C.byref(n), C.byref(err)):
            raise Error(err)
        return sc[:min(n.value, cap)].copy()

    def prior_row(self, classifier_labels: list, latitude: float, longitude: float, month: int, day: int) -> np.ndarray:
        """One row of a Prior's table: the score of every classifier label in classifier order, BN_PRIOR_UNKNOWN where the meta model
        lacks the label."""
        err = BnhError()
        labels = (C.c_char_p * max(len(classifier_labels), 1))(*[x.encode() for x in classifier_labels])
        row = np.zeros(max(len(classifier_labels), 1), dtype=np.float32)
        if lib.bnh_range_filter_prior_row(self._h, labels, len(classifier_labels), C.c_float(latitude), C.c_float(longitude), month, day,
                                          row.ctypes.data_as(C.POINTER(C.c_float)), C.byref(err)):
            raise Error(err)
        return row[:len(classifier_labels)].copy()

    def filter_predictions(self, predictions: list, location_scores: list, rerank: bool) -> list:
        return filter_predictions(predictions, location_scores, self.threshold, rerank)

    def filter_batch_predictions(self, predictions_batch: list, location_scores: list, rerank: bool) -> list:
        return [filter_predictions(p, location_scores, self.threshold, rerank) for p in predictions_batch]


class RangeFilterBuilder:
    """reference src/rangefilter.rs:142-277."""

    def __init__(self):
        self._model_path = None
        self._labels_path = None
        self._labels = None
        self._threshold = 0.01
        self._device = 0

    def model_path(self, p: str):
        self._model_path = p
        return self

    def labels_path(self, p: str):
        self._labels_path, self._labels = p, None
        return self

    def labels(self, l: list):
        self._labels, self._labels_path = list(l), None
        return self

    def from_classifier_labels(self, l: list):
        return self.labels(l)

    def threshold(self, t: float):
        self._threshold = t
        return self

    def with_rocm(self, device: int = 0):
        self._device = device
        return self

    def build(self) -> RangeFilter:
        h, err = C.c_void_p(), BnhError()
        labels = None
        if self._labels is not None:
            labels = (C.c_char_p * max(len(self._labels), 1))(*[x.encode() for x in self._labels])
        st = lib.bnh_range_filter_build(self._model_path.encode() if self._model_path else None,
                                        self._labels_path.encode() if self._labels_path else None, labels,
                                        len(self._labels) if self._labels is not None else 0, C.c_float(self._threshold), self._device,
                                        C.byref(h), C.byref(err))
        if st:
            raise Error(err)
        return RangeFilter(h, self._threshold)


def live_resampled_samples(src_rate: int, dst_rate: int, pushed: int, closed: bool = False, zero_crossings: int = 0) -> int:
    """bn_live_resampled_samples: outputs of a resampling live source that are final after `pushed` source samples (closed: all
    of them, the length of the resampled recording) -- host arithmetic, needs no device."""
    return int(lib.bn_live_resampled_samples(src_rate, dst_rate, zero_crossings, pushed, 1 if closed else 0))


def resample_table(src_rate: int, dst_rate: int, zero_crossings: int = 0):
    """The resampler's polyphase table [L, T] and (L, M, T) -- host arithmetic, needs no device."""
    L, M, T = C.c_uint32(), C.c_uint32(), C.c_uint32()
    n = lib.bn_resample_table(src_rate, dst_rate, zero_crossings, None, 0, C.byref(L), C.byref(M), C.byref(T))
    tab = np.zeros(n, dtype=np.float32)
    lib.bn_resample_table(src_rate, dst_rate, zero_crossings, tab.ctypes.data_as(C.POINTER(C.c_float)), n, C.byref(L), C.byref(M), C.byref(T))
    return tab.reshape(L.value, T.value), L.value, M.value, T.value


def topk_host(logits: np.ndarray, top_k: int, min_confidence: Optional[float] = None, device: int = 0):
    """top_k_predictions (reference src/postprocess.rs:40-87) on the GPU for host logits [rows, n]."""
    a = np.ascontiguousarray(logits, dtype=np.float32)
    if a.ndim == 1:
        a = a[None, :]
    rows, n = a.shape
    k = max(min(top_k, n), 1)
    idx = np.zeros((rows, k), dtype=np.uint32)
    conf = np.zeros((rows, k), dtype=np.float32)
    cnt = np.zeros(rows, dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    st = lib.bn_topk_host(device, a.ctypes.data_as(C.POINTER(C.c_float)), rows, n, min(top_k, 2 ** 63 - 1),
                          *_min_args(min_confidence), k,
                          idx.ctypes.data_as(u32p), conf.ctypes.data_as(C.POINTER(C.c_float)), cnt.ctypes.data_as(u32p))
    if st:
        raise EngineError(st)
    return idx, conf, cnt


class Group:
    """bn_group: one model replica per device, a recording sharded by window across them, results all-gathered on the
    devices (RCCL between distinct devices, device copies between ranks that share one)."""

    def __init__(self, models, max_batch: int = 32, contexts_per_device: int = 4):
        self.models = list(models)
        n = len(self.models)
        hs = (C.c_void_p * n)(*[m._h for m in self.models])
        devs = (C.c_int32 * n)(*[m.device for m in self.models])
        h = C.c_void_p()
        st = lib.bn_group_create(hs, devs, n, max_batch, contexts_per_device, C.byref(h))
        if st:
            raise RuntimeError(f"bn_group_create: status {st}: {group_last_error()}")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib.bn_group_destroy(self._h)
            self._h = None

    def size(self) -> int:
        return lib.bn_group_size(self._h)

    def uses_rccl(self) -> bool:
        return bool(lib.bn_group_uses_rccl(self._h))

    def stats(self) -> dict:
        """bn_group_get_stats: the contexts' counters summed (capture_fallbacks must be 0)."""
        st = BnCtxStats()
        if lib.bn_group_get_stats(self._h, C.byref(st), C.sizeof(st)):
            raise RuntimeError(group_last_error())
        d = {k: int(getattr(st, k)) for k, _ in BnCtxStats._fields_ if k != "last_fallback"}
        d["last_fallback"] = st.last_fallback.decode(errors="replace")
        return d

    def analyze_recording(self, samples: np.ndarray, step_samples: int, top_k: int = 10, min_confidence: Optional[float] = None,
                          want_logits: bool = True):
        """(logits or None, idx, conf, count) for every window of the recording, in time order.  The default gathers the
        [G, N] logits too (the reference's `raw_scores`, classifier.rs:907,948); want_logits=False is the lighter opt-in that
        gathers the packed top-K rows only (the logits slab is then not even allocated)."""
        x = np.ascontiguousarray(samples)
        fmt = {np.dtype(np.int16): 0, np.dtype(np.float32): 1}[x.dtype]
        cfg = self.models[0].config
        G = lib.bn_chunk_count(x.shape[0], step_samples)
        N = int(cfg.num_species)
        k = min(top_k, N)
        f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        logits = np.empty((G, N), dtype=np.float32) if want_logits else None
        idx, conf, cnt = np.zeros((G, max(k, 1)), dtype=np.uint32), np.zeros((G, max(k, 1)), dtype=np.float32), np.zeros(G, dtype=np.uint32)
        ng = C.c_size_t(0)
        st = lib.bn_group_analyze_recording(self._h, x.ctypes.data_as(C.c_void_p), x.shape[0], fmt, step_samples, top_k,
                                            *_min_args(min_confidence),
                                            None if logits is None else logits.ctypes.data_as(f32p), max(k, 1), idx.ctypes.data_as(u32p),
                                            conf.ctypes.data_as(f32p), cnt.ctypes.data_as(u32p), C.byref(ng))
        if st:
            raise RuntimeError(f"bn_group_analyze_recording: status {st}: {group_last_error()}")
        assert ng.value == G
        return logits, idx[:, :k], conf[:, :k], cnt


def group_last_error() -> str:
    buf = C.create_string_buffer(1024)
    lib.bn_group_last_error(buf, 1024)
    return buf.value.decode(errors="replace")


def plan_describe(path: str, model_type: int = -1, all_outputs: bool = False) -> str:
    st = C.c_int32()
    n = lib.bn_plan_describe(path.encode(), model_type, 1 if all_outputs else 0, None, 0, C.byref(st))
    if st.value:
        raise EngineError(st.value)
    buf = C.create_string_buffer(n + 1)
    lib.bn_plan_describe(path.encode(), model_type, 1 if all_outputs else 0, buf, n + 1, C.byref(st))
    return buf.value.decode()


SHARING_AUTO, SHARING_ALONE, SHARING_SHARED = -1, 0, 1


def set_sharing_mode(mode: int) -> None:
    """bn_set_sharing_mode: grids sized for a device of the caller's own (0, the default), a shared one (1), or by the number of live
    contexts (-1).  Results are bit-identical in every mode."""
    lib.bn_set_sharing_mode(int(mode))


def model_survey(path: str):
    """bn_model_survey: (status, text).  Needs no device.  status 0 = every plan accepted, BN_ERR_UNSUPPORTED_MODEL = a plan refused
    (the text says which node and why); an unreadable file raises."""
    st = C.c_int32()
    n = lib.bn_model_survey(path.encode(), None, 0, C.byref(st))
    if n == 0 and st.value:
        raise EngineError(st.value)
    buf = C.create_string_buffer(n + 1)
    lib.bn_model_survey(path.encode(), buf, n + 1, C.byref(st))
    return st.value, buf.value.decode()


def parse_labels(content: str, csv: bool) -> list:
    n = lib.bnh_parse_labels(content.encode("utf-8"), 1 if csv else 0, None, 0)
    buf = C.create_string_buffer(max(n, 1))
    lib.bnh_parse_labels(content.encode("utf-8"), 1 if csv else 0, buf, max(n, 1))
    s = buf.value.decode("utf-8")
    return s.split("\n") if s else []


class LabelFormat(enum.IntEnum):
    """reference src/types.rs LabelFormat."""
    Text = 0
    Csv = 1
    Json = 2


def parse_labels_format(content: str, fmt: "LabelFormat") -> list:
    """parse_labels (reference src/labels.rs:33-39) through the compiled C++ mirror; raises Error(LabelParse)."""
    err = BnhError()
    raw = content.encode("utf-8")
    n = lib.bnh_parse_labels_format(raw, int(fmt), None, 0, C.byref(err))
    if n == 0:
        raise Error(err)
    buf = C.create_string_buffer(n)
    lib.bnh_parse_labels_format(raw, int(fmt), buf, n, C.byref(err))
    s = buf.raw[:n - 1].decode("utf-8")
    return s.split("\x1f") if s else []


def chunk_plan(n_samples: int, segment_samples: int, overlap_secs: float, sample_rate: int):
    n = lib.bnh_chunk_plan(n_samples, segment_samples, C.c_float(overlap_secs), sample_rate, None, None, 0)
    starts = np.zeros(max(n, 1), dtype=np.uint64)
    times = np.zeros(max(n, 1), dtype=np.float32)
    lib.bnh_chunk_plan(n_samples, segment_samples, C.c_float(overlap_secs), sample_rate,
                       starts.ctypes.data_as(C.POINTER(C.c_uint64)), times.ctypes.data_as(C.POINTER(C.c_float)), n)
    return starts[:n], times[:n]


def device_count() -> int:
    return lib.bn_device_count()
