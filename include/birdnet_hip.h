/*
 * birdnet_hip.h -- C ABI of libbirdnet_hip.so, the MI355X-native (gfx950 / HIP)
 * replacement for the ONNX Runtime session behind the reference's
 * Classifier::predict / predict_batch / BatchInferenceContext path.
 *
 * The reference (tphakala/rust-birdnet-onnx, crate birdnet-onnx 2.0.0-rc.5) has
 * no FFI of its own; its seam is the safe `ort` crate API.  Every entry point
 * below names the `ort` call site (file:line under the reference tree) it
 * stands in for.  Plain pointers and sizes only; no C++/torch types.
 *
 * Threading: a bn_model is immutable after load and may be shared between
 * threads; a bn_ctx owns one HIP stream plus its buffers and must be used by
 * one thread at a time (same contract as BatchInferenceContext,
 * src/batch_context.rs:56-60).
 *
 * Errors: every call returns a bn_status; the message of the last failure on
 * the calling thread is available from bn_last_error().
 */
#ifndef BIRDNET_HIP_H
#define BIRDNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BN_ABI_VERSION 2 /* 2: bn_model_get_cost / bn_ctx_get_stats take the caller's struct size; bn_ctx_get_stats, bn_group_get_stats */
#define BN_MAX_OUTPUTS 8
#define BN_MAX_RANK 6
#define BN_NAME_LEN 64

typedef struct bn_model bn_model; /* stands in for ort::session::Session (src/classifier.rs:340-350,435) */
typedef struct bn_ctx bn_ctx;     /* stands in for ort IoBinding + buffers (src/batch_context.rs:70-85) */

typedef enum bn_status {
    BN_OK = 0,
    BN_ERR_INVALID_ARG = 1,       /* NULL handle, B > max_batch, bad index ... */
    BN_ERR_BAD_SIZE = 2,          /* reserved: size checks live in the host shim (classifier.rs:612-618,688-696) */
    BN_ERR_TIMEOUT = 3,           /* -> Error::Timeout   (classifier.rs:568-573) */
    BN_ERR_CANCELLED = 4,         /* -> Error::Cancelled (classifier.rs:568-573) */
    BN_ERR_BACKEND = 5,           /* HIP runtime failure -> Error::Inference(String) */
    BN_ERR_MODEL_LOAD = 6,        /* unreadable / malformed .onnx -> Error::ModelLoad */
    BN_ERR_UNSUPPORTED_MODEL = 7, /* graph uses an operator/shape outside the native subset */
    BN_ERR_MODEL_DETECTION = 8,   /* -> Error::ModelDetection{reason} (detection.rs:15-145) */
    BN_ERR_NO_DEVICE = 9          /* no usable gfx950 device: the path never falls back to CPU */
} bn_status;

/* ModelType (src/types.rs:3-11) */
typedef enum bn_model_type {
    BN_MODEL_BIRDNET_V24 = 0,
    BN_MODEL_BIRDNET_V30 = 1,
    BN_MODEL_PERCH_V2 = 2,
    /* Not an audio model: no detection rules, output 0 is the result.  Used for the range filter's
     * meta model ((lat, lon, week) -> per-species prior, src/rangefilter.rs:451-496); only valid as
     * model_type_override.  sample_count = elements per input row, num_species = last dim of output 0. */
    BN_MODEL_GENERIC = 100
} bn_model_type;

/* Tensor metadata: what session.inputs()/outputs() + dtype().tensor_shape()
 * return (src/classifier.rs:387-420).  A dynamic dimension is reported as -1. */
typedef struct bn_io_info {
    int32_t input_rank;
    int64_t input_shape[BN_MAX_RANK];
    char input_name[BN_NAME_LEN];
    int32_t n_outputs;
    int32_t output_rank[BN_MAX_OUTPUTS];
    int64_t output_shape[BN_MAX_OUTPUTS][BN_MAX_RANK];
    char output_name[BN_MAX_OUTPUTS][BN_NAME_LEN];
} bn_io_info;

/* ModelConfig (src/types.rs:72-85) + which graph outputs carry logits /
 * embeddings (src/classifier.rs:917-934: v2.4 -> 0; v3.0 -> 1,0; Perch -> 3,0). */
typedef struct bn_model_config {
    int32_t model_type; /* bn_model_type */
    uint32_t sample_rate;
    float segment_duration;
    uint64_t sample_count;
    uint64_t num_species;
    int32_t has_embedding;
    uint64_t embedding_dim;
    int32_t logits_output;    /* graph output index of the logits */
    int32_t embedding_output; /* graph output index of the embeddings, -1 if none */
} bn_model_config;

/* Work the loaded graph costs per segment, from the engine's own graph walk
 * (denominators for roofline reporting). */
typedef struct bn_model_cost {
    double macs_mfma;          /* multiply-accumulates issued on matrix cores (1x1 conv / conv1d / FC) */
    double macs_valu;          /* multiply-accumulates on the vector ALU (depthwise, stem conv) */
    double weight_bytes;       /* resident parameter bytes after folding/pruning */
    double activation_bytes;   /* bytes of intermediates written to HBM per segment by the current plan */
    int32_t n_launches;        /* kernel launches per batch in the current plan */
    /* The front end's windowed-DFT filter banks (+ absorbed mel product) counted two ways, SURVEY.md 8(d):
     * multiply-accumulates of the matrix-product evaluation the exporter's graph spells out, and flops of the
     * FFT formulation the plan runs where it can (2.5 L log2 L per real frame + 2 per mel non-zero); both 0
     * when the graph has no such bank.  macs_valu contains fft_flops / 2 for banks that run as FFTs. */
    double dft_gemm_macs;
    double fft_flops;
    /* what the current plan spends on those banks (folded matrix product: half the taps; FFT: fft_flops / 2), and the
     * real-FFT flop count of the same frames (2.5 L log2 L each) whichever way they run: a roofline quoted on
     * 2 x (macs_mfma + macs_valu) counts the former ("flops performed"); replacing it by the latter gives the
     * FFT-normalised count SURVEY.md 8(d) prices the front end at. */
    double dft_performed_macs;
    double dft_fft_equiv_flops;
    /* (appended in round 4; callers pass their struct size) multiply-accumulates of macs_mfma that are RECOMPUTE: the fused
     * MBConv launches expand the halo rows / columns of neighbouring bands and strips again (and the padded k of an opt-in
     * configuration); 2 x (macs_mfma - recompute_macs + macs_valu) is the work the graph asks for. */
    double recompute_macs;
} bn_model_cost;

/* ---- version / device ------------------------------------------------- */
int32_t bn_abi_version(void);
/* Number of visible HIP devices whose arch is gfx950 (0 => every load fails with BN_ERR_NO_DEVICE). */
int32_t bn_device_count(void);

/* ---- model load: Session::builder()...commit_from_file(path)  (classifier.rs:340-350) ---- */
/* model_type_override: -1 for auto-detection, else a bn_model_type (ClassifierBuilder::model_type).
 * The BN_* environment switches (diagnostic A/B knobs) are read when the plan is built AND by the
 * launchers' shape checks: they must not change between bn_model_load and the last launch of that model's contexts.  The
 * plan forms of round 4 (quarter fold, folded GEMMs with absorbed chains, pooled epilogue) have no generic fallback kernel,
 * so a switch flipped in between is a launch error (BN_ERR_BACKEND), never a silently different result. */
bn_status bn_model_load(const char *onnx_path, int32_t device, int32_t model_type_override,
                        bn_model **out);
bn_status bn_model_load_buffer(const void *onnx_bytes, size_t len, int32_t device,
                               int32_t model_type_override, bn_model **out);
/* Drops the caller's reference.  Contexts created from the model keep it alive: the order of
 * bn_model_free and bn_ctx_destroy does not matter (the reference's BatchInferenceContext is an owned
 * value, src/batch_context.rs:70-85). */
void bn_model_free(bn_model *m);
/* HIP device ordinal the model was loaded on (device_id of the reference's GPU configs, cuda_config.rs:179-182); -1 for NULL. */
int32_t bn_model_device(const bn_model *m);
/* session.inputs()/outputs() metadata (classifier.rs:387-420) */
bn_status bn_model_io_info(const bn_model *m, bn_io_info *out);
/* detect_model_type() result for the loaded graph (detection.rs:15-145) */
bn_status bn_model_get_config(const bn_model *m, bn_model_config *out);
/* struct_size = sizeof(bn_model_cost) as the CALLER was compiled: at most that many bytes are written, so a caller
 * built against a shorter struct keeps working when fields are appended. */
bn_status bn_model_get_cost(const bn_model *m, bn_model_cost *out, size_t struct_size);

/* The same detection rules exposed on raw shapes, for shims that keep
 * detection on their side (detection.rs:15-80; override < 0 means None).
 * out_shapes is the concatenation of all output shapes, out_ranks their ranks. */
bn_status bn_detect_model_type(const int64_t *in_shape, size_t in_rank, const int64_t *out_shapes,
                               const size_t *out_ranks, size_t n_out, int32_t model_type_override,
                               bn_model_config *out);

/* ---- context: session.create_binding() + vec![0f32; max*S]  (batch_context.rs:102-133) ---- */
#define BN_CTX_DEFAULT 0u
#define BN_CTX_ALL_OUTPUTS 1u /* also compute graph outputs the reference discards (Perch 1,2) */
#define BN_CTX_NO_GRAPH 2u    /* launch kernels eagerly instead of replaying a captured hipGraph */
bn_status bn_ctx_create(bn_model *m, size_t max_batch, uint32_t flags, bn_ctx **out);
void bn_ctx_destroy(bn_ctx *c);
size_t bn_ctx_max_batch(const bn_ctx *c);
/* How the context's plans reached the stream so far.  A plan is captured into a hipGraph once per (batch size, input
 * buffer) and replayed; every LDS opt-in and allocation the launches need happens at bn_ctx_create, so a capture holds
 * kernel launches only.  Should a capture still fail, that batch runs launch by launch, the event is COUNTED here
 * (capture_fallbacks, with the runtime's message in last_fallback) and printed to stderr once per context;
 * BN_STRICT_GRAPH=1 in the environment makes it BN_ERR_BACKEND instead.  capture_fallbacks must read 0 in a
 * healthy process. */
typedef struct bn_ctx_stats {
    uint64_t captures;          /* hipStreamBeginCapture..EndCapture runs */
    uint64_t instantiates;      /* hipGraphInstantiate calls */
    uint64_t replays;           /* hipGraphLaunch calls */
    uint64_t eager_runs;        /* plans launched kernel by kernel (BN_CTX_NO_GRAPH, or a failed capture) */
    uint64_t capture_fallbacks; /* captures that did not become a graph */
    uint64_t evictions;         /* instantiated graphs dropped from the 16-entry cache */
    uint64_t cached_graphs;
    char last_fallback[192];
    uint64_t input_copies;      /* device-to-device copies of a caller's batch into the context's own input buffer */
} bn_ctx_stats;
bn_status bn_ctx_get_stats(const bn_ctx *c, bn_ctx_stats *out, size_t struct_size);
/* Bytes of device memory held by the context (activations arena + I/O buffers). */
size_t bn_ctx_device_bytes(const bn_ctx *c);

/*
 * The hot call: session.run_with_options / run_binding_with_options
 * (classifier.rs:637-639, 721-723, 851-853) together with the host staging of
 * prepare_input (batch_context.rs:188-226) and the output copies of
 * extract_outputs / extract_tensor_data (batch_context.rs:289-338,
 * classifier.rs:1062-1077).
 *
 *   segs        batch_size pointers to sample_count host floats each
 *   logits_out  host [batch_size * num_species]
 *   emb_out     host [batch_size * embedding_dim], or NULL
 *   cancel      optional flag polled while the batch runs (CancellationToken,
 *               inference_options.rs:24-47); non-zero => BN_ERR_CANCELLED
 *   timeout_ns  0 = none; exceeded => BN_ERR_TIMEOUT (RunOptions::terminate,
 *               classifier.rs:527-554).  Granularity is one launch group.
 * batch_size == 0 returns BN_OK and touches nothing (classifier.rs:681-683).
 */
bn_status bn_infer(bn_ctx *c, const float *const *segs, size_t batch_size, float *logits_out,
                   float *emb_out, const volatile int32_t *cancel, uint64_t timeout_ns);

/*
 * The same hot call split in two, so that the host staging and the PCIe upload of batch k+1 overlap the device
 * work of batch k (a synchronous call leaves the GPU idle while the caller's 576 KB per segment are copied and
 * uploaded, and the link idle while the plan runs):
 *
 *   bn_infer_submit   validates, copies the caller's slices into pinned staging (prepare_input,
 *                     batch_context.rs:188-226; a persistent pool of staging threads copies segment by segment
 *                     and every finished chunk goes on the wire while the next is still being copied), enqueues
 *                     the plan, the top-K kernel (top_k > 0: top_k_predictions, postprocess.rs:40-87, with the
 *                     same has_min / min_conf meaning as bn_topk) and the device-to-host copies of logits,
 *                     embeddings and top-K rows, and returns a ticket.  The caller's slices are no longer
 *                     referenced once it returns.
 *   bn_infer_collect  waits for that batch (cancel / timeout_ns as in bn_infer) and copies its results out:
 *                     logits_out [batch * num_species], emb_out [batch * embedding_dim] or NULL, and -- when
 *                     count_out is not NULL -- idx_out / conf_out [batch * k_stride] and count_out [batch] as
 *                     bn_topk writes them (k_stride >= min(top_k, num_species)).
 *
 * A context holds at most TWO submitted batches (a third submit before a collect is BN_ERR_INVALID_ARG);
 * batches complete in submission order.  More batches in flight = more contexts, each on its own stream.
 * A batch that timed out or was cancelled in bn_infer_collect is abandoned: its ticket is gone and the context
 * drains before its next use.  batch_size == 0 yields ticket 0, which collects to nothing.  Same threading rule
 * as every context call: one thread at a time per context.  Tickets share nothing with the synchronous entry points
 * (bn_infer_windows, bn_step_device, bn_step_windows) but the context's stream: each of the two slots owns its device
 * input and pinned staging, so those calls may be mixed with tickets in flight; they run in call order.
 */
bn_status bn_infer_submit(bn_ctx *c, const float *const *segs, size_t batch_size, size_t top_k,
                          int32_t has_min, float min_conf, uint64_t *ticket);
bn_status bn_infer_collect(bn_ctx *c, uint64_t ticket, float *logits_out, float *emb_out,
                           size_t k_stride, uint32_t *idx_out, float *conf_out, uint32_t *count_out,
                           const volatile int32_t *cancel, uint64_t timeout_ns);

/* Same computation with the batch already resident in HBM as one contiguous
 * [batch_size, sample_count] f32 array; outputs stay on the device.
 * d_pcm must be 16-byte aligned (the kernels read it as float4); a pointer that is
 * not is refused with BN_ERR_INVALID_ARG, nothing is launched.
 * Asynchronous on the context's stream unless `sync` is non-zero. */
bn_status bn_infer_device(bn_ctx *c, const float *d_pcm, size_t batch_size, int32_t sync);
/* The context's OWN device input buffer ([max_batch, sample_count] f32, 256-byte aligned).  The plan always reads its batch
 * from here: one hipGraph per batch size, however many buffers a caller cycles through.  bn_infer_device /
 * bn_step_device copy a batch that lives elsewhere in on the context's stream (device to device, ~10 us for 32 x 3 s);
 * a caller that produces its batch directly in this buffer and passes this pointer pays no copy.  The buffer is also
 * what bn_infer_windows / bn_step_windows fill: do not write it while such a call is in flight. */
bn_status bn_ctx_input_device(const bn_ctx *c, float **d_ptr, size_t *capacity_floats);
/* Device pointer and row length of graph output `index` after the last run
 * (row-major [batch, row_elems] f32). */
bn_status bn_ctx_output_device(const bn_ctx *c, int32_t index, const float **d_ptr,
                               size_t *row_elems);
/* Copy graph output `index` of the last run to host: [batch_size * row_elems]. */
bn_status bn_ctx_read_output(bn_ctx *c, int32_t index, size_t batch_size, float *host_out);
/* Block until the context's stream is idle (IoBinding::synchronize_outputs, batch_context.rs:276-281). */
bn_status bn_ctx_synchronize(bn_ctx *c);
/* The context's hipStream_t, for callers that order their own device work after it.  It is a non-blocking stream at the greatest
 * priority the device reports, so that the contexts' streams do not share the default level's hardware queues with the null
 * stream (BN_CTX_STREAM_PRIO=0: default priority). */
void *bn_ctx_stream(const bn_ctx *c);
/* Mean device time per launch group of the last timed run is not kept here;
 * use bn_ctx_time_kernels to measure: runs the plan once for batch_size with a
 * HIP event pair around every launch on the context's stream and writes up to
 * cap (name, microseconds) pairs.  Returns the number of launches. */
size_t bn_ctx_time_kernels(bn_ctx *c, size_t batch_size, char (*names)[BN_NAME_LEN], float *usec,
                           double *macs, double *bytes, size_t cap);
/* The planner's cost figures per launch for batch_size (no device work): multiply-adds on the
 * matrix cores (a fused MBConv launch's expand conv included, with its halo / band recompute),
 * on the vector ALU, the recompute share of the first, and algorithmic bytes (activations in +
 * out + weights).  macs_mfma[k] + macs_valu[k] is what bn_ctx_time_kernels reports as macs[k];
 * summed over the launches they equal bn_model_get_cost's macs_mfma / macs_valu x batch_size.
 * Measurement only; the reference has no counterpart.  Returns the number of
 * launches; arrays may be NULL. */
size_t bn_ctx_launch_costs(const bn_ctx *c, size_t batch_size, double *macs_mfma, double *macs_valu,
                           double *macs_recompute, double *bytes, size_t cap);

/*
 * top_k_predictions (postprocess.rs:40-87) on the device-resident logits of
 * the last run: per row the K = min(top_k, num_species) entries the
 * reference's BinaryHeap keeps, sigmoid (postprocess.rs:91-93), the
 * `confidence >= min_confidence` filter and the stable descending sort.
 * Outputs are host arrays with row stride k_stride >= K:
 *   idx_out[b*k_stride + j], conf_out[b*k_stride + j] for j < count_out[b].
 * has_min == 0 <=> min_confidence == None.
 */
bn_status bn_topk(bn_ctx *c, size_t batch_size, size_t top_k, int32_t has_min, float min_conf,
                  size_t k_stride, uint32_t *idx_out, float *conf_out, uint32_t *count_out);
/* The same kernel on caller-provided device logits [rows, n] (any device buffer). */
bn_status bn_topk_device(int32_t device, const float *d_logits, size_t rows, size_t n, size_t top_k,
                         int32_t has_min, float min_conf, size_t k_stride, uint32_t *idx_out,
                         float *conf_out, uint32_t *count_out);
/* Host logits in, host results out (uploads, runs the kernel, downloads). */
bn_status bn_topk_host(int32_t device, const float *logits, size_t rows, size_t n, size_t top_k,
                       int32_t has_min, float min_conf, size_t k_stride, uint32_t *idx_out,
                       float *conf_out, uint32_t *count_out);

/*
 * One whole pass of the hot path over a device-resident batch, fully asynchronous
 * on the context's stream: the plan (bn_infer_device), the top-K kernel
 * (bn_topk), and the device-to-host copies of the logits rows (raw_scores,
 * classifier.rs:907,948) and of the top-K results into pinned buffers owned by
 * the context.  With sync == 0 the caller overlaps host work and calls
 * bn_ctx_synchronize() before reading bn_step_results().
 */
bn_status bn_step_device(bn_ctx *c, const float *d_pcm, size_t batch_size, size_t top_k,
                         int32_t has_min, float min_conf, int32_t sync);
/* Pinned host views of the last bn_step_device: logits [batch, num_species], idx/conf
 * [batch, k_stride], count [batch].  Valid until the next step on this context. */
bn_status bn_step_results(const bn_ctx *c, const float **logits, const uint32_t **idx,
                          const float **conf, const uint32_t **count, size_t *k_stride);

/*
 * Recording-level ingest: the caller side of the
 * hot path.  The reference CLI reads a 16-bit mono WAV, converts every sample
 * with `f32::from(s) / 32768.0` (src/bin/birdnet-analyze.rs:683-687), cuts it
 * into fixed-length windows with `chunk_audio` (:707-743: step = S -
 * floor(overlap * sample_rate), one window for every pos = k*step < len, the
 * tail zero-padded) and uploads each window as f32.  Here the recording is
 * uploaded ONCE in its storage format (i16: half the PCIe bytes; with overlap no
 * sample crosses the bus twice) and the windows of a batch are materialised on
 * the device, straight into the context's input buffer, by one small kernel in
 * front of the plan.  The conversion is a division by a power of two, so the
 * windows are bit-identical to the reference's.
 */
typedef struct bn_recording bn_recording;
#define BN_PCM_I16 0 /* int16_t mono, value / 32768.0 */
#define BN_PCM_F32 1 /* float mono, used as is */
bn_status bn_recording_create(int32_t device, const void *pcm, size_t n_samples, int32_t format,
                              bn_recording **out);
/* The same, returning at once: a thread of the recording's own uploads `pcm` chunk by chunk (32 MiB; BN_UPLOAD_CHUNK_MB) while
 * the caller already analyses the first windows -- bn_infer_windows / bn_step_windows / bn_recording_windows / bn_recording_read_f32
 * block (on the host) until the last sample they read has arrived, so a loop over the windows in time order overlaps the
 * upload of a long recording with its analysis (a 24 h recording on one GPU: 0.72 s -> the analysis time alone).
 * `pcm` must stay valid and unchanged until bn_recording_wait() has returned or the recording is freed (the reference CLI
 * keeps the whole file in memory for the run, src/bin/birdnet-analyze.rs:653-704). */
bn_status bn_recording_create_async(int32_t device, const void *pcm, size_t n_samples, int32_t format,
                                    bn_recording **out);
/* Blocks until the whole recording is on the device (BN_ERR_BACKEND if the upload failed). */
bn_status bn_recording_wait(const bn_recording *r);
/* Sample-rate conversion front end (the reference CLI refuses a WAV whose rate differs
 * from the model's, src/bin/birdnet-analyze.rs:447-455).  The recording is uploaded in its storage format and
 * converted ON THE DEVICE to f32 at dst_rate by a polyphase windowed-sinc FIR: L/M = dst/src reduced, cutoff
 * 0.5*min(1, L/M) of the source Nyquist band, `zero_crossings` sinc lobes per side (0 => 16) under a Kaiser
 * window (beta 8.6, ~ -90 dB), every phase normalised to unit DC gain.  The result holds
 * ceil(n_samples * L / M) samples and is used like any other recording.  src_rate == dst_rate is a plain upload.
 * There is no reference behaviour to match; the filter design above is the contract (oracle/resample.py). */
bn_status bn_recording_create_resampled(int32_t device, const void *pcm, size_t n_samples, int32_t format,
                                        uint32_t src_rate, uint32_t dst_rate, uint32_t zero_crossings,
                                        bn_recording **out);
/* The polyphase table the resampler uses, for inspection / tests: writes up to cap floats of [L][T] and
 * returns L*T; *L_out, *M_out, *T_out receive the factors.  Needs no device. */
size_t bn_resample_table(uint32_t src_rate, uint32_t dst_rate, uint32_t zero_crossings, float *table, size_t cap,
                         uint32_t *L_out, uint32_t *M_out, uint32_t *T_out);
/* Copy samples [first, first+count) of an f32 recording back to the host (tests, diagnostics).  A recording created with a
 * layout (below) is read in any format: frames [first, first+count) as the f32 samples the layout rule defines. */
bn_status bn_recording_read_f32(const bn_recording *r, size_t first, size_t count, float *host_out);
void bn_recording_free(bn_recording *r);
size_t bn_recording_samples(const bn_recording *r);
/* Number of windows chunk_audio produces for n_samples at this step (0 for an
 * empty recording or step == 0). */
size_t bn_chunk_count(size_t n_samples, size_t step_samples);
/* chunk_audio on the device, copied back: windows [first, first+count) as host
 * f32 [count, segment_samples] (segment_samples % 4 == 0). */
bn_status bn_recording_windows(const bn_recording *r, size_t segment_samples, size_t step_samples,
                               size_t first_window, size_t count, float *host_out);
/* bn_infer over windows [first_window, first_window+count) of the recording
 * (count <= max_batch; the window length is the model's sample_count).  Same
 * outputs, cancel and timeout behaviour as bn_infer. */
bn_status bn_infer_windows(bn_ctx *c, const bn_recording *r, size_t step_samples,
                           size_t first_window, size_t count, float *logits_out, float *emb_out,
                           const volatile int32_t *cancel, uint64_t timeout_ns);

/* bn_step_device over windows of an uploaded recording: window kernel + plan + top-K + D2H of
 * logits and top-K into the context's pinned buffers, asynchronous unless sync != 0; read with
 * bn_step_results after bn_ctx_synchronize.  This is the loop body of a recording analysis
 * (src/bin/birdnet-analyze.rs:556-600) with several contexts in flight. */
bn_status bn_step_windows(bn_ctx *c, const bn_recording *r, size_t step_samples, size_t first_window,
                          size_t count, size_t top_k, int32_t has_min, float min_conf, int32_t sync);

/*
 * PCM layouts: interleaved multi-channel and 8/24/32-bit PCM, converted ON THE DEVICE.  Field recorders and sound cards
 * deliver stereo or 4-channel frames, very often 24-bit packed; with a layout such bytes are uploaded ONCE as they are and
 * every consumer reads them through one rule.  No reference counterpart (the reference CLI takes mono int16 only).
 *
 * A layout is {format, channels, channel}.  PCM is interleaved frames of `channels` samples each, little-endian.  Every
 * count of the API is in FRAMES: a layout recording of n_frames frames has bn_recording_samples() == n_frames, a push of
 * n_samples to a layout pool carries n_samples frames.
 *
 *   format           storage                           f32 sample
 *   BN_PCM_I16 (0)   int16                             v / 32768 (exact)
 *   BN_PCM_F32 (1)   float                             as is (bits preserved, NaN payloads included)
 *   BN_PCM_I24 (2)   3 packed bytes, two's complement  sign-extended, v / 8388608 (exact)
 *   BN_PCM_I32 (3)   int32                             (float)v rounded to nearest even, then * 2^-31 (exact scale)
 *   BN_PCM_U8  (4)   uint8                             (v - 128) / 128 (exact)
 *
 * channels is 1..16.  channel >= 0 selects that channel of every frame (a value >= channels is refused).  channel ==
 * BN_PCM_MIX mixes the frame down: acc = s[0]; acc = acc + s[c] in f32 for c = 1, 2, ... ascending; result = acc * inv with
 * inv = 1.0f / (float)channels rounded once.  No fused multiply-add anywhere in the rule.  With channels == 1 both ops are
 * the identity, and for I16 and F32 the result is bit-identical to the mono entry points above.
 *
 * The invariant: every consumer of a layout recording or pool -- bn_recording_windows, bn_infer_windows, bn_step_windows,
 * bn_recording_read_f32, the resampler, bn_live_push / bn_live_push_many / bn_live_read_window / bn_step_live -- sees exactly
 * the f32 sample the rule defines, so any path over a layout input is BIT-FOR-BIT equal to the same path over a BN_PCM_F32
 * mono input holding the rule's samples (the resampler's FIR arithmetic after the load is the same code).  The tail past
 * n_frames reads 0, as chunk_audio pads.
 *
 * struct_size is sizeof(bn_pcm_layout) as the caller compiled it.  BN_ERR_INVALID_ARG, with a message, and no handle written:
 * an unknown format, channels outside 1..16, channel outside [-1, channels), a NULL layout, a struct_size below the struct's.
 *
 * bn_recording_create_layout_async uploads in chunks (BN_UPLOAD_CHUNK_MB) cut at FRAME boundaries, and otherwise behaves as
 * bn_recording_create_async.  bn_recording_create_layout_resampled converts during its synchronous upload as
 * bn_recording_create_resampled does; its result is mono f32 at dst_rate.
 *
 * bn_recording_view_channel: a second recording over the SAME device bytes with another channel op -- no second upload; use
 * it to analyse both channels of a stereo file.  Either recording may be freed first (an asynchronous upload is joined when
 * the last of them goes).  The channel is checked against the recording's own layout; a resampled recording has no
 * storage-format bytes left -- it is mono f32 -- and accepts only channel 0 or BN_PCM_MIX.
 *
 * Mono only, as before: bn_group_analyze_recording; WAV headers are the caller's to parse.
 */
#define BN_PCM_I24 2 /* 3 packed bytes, little-endian two's complement, value / 8388608.0 */
#define BN_PCM_I32 3 /* int32_t, (float)value * 2^-31 */
#define BN_PCM_U8 4  /* uint8_t, (value - 128) / 128.0 */
#define BN_PCM_MIX (-1)
typedef struct bn_pcm_layout {
    int32_t format;    /* BN_PCM_* */
    uint32_t channels; /* samples per frame, 1..16 */
    int32_t channel;   /* the channel to select, or BN_PCM_MIX */
} bn_pcm_layout;
bn_status bn_recording_create_layout(int32_t device, const void *pcm, size_t n_frames, const bn_pcm_layout *layout,
                                     size_t struct_size, bn_recording **out);
bn_status bn_recording_create_layout_async(int32_t device, const void *pcm, size_t n_frames, const bn_pcm_layout *layout,
                                           size_t struct_size, bn_recording **out);
bn_status bn_recording_create_layout_resampled(int32_t device, const void *pcm, size_t n_frames, const bn_pcm_layout *layout,
                                               size_t struct_size, uint32_t src_rate, uint32_t dst_rate,
                                               uint32_t zero_crossings, bn_recording **out);
bn_status bn_recording_view_channel(const bn_recording *r, int32_t channel, bn_recording **out);

/*
 * Window levels and list steps: analyse CHOSEN windows of many recordings.  No reference counterpart (the reference CLI runs every
 * window of one file in order).  Two workloads: a mostly-quiet archive, where an amplitude gate picks the few windows worth the
 * model (levels -> the host picks -> list steps), and a library of short clips, where one list step fills a batch from many files.
 *
 * bn_recording_levels: out[i] receives the levels of window first_window + i, i < count.  segment_samples, step_samples,
 * first_window and count mean what they mean for bn_recording_windows (segment_samples % 4 == 0; a window k exists iff
 * k * step_samples < bn_recording_samples), and a window's S = segment_samples samples are exactly the f32 values
 * bn_recording_windows returns for it -- the layout rule's samples ("PCM layouts"), zeros past the end.  There is no second
 * sample rule.
 *
 *   peak          max |s| over the window's S samples; exact
 *   mean          (sum s) / S
 *   mean_square   (sum s*s) / S         the divisor is always S, padding included: that is what the model sees
 *   flags         BN_LEVEL_PADDED       iff the window reaches past the last sample (k * step + S > samples)
 *                 BN_LEVEL_NONFINITE    iff any sample is NaN or +-Inf.  Then peak = mean_square = +Inf and mean = 0, whatever the
 *                                       other samples are: such a window is never "quiet" to a gate that compares peak or
 *                                       mean_square against a threshold
 *
 * Arithmetic.  Plain f32 operations, no fused multiply-add (s*s is rounded, then added); every partial sum is f32, in a fixed
 * tree that is a function of S alone (csrc/levels.hip).  BN_LEVEL_SUM_DEPTH is the longest chain of additions any term passes
 * through for S <= 2^20.  From it, against the float64 value of the same f32 samples and barring underflow of s*s:
 *   mean_square   within (BN_LEVEL_SUM_DEPTH + 2) * 2^-24, relative (all terms are non-negative)
 *   mean          within (BN_LEVEL_SUM_DEPTH + 1) * 2^-24 * mean|s|, absolute
 * (derivation in DESIGN.md 7c).
 *
 * Invariance.  A window's four fields depend only on its S samples and on S: not on first_window, count, step_samples, the
 * recording's length or its layout.  The same bits come from an I16 mono recording, an F32 mono recording of the rule's samples
 * and a stereo I24 recording whose mix or selected channel gives those samples, and from any split of a window range into calls.
 *
 * The call blocks (on the host) on an asynchronous upload until the last sample its windows read has arrived, as
 * bn_recording_windows does, and returns when `out` is written.  struct_size is sizeof(bn_window_level) as the caller compiled it;
 * element i of `out` lies at byte offset i * struct_size, and bytes of an element past this header's struct are left alone.
 * BN_ERR_INVALID_ARG, with a message: a NULL recording, a struct_size below the struct's, segment_samples that is 0 or no multiple
 * of 4, step_samples == 0, a window range past the recording's windows, NULL `out` with count > 0.  count == 0 is BN_OK.
 */
#define BN_LEVEL_NONFINITE 1u
#define BN_LEVEL_PADDED 2u
#define BN_LEVEL_SUM_DEPTH 1034 /* 1024 (one of 1024 accumulators over S <= 2^20) + 2 (a lane's four) + 6 (a wave) + 2 (four waves) */
typedef struct bn_window_level {
    float peak;        /* max |s| over the window's S samples */
    float mean;        /* sum s / S */
    float mean_square; /* sum s*s / S */
    uint32_t flags;    /* BN_LEVEL_NONFINITE | BN_LEVEL_PADDED */
} bn_window_level;
bn_status bn_recording_levels(const bn_recording *r, size_t segment_samples, size_t step_samples, size_t first_window,
                              size_t count, bn_window_level *out, size_t struct_size);

/*
 * bn_recording_band_levels: per window, the power inside caller-chosen frequency bands -- the levels a gate needs where wind,
 * traffic or handling noise below a few hundred hertz makes every window "loud" to peak and mean_square.  out[i] receives the
 * bands of window first_window + i; r, segment_samples, step_samples, first_window and count mean what they mean for
 * bn_recording_levels, and a window is the same S = segment_samples f32 samples, zeros past the end.
 *
 * Frames.  A window is cut into frames of N = spec->frame samples every spec->hop samples, all inside the window: frame j covers
 * window positions [j * hop, j * hop + N), n_frames = (S - N) / hop + 1.  The up to hop - 1 trailing positions that no full frame
 * covers are not read: they change no field, not even the non-finite flag.
 * Transform.  A frame x is multiplied by the periodic Hann window w_n = 0.5 - 0.5 cos(2 pi n / N) and transformed:
 * X_k = sum_n w_n x_n exp(-2 pi i k n / N), k = 0 .. N/2.
 * One-sided power.  P_k = c_k |X_k|^2 / (N * sum_n w_n^2), c_k = 1 for k = 0 and k = N/2, 2 otherwise.  sum_k P_k equals
 * sum (w x)^2 / sum w^2, so a bin-centred sine of amplitude A reads A^2 / 2 in its band: the scale of mean_square.
 * A band b is the bin range [bin_lo[b], bin_hi[b]); bands may overlap.  Its power in a frame is the sum of P_k over it; the
 * frame's total the sum over all N/2 + 1 bins.
 *
 *   mean[b], max[b]          the mean and the maximum over the window's frames of band b's power; 0 for b >= n_bands
 *   total_mean, total_max    the same pair for the total
 *   n_frames                 (S - N) / hop + 1
 *   flags                    BN_LEVEL_PADDED as for bn_recording_levels; BN_LEVEL_NONFINITE iff any sample a frame reads is NaN or
 *                            +-Inf: then mean[b] and max[b] of every b < n_bands and both totals are +Inf, so such a window is
 *                            never quiet
 *
 * Arithmetic.  Plain f32, no fused multiply-add, no math-library call on the device: window and twiddles are tables computed in
 * double on the host and rounded once.  A frame is a radix-2 transform of N/2 complex points and the real-input unpack, the bins
 * of a band are added in a fixed tree, the frames in ascending order in one of four chains (csrc/band_levels.hip).  Against the
 * float64 value of the same f32 samples with the double-precision window, with u = 2^-24, eps = BN_BAND_EPS_ULPS * u,
 * delta = (BN_BAND_SUM_DEPTH + ceil(n_frames / 4)) * u, P the reference value of the field and T the reference total_mean (for
 * max[b] and total_max: total_max), barring underflow:
 *   |got - P| <= 2 eps sqrt(P T) + eps^2 T + delta P
 * (derivation in DESIGN.md 7c, "Band levels").
 *
 * Invariance.  A window's record depends only on its S samples, S and the spec: not on first_window, count, step_samples, the
 * recording's length or its layout, nor on how a window range is split into calls.
 *
 * The call blocks on an asynchronous upload until the last sample its frames read has arrived, and returns when `out` is written.
 * spec_size is sizeof(bn_band_spec), struct_size sizeof(bn_window_bands), as the caller compiled them; element i of `out` lies at
 * byte offset i * struct_size and bytes of an element past this header's struct are left alone.  BN_ERR_INVALID_ARG, with a
 * message and nothing enqueued: whatever bn_recording_levels refuses, a NULL spec, a spec_size below the struct's, a frame that is
 * not 256, 512, 1024 or 2048, segment_samples < frame, hop 0 or above frame, n_bands 0 or above BN_BAND_MAX, a band with
 * bin_lo >= bin_hi or bin_hi > frame / 2 + 1.  count == 0 is BN_OK.
 *
 * bn_band_bins (host only, no device): the bins of [lo_hz, hi_hz) at a sample rate -- a recording does not carry its rate.  Bin k
 * lies at k * sample_rate / frame Hz and belongs to the band iff that centre does.  BN_ERR_INVALID_ARG: a rate of 0, a frame not
 * in the list, lo_hz >= hi_hz (or a NaN), a band that holds no bin centre, a NULL output.
 */
#define BN_BAND_MAX 8
#define BN_BAND_EPS_ULPS 80  /* 7 per radix-2 stage * 10 stages at frame 2048 + 2 (window) + 7 (unpack) + 1 (second order) */
#define BN_BAND_SUM_DEPTH 32 /* 17 (a lane's bins) + 6 (a wave) + 2 (four waves) + 7 (squares, scale, division, reference scale) */
typedef struct bn_band_spec {
    uint32_t frame;   /* N: 256, 512, 1024 or 2048 */
    uint32_t hop;     /* 1 .. N */
    uint32_t n_bands; /* 1 .. BN_BAND_MAX */
    uint32_t bin_lo[BN_BAND_MAX]; /* band b is bins [bin_lo[b], bin_hi[b]) */
    uint32_t bin_hi[BN_BAND_MAX]; /* bin_lo[b] < bin_hi[b] <= N/2 + 1 */
} bn_band_spec;
typedef struct bn_window_bands {
    float mean[BN_BAND_MAX]; /* entries >= n_bands are 0 */
    float max[BN_BAND_MAX];
    float total_mean;
    float total_max;
    uint32_t flags; /* BN_LEVEL_NONFINITE | BN_LEVEL_PADDED */
    uint32_t n_frames;
} bn_window_bands;
bn_status bn_recording_band_levels(const bn_recording *r, size_t segment_samples, size_t step_samples, size_t first_window,
                                   size_t count, const bn_band_spec *spec, size_t spec_size, bn_window_bands *out, size_t struct_size);
bn_status bn_band_bins(uint32_t sample_rate, uint32_t frame, double lo_hz, double hi_hz, uint32_t *bin_lo, uint32_t *bin_hi);

/*
 * bn_step_window_list: bn_step_windows over an explicit list.  Row i of the batch is the S = sample_count frames of
 * refs[i].recording from frame refs[i].start on, zeros past the end; start is any frame of the recording, no multiple of any step
 * (a window centred on a peak is fine).  The rows are gathered on the device straight into the context's input buffer -- the
 * recordings of one list may have different layouts -- and everything after the gather is the step of bn_step_windows: the row
 * bits are those bn_step_windows produces for the same samples, the plan's graph is the one of that batch size (capture_fallbacks
 * stays 0), and bn_step_results, bn_step_head_results, bn_step_prior_results, bn_step_index_results and bn_step_track_results read
 * the results as after bn_step_live.  refs[i].source and refs[i].window are what an attached prior (its site map) and tracker see
 * of row i, as bn_step_live's source_out[i] and window_out[i]: per source the tracker takes windows in increasing order, and a row
 * whose window does not exceed its source's last is a stale row, as there.  Nothing of `refs` is read after the call returns.
 *
 * An asynchronously uploaded recording is waited for, on the host, up to the last frame any of its rows reads.
 *
 * struct_size is sizeof(bn_window_ref) as the caller compiled it; element i lies at byte offset i * struct_size.
 * BN_ERR_INVALID_ARG, with a message, before anything is enqueued (the context stays as it was): a NULL context or list,
 * a struct_size below the struct's, count == 0 or count > max_batch, a NULL recording, a recording on another device than the
 * context, start >= bn_recording_samples(recording), a negative source, with a tracker attached a window of 2^31 or more, a top_k
 * that bn_step_device refuses, and whatever an attached prior or tracker refuses of a bn_step_live over these sources (more
 * sources than the site map or the tracker has).
 *
 * bn_recording_window_list: the gathered rows alone, copied back as host f32 [count, segment_samples] (segment_samples % 4 == 0),
 * for tests; source and window are ignored, every recording lies on the first one's device, count == 0 is BN_OK.
 */
typedef struct bn_window_ref {
    const bn_recording *recording;
    uint64_t start;  /* first frame of the window; any value < bn_recording_samples(recording) */
    int32_t source;  /* reported to an attached prior / tracker, as bn_step_live's sources */
    uint64_t window; /* the window number reported to them */
} bn_window_ref;
bn_status bn_step_window_list(bn_ctx *c, const bn_window_ref *refs, size_t count, size_t struct_size, size_t top_k,
                              int32_t has_min, float min_conf, int32_t sync);
bn_status bn_recording_window_list(const bn_window_ref *refs, size_t count, size_t struct_size, size_t segment_samples,
                                   float *host_out);

/* Device view of the packed top-K rows of the last bn_step_device / bn_step_windows on this context:
 * [idx: m*k][conf: m*k (float bits)][count: m] for the m rows and k = min(top_k, num_species) of that step.
 * Valid until the next step; reading it must be ordered after the step on bn_ctx_stream(). */
bn_status bn_ctx_step_device_rows(const bn_ctx *c, const uint32_t **d_rows);

/*
 * Multi-GPU (BASELINE.json configs[4]).  The reference has no multi-device code -- its only
 * knob is device_id (src/cuda_config.rs:179-182, src/tensorrt_config.rs:273-276) -- so the contract is "identical to
 * running every window on one device": windows of chunk_audio (src/bin/birdnet-analyze.rs:707-743) are sharded by
 * contiguous range, rank r of R owns [r * ceil(G/R), min(G, (r+1) * ceil(G/R))) (bn_shard_range).
 *
 * bn_group_create takes one model replica per device (load the same file once per device with bn_model_load) and
 * creates contexts_per_device contexts (streams) of max_batch on each.  bn_group_analyze_recording cuts the recording
 * (host int16 / f32 samples) into windows of the model's sample_count at step_samples, lets every rank upload and
 * analyse only its own slice (one host thread per device inside the call), and assembles the results with ONE
 * all-gather of the [G, num_species] logits (logits_out != NULL) and one of the packed top-K rows (count_out != NULL)
 * -- RCCL ncclAllGather over xGMI when the ranks sit on distinct devices (librccl is loaded on first use), plain
 * device copies when they share one (tests on a single GPU).  Outputs are host arrays in window order:
 * logits_out [G * num_species], idx_out / conf_out [G * k_stride], count_out [G]; *n_windows_out = G.
 * A step of 0 (overlap >= segment) yields G = 0 as chunk_audio does.  Errors: bn_group_last_error().
 */
typedef struct bn_group bn_group;
bn_status bn_group_create(bn_model *const *models, const int32_t *devices, int32_t n, size_t max_batch,
                          int32_t contexts_per_device, bn_group **out);
void bn_group_destroy(bn_group *g);
int32_t bn_group_size(const bn_group *g);
int32_t bn_group_uses_rccl(const bn_group *g);
/* bn_ctx_get_stats summed over every context of the group (last_fallback: the most recent one); capture_fallbacks must be 0. */
bn_status bn_group_get_stats(const bn_group *g, bn_ctx_stats *out, size_t struct_size);
void bn_shard_range(size_t n_windows, int32_t rank, int32_t world, size_t *lo, size_t *hi);
bn_status bn_group_analyze_recording(bn_group *g, const void *pcm, size_t n_samples, int32_t format,
                                     size_t step_samples, size_t top_k, int32_t has_min, float min_conf,
                                     float *logits_out, size_t k_stride, uint32_t *idx_out, float *conf_out,
                                     uint32_t *count_out, size_t *n_windows_out);
size_t bn_group_last_error(char *buf, size_t cap);

/*
 * Embedding index: a device-resident store of L2-normalised f32 embedding rows on one device, answering exact top-M
 * cosine-similarity queries (retrieval over a season of audio: "find the windows that sound like this one").  The
 * reference has embeddings but no search; the contract is what an exact float64 brute-force search returns, up to f32
 * rounding, in a total order that makes results deterministic.
 *
 * Row ids are the append order: appending the windows of bn_infer_windows in order makes the id the window index, so
 * start = id * step / sample_rate as chunk_audio reports it (src/bin/birdnet-analyze.rs:707-743).
 *
 *   Normalisation  stored row = x / sqrt(sum x^2).  A row with zero norm or any non-finite element (or whose f32 sum of
 *                  squares overflows, or whose f32 sum of squares underflows to zero) is stored as zeros, counts toward
 *                  bn_index_size and is never returned.  A query with zero norm or a non-finite element returns
 *                  count = 0.  The "up to f32 rounding" above holds while that sum is a normal f32.
 *   Score          the f32 dot product of the normalised query and the normalised row.  For one (query, row) pair its
 *                  summation order depends only on dim: not on where the row lands in a tile, the number of queries of
 *                  the call, the index size or how the index was appended.
 *   Order          score descending, ties by id ascending (-0.0 == +0.0).  count = min(top_m, eligible rows); entries
 *                  past count are not written.
 *   Limits         1 <= top_m <= 256 and m_stride >= top_m, otherwise BN_ERR_INVALID_ARG.  An append past capacity_rows
 *                  is refused whole (nothing appended, size unchanged).  An empty index returns count = 0.
 *
 * Outputs are host arrays [n_queries * m_stride] (id_out, score_out) and count_out [n_queries].  Errors through
 * bn_last_error().  Threading: one thread at a time per index, like a context.
 */
typedef struct bn_index bn_index;
/* dim >= 1, 1 <= capacity_rows < 2^32 - 1; the slab (capacity x dim rounded up to the scan's k-step) is allocated here */
bn_status bn_index_create(int32_t device, size_t dim, size_t capacity_rows, bn_index **out);
void bn_index_free(bn_index *x);
/* rows appended so far */
size_t bn_index_size(const bn_index *x);
size_t bn_index_dim(const bn_index *x);
/* append n host rows [n * dim]; their ids are *first_id .. *first_id + n - 1 (first_id may be NULL) */
bn_status bn_index_add_host(bn_index *x, const float *rows, size_t n, uint64_t *first_id);
/* append the embedding output of the last run of c (rows 0 .. batch_size-1, batch_size <= that run's batch), device to device,
 * ordered after that run on the context's stream (the call returns without waiting; the index's next use waits for it).
 * Refused, with the index unchanged, for a model without embeddings, a dimension mismatch, a context on another device or a
 * batch_size larger than the last run's. */
bn_status bn_index_add_ctx(bn_index *x, bn_ctx *c, size_t batch_size, uint64_t *first_id);
/* copy stored (normalised) rows [first, first + count) to host [count * dim] */
bn_status bn_index_read(const bn_index *x, uint64_t first, size_t count, float *host_out);
/* top-M by cosine for n_queries host query vectors [n_queries * dim] */
bn_status bn_index_search(bn_index *x, const float *queries, size_t n_queries, size_t top_m, size_t m_stride,
                          uint64_t *id_out, float *score_out, uint32_t *count_out);
/* query by example: the queries are stored rows (used as stored, not normalised again); rows whose id lies within
 * exclude_radius of the query's own id are skipped (exclude_radius < 0: none skipped; 0: the row itself; with overlapping
 * windows the neighbours are near-duplicates).  A query id >= bn_index_size is BN_ERR_INVALID_ARG. */
bn_status bn_index_search_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius,
                              size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out);
/* Row tags: every row carries one tag below BN_INDEX_TAG_LIMIT, 0 until set: a source, a site, a species, a tombstone -- the caller's
 * meaning.  bn_subset_select (below) chooses rows by tag, a match (bn_ctx_attach_index, bn_index_match) and bn_index_search_above return the tags of their hits and bn_index_group_above groups its hits by tag; NOTHING ELSE reads a tag: bn_index_search, bn_index_search_ids, bn_ivf_*,
 * bn_sq8_*, bn_head_fit_index, bn_head_rank_index, bn_index_assign, bn_index_cluster and bn_index_save behave the same, bit for bit, with
 * and without tags.  The plane (two bytes per row of capacity) is allocated by the first bn_index_set_tags / bn_index_fill_tags; an index
 * that never tags pays nothing, and an absent plane reads as zeros.  The index file has no tags: it stays format version 1 and a loaded
 * index has every tag 0; carry tags alongside a file with bn_index_read_tags before the save and bn_index_set_tags after the load.
 * bn_index_set_tags gives rows [first_id, first_id + n) the host values tags[0 .. n), bn_index_fill_tags gives them all one tag (the
 * batch bn_index_add_ctx just appended: its first_id and batch_size), bn_index_read_tags copies the tags of rows [first, first + count)
 * to host.  The rows must lie in [0, bn_index_size) and every tag must be below the limit, otherwise BN_ERR_INVALID_ARG with a message
 * and no tag changed (the whole array is checked before any write).  The calls run on the index's stream, after a pending
 * bn_index_add_ctx, and are synchronous. */
#define BN_INDEX_TAG_LIMIT 65536u
bn_status bn_index_set_tags(bn_index *x, uint64_t first_id, size_t n, const uint32_t *tags);
bn_status bn_index_fill_tags(bn_index *x, uint64_t first_id, size_t n, uint32_t tag);
bn_status bn_index_read_tags(const bn_index *x, uint64_t first, size_t count, uint32_t *tags_out);

/*
 * Classifier heads: an immutable linear head z[c] = sum_k W[c][k] * x[k] + b[c] over a model's embedding, resident on one
 * device (label a few hundred search hits, fit a head on their embeddings, run it on everything that arrives from then on).
 * The reference exposes embeddings and has neither search nor heads; the contract is what a float64 evaluation of the
 * formulas below returns, up to the stated f32 bounds.
 *
 *   Logit          one f32 fmaf chain over k in a fixed order (fixed by dim alone), then the bias added.  Its bits depend only
 *                  on dim, the row, that class's weights and bias, and the flag: not on the batch size, the row's position,
 *                  how many other classes the head has, or the entry point (a step or bn_head_apply_host).  Against float64
 *                  |z - z64| <= 2 * (dim + 8) * 2^-24 * (sum_k |W[c][k] * xh[k]| + |b[c]|), xh the input (normalised in
 *                  float64 under BN_HEAD_L2NORM): the worst case of an f32 chain of that length plus an f32 norm.
 *   L2NORM         the index's rule: xh = x / sqrt(sum x^2); a row with zero norm, a non-finite element or an overflowing sum
 *                  of squares becomes zeros, so its logits equal the bias.
 *   Step           bn_ctx_attach_head makes every later bn_step_device / bn_step_windows / bn_step_live of the context also
 *                  run the head on that step's embedding rows, on the context's stream, after the plan and the step's own
 *                  top-K and outside the captured plan graph (capture_fallbacks stays 0), and rank the head logits with the
 *                  step's top-K kernel under the attached top_k / has_min / min_conf (top_k_predictions semantics, bit-identical
 *                  to bn_topk_host on the same logits).  Logits and packed rows reach pinned buffers as the step's own do;
 *                  bn_step_head_results is valid after bn_ctx_synchronize, until the next step.  The step's own outputs are
 *                  unchanged, bit for bit.  bn_infer*, tickets (bn_infer_submit / bn_infer_collect) and bn_group_* carry no
 *                  head results.
 *   Fit            with a_c = [W_c, b_c] and xt = [xh, 1], bn_head_fit minimises over all classes at once
 *                    L(A) = (1/n) sum_i sum_c [ -pw_c y_ic log s(a_c.xt_i) - (1 - y_ic) log(1 - s(a_c.xt_i)) ] + (l2/2) |A|^2
 *                  (s the logistic function; the bias is regularised with the same l2).  L is l2-strongly convex, so
 *                  L(A) - L* <= |grad L(A)|^2 / (2 l2): this right-hand side is the certificate.  The fit stops when its own
 *                  f32 certificate is <= tol or after max_iters evaluations of (L, grad L); after max_iters it still returns
 *                  the head, with converged = 0.  Deterministic: fixed reduction orders, no floating-point atomics; two fits
 *                  of the same inputs give the same bits.  A class with no positives, or no negatives, is legal.
 *   Refusals       BN_ERR_INVALID_ARG with a message, nothing changed: a model without embeddings, dim != embedding_dim, a
 *                  head on another device, a top_k the step's top-K refuses for n_classes (0, or beyond its on-chip heap),
 *                  labels other than 0/1, l2 / tol / pos_weight not positive and finite, n == 0, an id >= bn_index_size or one
 *                  whose stored row is all zeros, dim outside 1..8192, n_classes outside 1..4096, NULL where data is required.
 *                  Without a gfx950 device create, fit and apply return BN_ERR_NO_DEVICE.
 *   Lifetime       a context that attached a head keeps it alive: bn_head_free and bn_ctx_destroy may come in either order.
 *   Threading      a head is immutable and may be attached to any number of contexts; bn_head_apply_host / bn_head_read take
 *                  one thread at a time per head.
 */
typedef struct bn_head bn_head;
#define BN_HEAD_L2NORM 1u /* the head's input is x / sqrt(sum x^2), by the index's normalisation rule */
/* W [n_classes * dim] row-major, bias [n_classes] or NULL (= 0); flags: 0 or BN_HEAD_L2NORM */
bn_status bn_head_create(int32_t device, size_t dim, size_t n_classes, const float *W, const float *bias, uint32_t flags,
                         bn_head **out);
void bn_head_free(bn_head *h);
size_t bn_head_dim(const bn_head *h);
size_t bn_head_classes(const bn_head *h);
uint32_t bn_head_flags(const bn_head *h);
/* the head's parameters back on the host: W_out [n_classes * dim], bias_out [n_classes] (either may be NULL) */
bn_status bn_head_read(const bn_head *h, float *W_out, float *bias_out);
/* the head on n host rows [n * dim] -> logits_out [n * n_classes] */
bn_status bn_head_apply_host(const bn_head *h, const float *rows, size_t n, float *logits_out);

typedef struct bn_head_fit_opts { /* zero / NULL fields take the defaults in brackets */
    float l2;                /* lambda > 0 [1e-3] */
    float tol;               /* stop when the certificate <= tol [1e-6] */
    uint32_t max_iters;      /* [2000] */
    uint32_t flags;          /* BN_HEAD_L2NORM */
    const float *pos_weight; /* [n_classes] > 0, or NULL = 1 */
} bn_head_fit_opts;
typedef struct bn_head_fit_report {
    uint32_t iters;
    int32_t converged;
    double loss;
    double certificate;
} bn_head_fit_report;
/* fit on n host rows [n * dim] with labels [n * n_classes] (0 / 1); opts may be NULL (all defaults), report may be NULL.
 * Both structs are read / written through the caller's struct size, as bn_model_get_cost does. */
bn_status bn_head_fit(int32_t device, size_t dim, size_t n_classes, const float *rows, const uint8_t *labels, size_t n,
                      const bn_head_fit_opts *opts, size_t opts_size, bn_head **out, bn_head_fit_report *report,
                      size_t report_size);
/* training rows taken from an index by id, device to device, used as stored; the head gets BN_HEAD_L2NORM */
bn_status bn_head_fit_index(bn_index *x, const uint64_t *ids, const uint8_t *labels, size_t n, size_t n_classes,
                            const bn_head_fit_opts *opts, size_t opts_size, bn_head **out, bn_head_fit_report *report,
                            size_t report_size);
/*
 * Ranking an index by a head: per class, the top_m stored rows by the head's own logit, computed where the slab lives (re-score
 * the archive after a fit; choose the rows worth labelling next).  One pass over the slab serves up to 64 classes.
 *
 *   Logit          for class c and stored row r, z = chain(W_c, stored row r) + b_c, chain the head block's accumulation: one
 *                  accumulator, the k order fixed by the padded dim alone, then the bias added.  The row is used AS STORED
 *                  (normalised once at append, not again), which is what bn_head_fit_index trains on.  So the bits equal
 *                  bn_head_apply_host's for a head with the same W, b and flags 0 on the row as bn_index_read returns it; and,
 *                  the head's normalisation being the index's (the same bits), for a window appended by bn_index_add_ctx they
 *                  equal that step's bn_step_head_results logit of the same head.  A logit's bits depend on dim, the row, W_c
 *                  and b_c only: not on the row's position, the index size, the id range, the exclusions, top_m, the mode or
 *                  how many classes the head has.
 *   Eligible rows  inside the id range, not in exclude_ids, and valid: a row the index stored as zeros is never returned, as in
 *                  a search.  A row whose logit is NaN is never returned in either mode.
 *   Order          BN_RANK_TOP: z descending, ties by id ascending (-0.0 == +0.0, the index's rule).  BN_RANK_UNCERTAIN: |z|
 *                  ascending, ties by id ascending, so z and -z tie.  count = min(top_m, eligible rows); entries past count
 *                  are not written.  logit_out holds z itself in both modes; the caller applies the sigmoid.
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing changed: NULL where data is required, an
 *                  unknown mode, top_m outside 1..256, m_stride < top_m, first_id > bn_index_size or a range that runs past the
 *                  end, an excluded id >= bn_index_size, bn_head_dim != bn_index_dim, a head on another device, a head without
 *                  BN_HEAD_L2NORM (its weights expect raw embeddings, and the index no longer has them).
 *   Empty cases    an empty index or an empty range gives every count = 0.  Duplicates in exclude_ids are legal.
 *   No device      without a gfx950 device the call returns BN_ERR_NO_DEVICE.
 *   Determinism    no floating-point atomics; two calls give the same bytes.  The head and the index are unchanged.
 *   Threading      one thread at a time per index; the head is immutable and may be in use elsewhere.
 *
 * Outputs are host arrays: id_out and logit_out [n_classes * m_stride] (class c's list starts at c * m_stride), count_out
 * [n_classes].  The call is synchronous; like bn_index_search it first waits for a pending bn_index_add_ctx.
 */
#define BN_RANK_TOP 0u       /* logit descending */
#define BN_RANK_UNCERTAIN 1u /* |logit| ascending: nearest the decision boundary */
/* rows [first_id, first_id + n_ids), n_ids == 0: to the end; exclude_ids [n_exclude] (e.g. the rows already labelled), NULL / 0: none */
bn_status bn_head_rank_index(const bn_head *h, bn_index *x, uint32_t mode, uint64_t first_id, uint64_t n_ids,
                             const uint64_t *exclude_ids, size_t n_exclude, size_t top_m, size_t m_stride, uint64_t *id_out,
                             float *logit_out, uint32_t *count_out);
/* every later bn_step_device / bn_step_windows / bn_step_live on c also runs the head on that step's embedding rows;
 * h == NULL detaches (the other arguments are then ignored) */
bn_status bn_ctx_attach_head(bn_ctx *c, bn_head *h, size_t top_k, int32_t has_min, float min_conf);
/* pinned host views of the last step's head results: logits [batch, n_classes], idx / conf [batch, k_stride], count [batch] */
bn_status bn_step_head_results(const bn_ctx *c, const float **logits, const uint32_t **idx, const float **conf,
                               const uint32_t **count, size_t *k_stride, size_t *n_classes);

/*
 * Matching a step against an attached index (a watch list): a library of labelled example rows (an index with row tags) searched
 * for every embedding row of every step, where the step runs.  Heads answer "a class I have fitted"; this answers "the nearest
 * labelled examples of this window, now".  Nothing but finished results crosses the bus, and any number of contexts share one index.
 *
 *   Snapshot       the attachment searches rows [0, n), n = bn_index_size at the attach (a pending bn_index_add_ctx is waited for
 *                  first).  The slab is allocated once at bn_index_create and an append writes only rows >= the size, so appends
 *                  and every other index call, on other threads, are legal while attached steps run: the rows a step sees are
 *                  masked by id, never by what an append may be writing.  Attaching again takes a new snapshot; refreshing one
 *                  without re-attaching is not offered.  rows_searched reports n; n == 0 is legal and gives every count 0.
 *   Query          the step's embedding row, normalised by the index's rule (the same bits as an append or a search query).  A
 *                  row with zero norm, a non-finite element or an overflowing or underflowing sum of squares has count 0.
 *   Score, order   the f32 score of bn_index_search, bit for bit; its bits depend on dim, the query and the row only: not on the
 *                  batch size, the row's position in the batch, the number of rows searched or the entry point (a step or
 *                  bn_index_match).  Score descending, ties by id ascending (-0.0 == +0.0).  A row stored as zeros is never returned.
 *   Threshold      with has_min a row is a candidate iff its f32 score >= min_score, so the result is exactly the prefix of
 *                  bn_index_search's list of the same top_m whose scores are >= min_score.  min_score must then be finite.
 *   Tags           tag[j] is the tag of row id[j] as the tag plane holds it when the step executes (the plane is looked up at every
 *                  step, not at the attach); an index that never tagged gives zeros.  bn_index_set_tags / bn_index_fill_tags must
 *                  not run while an attached step is in flight: ordering the two is the caller's.
 *   Results        pinned host arrays owned by the attachment: id, score, tag [batch * m_stride] (m_stride >= top_m is reported;
 *                  query i's list starts at i * m_stride) and count [batch], valid after bn_ctx_synchronize until the context's
 *                  next step; entries past a count are unspecified.  Before any step since the attach bn_step_index_results is
 *                  BN_ERR_INVALID_ARG.
 *   Step           bn_ctx_attach_index makes every later bn_step_device / bn_step_windows / bn_step_live of the context also run
 *                  the match on that step's embedding rows, on the context's stream, after the plan and the step's own top-K
 *                  and outside the captured plan graph (capture_fallbacks stays 0): three launches and one copy per step, whatever
 *                  the batch.  The step's own outputs and the head's, prior's and tracker's results are unchanged, bit for bit.
 *                  bn_infer*, tickets (bn_infer_submit / bn_infer_collect) and bn_group_* carry no match results.
 *   Refusals       BN_ERR_INVALID_ARG with a message, nothing changed (an earlier attachment stays in place and working): a NULL
 *                  context, a model without a computed embedding output, bn_index_dim != embedding_dim, an index on another
 *                  device, top_m outside 1..256, m_stride < top_m, a non-finite min_score with has_min, NULL rows or outputs with
 *                  n > 0.  Without a gfx950 device bn_index_match returns BN_ERR_NO_DEVICE.
 *   Lifetime       the attachment holds a reference on the index: bn_index_free and bn_ctx_destroy may come in either order, the
 *                  slab lives until the last of them.
 *   Threading      an index may be attached to any number of contexts, each stepped by its own thread.  bn_ctx_attach_index and
 *                  bn_index_match take one thread at a time per index, like every other index call.
 */
/* every later bn_step_device / bn_step_windows / bn_step_live on c also matches that step's embedding rows against the rows x
 * holds now; x == NULL detaches (the other arguments are then ignored) */
bn_status bn_ctx_attach_index(bn_ctx *c, bn_index *x, size_t top_m, int32_t has_min, float min_score);
/* pinned host views of the last step's match results (any output may be NULL): id / score / tag [batch, m_stride], count [batch] */
bn_status bn_step_index_results(const bn_ctx *c, const uint64_t **id, const float **score, const uint32_t **tag,
                                const uint32_t **count, size_t *m_stride, size_t *rows_searched);
/* the same kernels on n host rows [n * dim], without a model: outputs [n * m_stride] and count_out [n].  Synchronous, on the index's
 * stream, over the index's current size (after a pending bn_index_add_ctx), any n (in rounds) */
bn_status bn_index_match(bn_index *x, const float *rows, size_t n, size_t top_m, int32_t has_min, float min_score,
                         size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *tag_out, uint32_t *count_out);

/*
 * Clustering an index: what is in the archive, before there is a window to search from or a label to fit on.  bn_index_assign
 * gives every stored row its nearest centroid; bn_index_cluster is spherical k-means (Lloyd) on top of it.  Both run where the
 * slab lives: one pass over it serves up to 64 centroids, and no row crosses the bus.  The reference has embeddings and nothing
 * built on them; this comment is the contract.
 *
 *   Score          for stored row r and centroid c, s = chain(centroid c, stored row r) + 0.0f, chain the head block's
 *                  accumulation: one accumulator, the k order fixed by the padded dim alone.  So the bits equal
 *                  bn_head_apply_host's for a head with W = centroids, no bias and flags 0 on the row as bn_index_read returns it.
 *                  Host centroids are used AS GIVEN (not normalised), as a head's W is.  A score's bits depend on dim, the row
 *                  and that centroid only: not on k, the centroid's position, the pass of 64 it falls in, the row's position,
 *                  the id range or the index size.
 *   Order          the centroid of largest score wins; ties go to the lowest centroid index (-0.0 == +0.0); a NaN score never
 *                  wins.  Centroids beyond 64 take further passes over the slab; a row's running (best score, best index) is
 *                  carried from pass to pass on the device, and a later pass replaces it only on a strictly larger score.
 *   Eligible rows  inside the id range and valid.  A row the index stored as zeros, or one all of whose scores are NaN, gets
 *                  BN_CLUSTER_NONE and score NaN, belongs to no cluster and counts toward no centroid.
 *   Start          (cluster) init_ids: the stored rows of k ids, as stored.  init_centroids: host vectors, as given.  Neither:
 *                  max-min.  The first centroid is the lowest-id valid row of the range; each further one is the valid row, not
 *                  yet chosen, whose best score against the centroids so far is smallest, ties by lowest id (one single-centroid
 *                  pass per centroid).  Rows that coincide with chosen ones tie at their own score, so when nothing else is left
 *                  the next unchosen row in id order is taken.  start_ids_out receives the chosen ids (or init_ids).
 *   Update         (cluster) per cluster, its member rows summed in ascending id order: segments of 256 consecutive members,
 *                  each summed member by member in float64, the segments added in order in float64; then the float64 norm, and
 *                  sum / norm stored as f32.  The association depends on a member's rank inside its cluster alone, never on the
 *                  device.  Against a float64 evaluation, per component, with n_c members and s the sum,
 *                  |c - c64| <= 2^-24 |c64| + n_c * 2^-52 * (sum_members |x|) / |s|.  A cluster with no members, or whose sum
 *                  has zero or non-finite norm, keeps its centroid; report.empty_clusters counts those of the last update.
 *   Stop           (cluster) assign, update, assign, ...: the call stops after an assignment pass that moved no row against the
 *                  pass before it (converged = 1), or after max_iters updates, and always right after an assignment pass.  So
 *                  assign_out / score_out are the exact assignment under centroids_out, counts_out its cluster sizes, and with
 *                  converged = 1 centroids_out is also the update of assign_out.  moved_last is the last pass's count (the first
 *                  pass of a call moves every row of the range).  objective is the float64 sum, in id order, of the last pass's
 *                  winning scores; objective_history receives the same sum for every pass (history_len of them, at most
 *                  history_capacity).
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing changed: NULL where data is required (the
 *                  index, centroids, assign_out, centroids_out, counts_out), k outside 1..1024, first_id > bn_index_size or a
 *                  range that runs past the end, a non-finite centroid or init centroid, an init id outside the range, one whose
 *                  stored row is all zeros, a duplicate init id, both init_ids and init_centroids, and (cluster) a range with
 *                  fewer valid rows than k.
 *   Empty cases    an empty index or an empty range is legal for bn_index_assign and writes nothing; for bn_index_cluster it
 *                  falls under the fewer-rows refusal.
 *   No device      without a gfx950 device both calls return BN_ERR_NO_DEVICE and leave the outputs untouched.
 *   Determinism    no floating-point atomics; two calls with the same inputs give the same bytes in every output.  t iterations
 *                  in one call give the same centroids_out, assign_out, score_out and counts_out as t calls of one iteration each,
 *                  every call started from the previous call's centroids_out through init_centroids.
 *   Memory         the centroids [k, dim padded], the running best and previous-assignment planes and the member lists (4 words
 *                  per row), and partial sums of at most 32 MB or one slot of k x padded dim doubles: allocated by the first
 *                  call that needs them, kept for the next, freed with the index.  An index that never clusters allocates none.
 *   Threading      one thread at a time per index.
 *
 * Outputs are host arrays: assign_out (u32) and score_out (f32, may be NULL) [rows of the range], entry i for row first_id + i;
 * centroids_out [k * dim]; counts_out [k].  Both calls are synchronous; like bn_index_search they first wait for a pending
 * bn_index_add_ctx.  The index is unchanged.
 */
#define BN_CLUSTER_NONE 4294967295u /* 0xFFFFFFFF: the assignment of a row that belongs to no cluster */
/* rows [first_id, first_id + n_ids), n_ids == 0: to the end; centroids host [k * dim] */
bn_status bn_index_assign(bn_index *x, const float *centroids, size_t k, uint64_t first_id, uint64_t n_ids,
                          uint32_t *assign_out, float *score_out);
typedef struct bn_cluster_opts { /* zero / NULL fields take the defaults in brackets */
    uint32_t max_iters;          /* updates at most [50] */
    const uint64_t *init_ids;    /* [k] stored rows as the first centroids, or NULL */
    const float *init_centroids; /* [k * dim] first centroids, or NULL; neither: the max-min start */
    uint64_t *start_ids_out;     /* [k]: receives the rows the start used (not written under init_centroids), or NULL */
    double *objective_history;   /* [history_capacity]: receives the objective of every assignment pass, or NULL */
    size_t history_capacity;
} bn_cluster_opts;
typedef struct bn_cluster_report {
    uint32_t iters;          /* updates made */
    int32_t converged;
    uint32_t empty_clusters; /* centroids the last update kept */
    uint32_t moved_last;
    double objective;
    uint32_t history_len;    /* entries written to objective_history */
} bn_cluster_report;
/* opts may be NULL (all defaults), report may be NULL; both structs are read / written through the caller's struct size */
bn_status bn_index_cluster(bn_index *x, size_t k, uint64_t first_id, uint64_t n_ids, const bn_cluster_opts *opts,
                           size_t opts_size, float *centroids_out, uint32_t *assign_out, float *score_out,
                           uint32_t *counts_out, bn_cluster_report *report, size_t report_size);

/*
 * Probed search: an inverted-file (IVF) view of an index.  The view holds k centroids, the exact assignment of the rows it covers
 * and one member list per centroid; a search scores the query against the centroids, takes the nprobe best lists and scans only
 * their rows.  The index's rule holds as a precise statement: A PROBED SEARCH RETURNS EXACTLY WHAT bn_index_search WOULD RETURN
 * IF ONLY THE ROWS OF THE PROBED LISTS EXISTED, with the same score bits, order and tie rule.  The one approximation is which
 * lists are probed, and that choice is exact, specified here and reported to the caller.  The reference has nothing of the kind;
 * this comment is the contract.
 *
 *   Build          k in 1..1024; host centroids [k * dim] are used AS GIVEN and must be finite, as for bn_index_assign.  The
 *                  assignment of rows [0, bn_index_size) is bn_index_assign's, to the byte: the same score chain, the same
 *                  lowest-index tie rule, BN_CLUSTER_NONE for an invalid row and for one all of whose scores are NaN.  List c
 *                  holds the ids of the rows assigned to c, ascending; a BN_CLUSTER_NONE row is in no list.  The view BORROWS
 *                  the index: free it before the index, and keep to one thread at a time per index, the view included.
 *   Memory         the view owns what it uses: the centroids [k, dim padded], the assignment planes and the member lists (3
 *                  words per row of the index's capacity), 2 words per (query of a round, centroid) of probe scratch, and 32 MB
 *                  of candidates.  A later bn_index_assign or bn_index_cluster on the index changes nothing the view returns.
 *   Extend         rows appended after the build are not searched until bn_ivf_extend: before it every call behaves as if the
 *                  index ended at bn_ivf_rows.  bn_ivf_extend assigns ids [bn_ivf_rows, bn_index_size) under the same centroids
 *                  and rebuilds the lists; after it, lists and search results are byte-identical to a fresh bn_ivf_build with
 *                  the same centroids.  The lists are rebuilt in place: a bn_ivf_extend that fails with BN_ERR_BACKEND leaves the
 *                  view fit for bn_ivf_free only.
 *   Probes         the score of a query against centroid c is the clustering score: the head block's chain + 0.0f, the bits of
 *                  bn_head_apply_host for a head with W = centroids, no bias and flags 0.  For bn_ivf_search the chain runs on
 *                  the query as the index normalises it (the row bn_index_read returns after bn_index_add_host of it); for
 *                  bn_ivf_search_ids on the stored row.  Lists are taken by score descending, ties to the lowest centroid index
 *                  (-0.0 == +0.0); a NaN score is never probed.  nprobe is in 1..k.  An empty list that ranks among the first
 *                  nprobe still uses its slot.  probes_out[q * nprobe ..] receives the probed lists in that order; slots past
 *                  the number probed, and every slot of an invalid query, hold BN_CLUSTER_NONE.  scanned_out[q] is the sum of
 *                  the probed lists' sizes.  So for bn_ivf_search_ids the first probe of query id i is row i's assigned list.
 *   Result         eligible rows are the members of the probed lists, less the exclusion radius for bn_ivf_search_ids.  Score,
 *                  order, count, the top_m / m_stride limits and the handling of an invalid query (count 0) are
 *                  bn_index_search's, word for word.  The bits of a (query, row) score are those bn_index_search gives that
 *                  pair: they depend on the padded dim alone, not on the list, the row's position in it, nprobe, the number of
 *                  queries of the call or how the lists are split among workgroups.  With nprobe == k and no BN_CLUSTER_NONE
 *                  row, id_out, score_out and count_out equal bn_index_search's (bn_index_search_ids') bytes.
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing changed: NULL where data is required (the
 *                  index, the view, centroids, out, queries / query_ids, id_out, score_out, count_out, sizes_out, n_out, and
 *                  ids_out for a list that is not empty), k outside 1..1024, nprobe outside 1..k, a non-finite centroid, top_m
 *                  outside 1..256, m_stride < top_m, a query id >= bn_ivf_rows, list >= k, and cap smaller than the list (n_out
 *                  still receives the size).
 *   Empty cases    an empty index builds a view with k empty lists; its searches return count 0.
 *   No device      without a gfx950 device every call that needs one (all but bn_ivf_free, bn_ivf_lists, bn_ivf_rows and
 *                  bn_ivf_list_sizes) returns BN_ERR_NO_DEVICE and leaves the outputs untouched; a NULL output pointer, k outside
 *                  1..1024, top_m outside 1..256 and m_stride < top_m are refused before the device is asked for.
 *   Determinism    no floating-point atomics; two calls with the same inputs give the same bytes; one call with Q queries gives
 *                  the same bytes as Q calls with one query each.
 *
 * Outputs are host arrays: id_out / score_out [n_queries * m_stride] and count_out [n_queries] as for bn_index_search;
 * probes_out (u32) [n_queries * nprobe] and scanned_out (u64) [n_queries] may be NULL.  All calls are synchronous; like
 * bn_index_search they first wait for a pending bn_index_add_ctx.  The index is unchanged.
 */
typedef struct bn_ivf bn_ivf;
bn_status bn_ivf_build(bn_index *x, const float *centroids, size_t k, bn_ivf **out);
void bn_ivf_free(bn_ivf *v);
size_t bn_ivf_lists(const bn_ivf *v); /* k */
size_t bn_ivf_rows(const bn_ivf *v);  /* the covered rows: ids [0, bn_ivf_rows) */
bn_status bn_ivf_extend(bn_ivf *v);
bn_status bn_ivf_list_sizes(const bn_ivf *v, uint32_t *sizes_out);
/* ids_out [cap] receives the list's ids ascending, *n_out their number */
bn_status bn_ivf_read_list(const bn_ivf *v, size_t list, uint64_t *ids_out, size_t cap, size_t *n_out);
bn_status bn_ivf_search(bn_ivf *v, const float *queries, size_t n_queries, size_t nprobe, size_t top_m, size_t m_stride,
                        uint64_t *id_out, float *score_out, uint32_t *count_out, uint32_t *probes_out, uint64_t *scanned_out);
bn_status bn_ivf_search_ids(bn_ivf *v, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t nprobe,
                            size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out,
                            uint32_t *probes_out, uint64_t *scanned_out);

/*
 * Coarse int8 search with exact re-rank: an 8-bit view of an index.  The view holds one code byte per slab element and one f32 scale
 * per row; a search ranks every covered row by an exact integer key, keeps the `refine` best as the query's candidates and re-scores
 * those with the index's own score.  The index's rule holds as a precise statement: A bn_sq8 SEARCH RETURNS EXACTLY WHAT
 * bn_index_search WOULD RETURN IF ONLY THE QUERY'S `refine` COARSE CANDIDATES EXISTED, with the same score bits, order and tie rule.
 * The one approximation is which rows become candidates, and that choice is exact, specified here and reported to the caller.  The
 * reference has nothing of the kind; this comment is the contract.
 *
 *   Code of a row  r = the stored f32 row (what bn_index_read returns), a = max_k |r[k]|.  An invalid row (stored as zeros) has all
 *                  codes 0 and scale +0.0f.  Otherwise inv = 127.0f / a (IEEE f32 division), code[k] = clamp(rint(r[k] * inv), -127,
 *                  127) with the product ONE f32 multiply rounded to nearest and rint to nearest, ties to even, and scale = a /
 *                  127.0f.  Pad columns hold code 0.  The bits are a function of the stored row alone: not of its id, the rows
 *                  around it, or whether build or extend wrote them.
 *   Query          the same rule, applied to the query as the index stages it: bn_sq8_search on the row as the index normalises it
 *                  (what bn_index_read returns after bn_index_add_host of it), bn_sq8_search_ids on the stored row, whose code is
 *                  therefore that row's code in the plane.
 *   Coarse key     of (query, row): D = sum_k qcode[k] * code[k] in int32 -- exact, since 127^2 * dim < 2^31 for dim <= 131072,
 *                  and free of summation order; key = (float)D * scale_row, a round-to-nearest int -> f32 conversion and one f32
 *                  multiply.  The query's scale is a positive constant per query and is left out.  A key is always finite; D == 0
 *                  gives +0.0f.
 *   Candidates     a row is eligible when it is valid, has an id < bn_sq8_rows and, for bn_sq8_search_ids, lies outside the
 *                  exclusion radius.  The candidates are the first `refine` eligible rows by key descending, ties by id ascending.
 *                  cand_out[q * refine ..] receives their ids in that order, cand_count_out[q] = min(refine, eligible rows);
 *                  entries past the count are not written.  An invalid query has cand_count 0 and count 0.
 *   Result         the candidates re-scored with bn_index_search's score: the bits are those bn_index_search gives that (query,
 *                  row) pair and depend on the padded dim alone, not on refine, the candidate's rank, the number of queries of the
 *                  call or the split among workgroups.  Order: score descending, ties by id ascending.  count = min(top_m,
 *                  cand_count); entries past count are not written.  With refine >= the number of eligible rows, id_out, score_out
 *                  and count_out equal bn_index_search's (bn_index_search_ids') bytes.
 *   Limits         1 <= top_m <= refine <= 256 and m_stride >= top_m.  256 is the widest list the selection keeps.
 *   Extend         rows appended after the build are not searched until bn_sq8_extend: before it every call behaves as if the
 *                  index ended at bn_sq8_rows.  bn_sq8_extend encodes ids [bn_sq8_rows, bn_index_size); after it codes, scales and
 *                  every search result are byte-identical to a fresh bn_sq8_build.
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing changed: NULL where data is required (the
 *                  index, the view, out, queries / query_ids, id_out, score_out, count_out), dim > 131072, refine outside 1..256,
 *                  top_m outside 1..refine, m_stride < top_m, a query id >= bn_sq8_rows, first + count > bn_sq8_rows.
 *   Empty cases    an empty index builds a view of no rows; its searches return count 0 and cand_count 0.
 *   No device      without a gfx950 device every call that needs one (all but bn_sq8_free and bn_sq8_rows) returns
 *                  BN_ERR_NO_DEVICE and leaves the outputs untouched; a NULL out / queries / query_ids / id_out / score_out /
 *                  count_out, refine outside 1..256, top_m outside 1..refine and m_stride < top_m are refused before the device is
 *                  asked for.
 *   Determinism    no floating-point atomics; two calls with the same inputs give the same bytes; one call with Q queries gives
 *                  the same bytes as Q calls with one query each.
 *   Threading      the index's rule, the view included: one thread at a time per index.  The view BORROWS the index: free it
 *                  before the index.  All work runs on the index's stream, after a pending bn_index_add_ctx.
 *   Memory         the view owns one byte per slab element (rows of the index's capacity rounded up to 64 x dim rounded up to
 *                  128), 4 bytes per such row of scales, the codes of a round of 1024 queries, and the candidate buffers: 2 KB per
 *                  (query of a pass of 64, scan workgroup) with two workgroups per compute unit -- 64 MB at 256 compute units --
 *                  plus 3 KB per query of a round.
 *   Persistence    none.  The plane is a deterministic function of the stored bits: bn_sq8_build after bn_index_load reproduces
 *                  it to the byte.
 *
 * Outputs are host arrays: id_out / score_out [n_queries * m_stride] and count_out [n_queries] as for bn_index_search; cand_out
 * (u64) [n_queries * refine] and cand_count_out (u32) [n_queries] may be NULL.  bn_sq8_read copies codes [count * dim] (no padding)
 * and scales [count] of rows [first, first + count); either output may be NULL.  All calls are synchronous.  The index is unchanged.
 */
typedef struct bn_sq8 bn_sq8;
bn_status bn_sq8_build(bn_index *x, bn_sq8 **out);
void bn_sq8_free(bn_sq8 *v);
size_t bn_sq8_rows(const bn_sq8 *v); /* the covered rows: ids [0, bn_sq8_rows) */
bn_status bn_sq8_extend(bn_sq8 *v);
bn_status bn_sq8_read(const bn_sq8 *v, uint64_t first, size_t count, int8_t *codes_out, float *scales_out);
bn_status bn_sq8_search(bn_sq8 *v, const float *queries, size_t n_queries, size_t refine, size_t top_m, size_t m_stride,
                        uint64_t *id_out, float *score_out, uint32_t *count_out, uint64_t *cand_out, uint32_t *cand_count_out);
bn_status bn_sq8_search_ids(bn_sq8 *v, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t refine,
                            size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out,
                            uint64_t *cand_out, uint32_t *cand_count_out);

/*
 * Filtered search: a bn_subset is a device-resident list of row ids of one index, strictly ascending, and a search over it reads only
 * those rows, once for all queries of a pass.  The index's rule holds as a precise statement: A bn_subset SEARCH RETURNS EXACTLY WHAT
 * bn_index_search / bn_index_search_ids WOULD RETURN IF ONLY THE SUBSET'S ROWS EXISTED, with the same score bits, order and tie rule.
 * The reference has nothing of the kind; this comment is the contract.
 *
 *   Members        bn_subset_select: a row is a member exactly when its id lies in [first_id, first_id + n_ids) (n_ids == 0: to the
 *                  end of the index, bn_index_assign's convention) and its tag passes the list: with tags == NULL or n_tags == 0
 *                  tags are not tested; otherwise the tag must be in the list (duplicates allowed), or, under
 *                  BN_FILTER_EXCLUDE_TAGS, must not be.  bn_subset_from_ids: the given ids, which must be strictly ascending and
 *                  below bn_index_size.  Validity is NOT tested: a row stored as zeros may be a member; like everywhere else it is
 *                  never returned.  bn_subset_size is the number of members, bn_subset_read copies members [first, first + count)
 *                  of the ascending list.
 *   Fixed          the list is made once.  Rows appended later and tags changed later do not alter it; its searches before and
 *                  after such calls return the same bytes.
 *   Result         the score of a (query, member) pair has the bits bn_index_search gives that pair: the same k-ordered chain over
 *                  the padded dim, whatever the subset, the member's position in it, the number of queries of the call or the split
 *                  among workgroups.  Order: score descending, ties by id ascending (-0.0 == +0.0).  count = min(top_m, valid
 *                  members not excluded); entries past count are not written.  The subset of all rows returns bn_index_search's
 *                  (bn_index_search_ids') bytes.
 *   Query          bn_index_search's rules: a host query is normalised as an appended row is, and one with zero norm or a non-finite
 *                  element returns count 0.  bn_subset_search_ids takes stored rows as queries: query_ids name ANY stored row of the
 *                  index, in or out of the subset (the index's current size bounds them), and members whose id lies within
 *                  exclude_radius of the query's own id are skipped (< 0: none; 0: the row itself).
 *   Limits         1 <= top_m <= 256 and m_stride >= top_m.
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing created: NULL where data is required (the index,
 *                  the filter, ids, out, the subset, queries / query_ids, id_out, score_out, count_out), a struct_size smaller than
 *                  bn_index_filter, an id range that does not lie in [0, bn_index_size], a listed tag >= BN_INDEX_TAG_LIMIT, flags
 *                  other than BN_FILTER_EXCLUDE_TAGS, ids that are not strictly ascending or reach bn_index_size, top_m outside
 *                  1..256, m_stride < top_m, a query id >= bn_index_size, first + count > bn_subset_size.
 *   Empty cases    an empty subset is legal (an empty range, a tag nobody has, n == 0); its searches return count 0 without a launch.
 *   No device      without a gfx950 device every call that needs one (all but bn_subset_free and bn_subset_size) returns
 *                  BN_ERR_NO_DEVICE and leaves the outputs untouched; the refusals that need neither the index nor the subset (a NULL
 *                  filter / out / queries / query_ids / id_out / score_out / count_out, struct_size, flags, a listed tag, ids out of
 *                  order, top_m, m_stride) come before the device is asked for.
 *   Determinism    no atomic decides a position and no floating-point atomics: two selections of the same state give the same
 *                  bytes; two searches with the same inputs give the same bytes; one call with Q queries gives the same bytes as Q
 *                  calls with one query each.
 *   Threading      the index's rule, its views included: one thread at a time per index.  The subset BORROWS the index: free it
 *                  before the index.  All work runs on the index's stream, after a pending bn_index_add_ctx; every call is
 *                  synchronous.
 *   Memory         four bytes per member.  A search uses the index's own query and candidate buffers.
 *   Persistence    none: bn_subset_read / bn_subset_from_ids carry a list across processes.
 *
 * struct_size is sizeof(bn_index_filter) as the caller compiled it.  Outputs are host arrays: id_out / score_out
 * [n_queries * m_stride] and count_out [n_queries] as for bn_index_search.  The index is unchanged by every call.
 */
typedef struct bn_subset bn_subset;
typedef struct bn_index_filter {
    uint64_t first_id;    /* the id range [first_id, first_id + n_ids) */
    uint64_t n_ids;       /* 0: to the end of the index */
    const uint32_t *tags; /* host list of tag values, duplicates allowed; NULL or n_tags == 0: tags are not tested */
    size_t n_tags;
    uint32_t flags; /* 0, or BN_FILTER_EXCLUDE_TAGS: the list names the tags left OUT */
} bn_index_filter;
#define BN_FILTER_EXCLUDE_TAGS 1u
bn_status bn_subset_select(bn_index *x, const bn_index_filter *f, size_t struct_size, bn_subset **out);
bn_status bn_subset_from_ids(bn_index *x, const uint64_t *ids, size_t n, bn_subset **out);
void bn_subset_free(bn_subset *s);
size_t bn_subset_size(const bn_subset *s);
bn_status bn_subset_read(const bn_subset *s, size_t first, size_t count, uint64_t *ids_out);
bn_status bn_subset_search(bn_subset *s, const float *queries, size_t n_queries, size_t top_m, size_t m_stride, uint64_t *id_out,
                           float *score_out, uint32_t *count_out);
bn_status bn_subset_search_ids(bn_subset *s, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t top_m,
                               size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out);

/*
 * Copying rows between indexes: rows of one index are appended to ANOTHER index, device to device, WITH THE BITS THEY ARE STORED WITH,
 * their validity and their tags.  An index has a fixed capacity, rows never leave it and two indexes never become one; a copy is what
 * acts on a choice of rows (an id range, or a bn_subset made by bn_subset_select / bn_subset_from_ids): growing is a bigger index and
 * the whole range, retention the last N rows into a fresh index, dropping tombstoned rows the subset that excludes the tombstone tag,
 * merging several appends into one index.  Reading rows back and appending them again normalises a second time and changes bits;
 * this does not.  The reference has nothing of the kind; this comment is the contract.
 *
 *   Result         the appended rows get ids *first_new_id + j, *first_new_id being dst's size before the call (first_new_id may be
 *                  NULL) and j the position in the range or in the subset: the old id of new row j is first_id + j, or the j-th entry
 *                  bn_subset_read gives.  No further map is returned.
 *   Bits           bn_index_read(dst) of a new row returns the bytes bn_index_read(src) returns for its source row: nothing is
 *                  normalised again, and the pad columns and the valid byte are copied too.  A source row stored as zeros arrives as
 *                  zeros, counts toward bn_index_size(dst) and is never returned.  EVERYTHING THAT READS dst AFTERWARDS BEHAVES AS IF
 *                  dst HAD BEEN BUILT BY APPENDS THAT PRODUCED EXACTLY THESE STORED BITS: every search, bn_index_assign /
 *                  bn_index_cluster, bn_head_fit_index / bn_head_rank_index, bn_index_save, a match and attachments.
 *   Tags           if src has a tag plane the new rows carry their source rows' tags, and dst's plane is allocated if absent.  If
 *                  src has none the new rows' tags are 0; when dst has a plane those zeros are written, not assumed.  dst's older
 *                  rows and their tags are untouched.
 *   Views          the call is an append like any other: bn_ivf_extend and bn_sq8_extend pick the new rows up, subsets of dst stay
 *                  fixed, and an attachment's snapshot behaves as it does after bn_index_add_host.  src and its views are unchanged.
 *   Refusals       BN_ERR_INVALID_ARG with a message; nothing is appended, *first_new_id is untouched and both sizes are unchanged.
 *                  A NULL dst, src or s (before the device is asked for); then dst == src, or a subset that borrows dst; different
 *                  dim; different devices (rows are not copied between devices); a range that does not lie in
 *                  [0, bn_index_size(src)]; an append past dst's capacity, refused whole as bn_index_add_host refuses it.
 *   Empty cases    an empty range (first_id == bn_index_size(src)) or an empty subset is BN_OK: nothing is launched and
 *                  *first_new_id is dst's size.
 *   No device      without a gfx950 device both calls return BN_ERR_NO_DEVICE and leave *first_new_id untouched.
 *   Ordering       the work runs on dst's stream after a pending bn_index_add_ctx of EITHER index; the call is synchronous, like
 *                  bn_index_add_host.
 *   Determinism    plain loads and stores, no atomics: the same state gives the same bytes.
 *   Threading      the index's rule, for both indexes: one thread at a time per index, and neither may be in another call meanwhile.
 *   Memory         none beyond dst's own slab, and its tag plane where the copy creates it.  Out of place by design: there is no
 *                  compaction or truncation of an index in place (views, subsets and attachments hold ids and sizes of the index they
 *                  borrow), so src and dst exist side by side for as long as the caller keeps both.
 *   Not carried    IVF lists and int8 codes (rebuilt, or extended, from the copied rows), and tags in the index file.
 */
/* rows [first_id, first_id + n_ids) of src (n_ids == 0: to the end of src, bn_index_assign's convention) */
bn_status bn_index_append_rows(bn_index *dst, bn_index *src, uint64_t first_id, uint64_t n_ids, uint64_t *first_new_id);
/* the members of s, in the subset's (ascending) order, from the index s borrows */
bn_status bn_index_append_subset(bn_index *dst, const bn_subset *s, uint64_t *first_new_id);

/*
 * Event-level search: rows are appended in window order, so a row id is a position in time, and overlapping windows make neighbouring
 * rows near-duplicates: one call in the archive that matches a query fills several consecutive ranks of bn_index_search, once per window
 * that overlaps it.  exclude_radius handles this around the query's own id; bn_index_search_peaks handles it AMONG THE HITS: IT RETURNS
 * ONLY THE LOCAL PEAKS OF THE SCORE OVER ROW IDS, the first top_m of them in bn_index_search's order, with bn_index_search's score bits.
 * The rule is exact, free of any processing order and deterministic.  The reference has nothing of the kind; this comment is the contract.
 *
 *   Eligible row   exactly the rows bn_index_search (bn_index_search_ids) may return for that query: valid, id < bn_index_size and, for
 *                  the _ids form, outside exclude_radius of the query's own id (< 0: none excluded; 0: the row itself).
 *   Score          the bits bn_index_search gives that (query, row) pair: the same k-ordered chain over the padded dim.  They do not
 *                  depend on peak_radius, on the tile, on the split among workgroups or on the number of queries.
 *   Peak           an eligible row i is a peak of query q when EVERY OTHER eligible row j with 0 < |i - j| <= peak_radius comes AFTER i
 *                  in the index's total order: score descending, ties by id ascending (-0.0 == +0.0).  Ineligible rows take no part:
 *                  they are never peaks and they never suppress a neighbour.  Rows past the end of the index do not exist.
 *   Result         the first top_m peaks in that same order; count = min(top_m, number of peaks); entries past count are not written.
 *   Consequences   two returned ids of one query differ by more than peak_radius.  peak_radius == 0 makes every eligible row a peak:
 *                  the call returns bn_index_search's (bn_index_search_ids') bytes.  A run of exact ties has one peak, its lowest id.
 *   Not greedy     this is deliberately NOT greedy non-maximum suppression (take the best row, delete its neighbourhood, repeat).  On a
 *                  monotone ramp of scores -- row i scores higher than row i - 1 over a long stretch -- the greedy rule returns the top
 *                  row and then one row every peak_radius + 1 ids down the slope, none of which is a moment of its own; here the ramp
 *                  has ONE peak, its top, because every other row has a better neighbour.  A row suppressed by a neighbour still
 *                  suppresses its own neighbours: whether a row is a peak depends on the scores within peak_radius of it and on nothing
 *                  else, which is what makes the rule independent of any order of processing.
 *   Caveat         adjacency is BY ID ONLY.  Where two recordings meet in the append order, up to peak_radius rows of one can be
 *                  suppressed by a better row of the other.  Tags are not consulted: nothing but bn_subset_select reads a tag.
 *   Query          bn_index_search's rules: a host query is normalised as an appended row is, and one with zero norm or a non-finite
 *                  element returns count 0; bn_index_search_peaks_ids takes stored rows as queries, used as stored, and the id of an
 *                  invalid row returns count 0.
 *   Limits         0 <= peak_radius <= BN_PEAK_RADIUS_MAX, 1 <= top_m <= 256, m_stride >= top_m.
 *   Refusals       BN_ERR_INVALID_ARG with a message and no output written: top_m outside 1..256, m_stride < top_m, peak_radius above
 *                  BN_PEAK_RADIUS_MAX, NULL queries / query_ids / id_out / score_out / count_out with n_queries > 0, a NULL index, a
 *                  query id >= bn_index_size.
 *   No device      without a gfx950 device both calls return BN_ERR_NO_DEVICE and leave the outputs untouched; the refusals that need
 *                  no index (top_m, m_stride, peak_radius, the NULLs other than the index) come before the device is asked for.
 *   Empty index    count 0 for every query.
 *   Determinism    no atomic decides anything; two calls with the same inputs give the same bytes, and one call with Q queries gives
 *                  the same bytes as Q calls with one query each.
 *   Threading      the index's rule: one thread at a time per index.  The work runs on the index's stream, after a pending
 *                  bn_index_add_ctx, in the index's own query and candidate buffers; both calls are synchronous.  The index is unchanged.
 *
 * Outputs are host arrays: id_out / score_out [n_queries * m_stride] and count_out [n_queries] as for bn_index_search.
 */
#define BN_PEAK_RADIUS_MAX 64
bn_status bn_index_search_peaks(bn_index *x, const float *queries, size_t n_queries, size_t peak_radius, size_t top_m, size_t m_stride,
                                uint64_t *id_out, float *score_out, uint32_t *count_out);
bn_status bn_index_search_peaks_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius, size_t peak_radius,
                                    size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out);

/*
 * Sequence search: a call, a song bout or a chorus lasts longer than one window, and what a user marks in a recording is a RUN of
 * seq_len consecutive windows.  Row ids are positions in time (see above), so the query "where in the archive does this run occur,
 * aligned window by window" is the mean of the seq_len window scores along the diagonal, score(i) = mean_j dot(query_j, row[i + j]),
 * for every start row i.  A returned id is the START row of a match.  Joining the top-M lists of the windows on the host is not exact
 * (a run whose windows are each rank 300 never shows up); this is.  The reference has nothing of the kind; this comment is the contract.
 *
 *   Window score   s_j(r) has exactly the bits bn_index_search (bn_index_search_ids) gives the pair (query row j, index row r): the
 *                  same k-ordered chain over the padded dim.  It does not depend on the tile, on the split among workgroups, on seq_len
 *                  or on the number of sequences in the call.
 *   Eligible start start i is eligible when i + seq_len <= bn_index_size, EVERY row i .. i + seq_len - 1 is valid and, for the _ids
 *                  form, |i - first_id| > exclude_radius (< 0: none excluded; 0: only the query's own start).
 *   Sequence score acc_0 = s_0(i); acc_j = fl32(acc_{j-1} + s_j(i + j)) for j = 1 .. seq_len - 1, in that order;
 *                  score = fl32(acc_{seq_len-1} * inv) with inv = fl32(1.0f / (float)seq_len), computed once on the host.  No step is
 *                  fused with another.  For seq_len == 1 the score is s_0(i) bit for bit.
 *   Order          score descending, ties by id ascending (-0.0 == +0.0).
 *   Peak           with peak_radius R in 1..BN_PEAK_RADIUS_MAX only peaks are returned: an eligible start i is a peak when EVERY OTHER
 *                  eligible start j with 0 < |i - j| <= R comes AFTER i in that order: bn_index_search_peaks' rule over the sequence
 *                  scores, NOT greedy suppression.  Ineligible starts are never peaks and never suppress a neighbour.  R == 0: every
 *                  eligible start counts.
 *   Result         the first top_m such starts in that order; count = min(top_m, their number); entries past count are not written.
 *   Query          host form: each of the seq_len rows is normalised as an appended row is; a sequence with any zero-norm or
 *                  non-finite row returns count 0.  _ids form: the query is the stored rows [first_id, first_id + seq_len), used as
 *                  stored; an invalid row among them returns count 0.
 *   Consequences   seq_len == 1 returns bn_index_search_peaks' bytes (the _ids form bn_index_search_peaks_ids'), and with R == 0
 *                  bn_index_search's.  An index shorter than seq_len returns count 0.  One call with n sequences returns the bytes of n
 *                  calls with one sequence each.  With R >= 1 two returned ids of one sequence differ by more than R.
 *   Caveat         adjacency is BY ID ONLY, as for peaks: a match may span the point where two recordings meet in the append order.
 *                  Tags are not read.
 *   Limits         1 <= seq_len <= BN_SEQ_LEN_MAX, 0 <= peak_radius <= BN_PEAK_RADIUS_MAX, 1 <= top_m <= 256, m_stride >= top_m.
 *   Refusals       BN_ERR_INVALID_ARG with a message and no output written: top_m outside 1..256, m_stride < top_m, seq_len outside
 *                  1..BN_SEQ_LEN_MAX, peak_radius above BN_PEAK_RADIUS_MAX, NULL queries / first_ids / id_out / score_out / count_out
 *                  with n_seq > 0, a NULL index, a first_id + seq_len above bn_index_size.
 *   No device      without a gfx950 device both calls return BN_ERR_NO_DEVICE and leave the outputs untouched; the refusals that need
 *                  no index (top_m, m_stride, seq_len, peak_radius, the NULLs other than the index) come before the device is asked for.
 *   Determinism    no atomic decides anything; two calls with the same inputs give the same bytes.
 *   Threading      the index's rule: one thread at a time per index.  The work runs on the index's stream, after a pending
 *                  bn_index_add_ctx, in the index's own query and candidate buffers; both calls are synchronous.  The index is unchanged.
 *   Cost           one scan of the slab per pass; a pass holds min(64 / seq_len, 28) sequences (64 query rows, and LDS for 28 lines of
 *                  sequence scores): n_seq sequences take ceil(n_seq / that) passes.  seq_len 1 and 2 therefore take more passes than
 *                  bn_index_search takes for as many query rows (64 x seq_len 1: three against one), and seq_len 33 to 63 leave query
 *                  rows of the pass idle.  Measured times are in DESIGN.md.
 *
 * queries is a host array [n_seq * seq_len * dim], sequence after sequence, window after window.  Outputs are host arrays: id_out /
 * score_out [n_seq * m_stride] and count_out [n_seq].
 */
#define BN_SEQ_LEN_MAX 64
bn_status bn_index_search_seq(bn_index *x, const float *queries, size_t n_seq, size_t seq_len, size_t peak_radius, size_t top_m, size_t m_stride,
                              uint64_t *id_out, float *score_out, uint32_t *count_out);
bn_status bn_index_search_seq_ids(bn_index *x, const uint64_t *first_ids, size_t n_seq, size_t seq_len, int64_t exclude_radius, size_t peak_radius,
                                  size_t top_m, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out);

/*
 * Threshold search: EVERY row of an id range that scores at least min_score against a query, in id (= time) order, and how many there
 * are.  The searches above answer "the M best rows" and stop at 256; a call rate or an occupancy count ("every window that sounds like
 * this exemplar at cosine >= 0.8", or simply how many) is this call.  The reference has nothing of the kind; this comment is the contract.
 *
 *   Hit            row r is a hit of query i iff r lies in the id range, r is valid (not stored as zeros), for the _ids form r is
 *                  outside exclude_radius of the query's own id by bn_index_search_ids' rule (< 0: none excluded; 0: the row itself),
 *                  and score(i, r) >= min_score[i] as an IEEE f32 comparison.  min_score holds one value per query, [n_queries]:
 *                  -inf is legal and makes every eligible row a hit, +inf is legal and gives no hit, NaN is refused.
 *   Score          the f32 score of bn_index_search, bit for bit: the same k-ordered chain over the padded dim.  The bits depend on
 *                  dim, the query and the row only: not on the id range, max_hits, the number of queries or the index size.
 *   Query          bn_index_search's rules: a host query is normalised as an appended row is, and one with zero norm or a non-finite
 *                  element has count 0; the _ids form takes stored rows as queries, used as stored, and the id of an invalid row
 *                  has count 0.
 *   Order          hits come out in id ascending order: the one order a list of unknown length has without a sort, and time order.
 *   Counts         count_out[i] is the TOTAL number of hits of query i in the range, also when it exceeds max_hits.
 *   Truncation     entries [0, min(count, max_hits)) of query i's list are written, at i * h_stride: the FIRST hits in id order.
 *                  Entries past that are not written.  A caller that sees count > max_hits continues with
 *                  first_id = the last returned id + 1 (and n_ids shortened to the same end); the pages put together are the
 *                  unpaged list, byte for byte.
 *   Count only     max_hits == 0 writes the counts alone; id_out, score_out and tag_out may then be NULL, and the call touches no
 *                  staging memory.
 *   Tags           tag_out may be NULL.  Otherwise tag_out[j] is the tag of row id_out[j] as the tag plane holds it at the call,
 *                  or 0 for an index that never tagged (as bn_index_match reports them).  Tags do not decide what is a hit.
 *   Id range       bn_head_rank_index's convention: rows [first_id, first_id + n_ids), n_ids == 0: to the end.
 *   Limits         0 <= max_hits <= BN_ABOVE_MAX_HITS, h_stride >= max_hits.
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing changed: max_hits above BN_ABOVE_MAX_HITS,
 *                  h_stride < max_hits, NULL queries / query_ids, min_score or count_out with n_queries > 0, NULL id_out or score_out
 *                  with max_hits > 0 and n_queries > 0, a NaN in min_score (the whole array is checked before any work), a NULL
 *                  index, first_id > bn_index_size or a range that runs past the end, a query id >= bn_index_size.
 *   Empty cases    an empty index, an empty range or n_queries == 0 gives BN_OK with every count 0.
 *   No device      without a gfx950 device both calls return BN_ERR_NO_DEVICE and leave the outputs untouched; the refusals that need
 *                  no index (max_hits, h_stride, the NULLs other than the index, NaN) come before the device is asked for.
 *   Memory         staging lists and device results are allocated by the first call that needs them and stay with the index.  A
 *                  pass over the slab serves up to 64 queries; that number shrinks (48, 32, 16, 8, 4, 2, 1) until
 *                  queries x (workgroups x min(rows of a workgroup, max_hits) x 8 B + max_hits x 12 B) fits 64 MiB.  One query per
 *                  pass is the floor: at most 8 B x min(rows in the range, workgroups x max_hits) + 12 B x max_hits, under 2 % of
 *                  the slab.  A large max_hits on a large range therefore costs passes, not memory.
 *   Determinism    no atomics of any kind; two calls with the same inputs give the same bytes.
 *   Threading      the index's rule: one thread at a time per index.  The work runs on the index's stream, after a pending
 *                  bn_index_add_ctx; both calls are synchronous.  The index, its tags and every other search's results are unchanged.
 *
 * Outputs are host arrays: id_out / score_out / tag_out [n_queries * h_stride] and count_out [n_queries].
 */
#define BN_ABOVE_MAX_HITS 65536u
bn_status bn_index_search_above(bn_index *x, const float *queries, size_t n_queries, const float *min_score, uint64_t first_id,
                                uint64_t n_ids, size_t max_hits, size_t h_stride, uint64_t *id_out, float *score_out,
                                uint32_t *tag_out, uint32_t *count_out);
bn_status bn_index_search_above_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius,
                                    const float *min_score, uint64_t first_id, uint64_t n_ids, size_t max_hits, size_t h_stride,
                                    uint64_t *id_out, float *score_out, uint32_t *tag_out, uint32_t *count_out);

/*
 * Grouped threshold search: the hits of bn_index_search_above grouped by row tag -- per (query, tag) how many there are, the best one,
 * the first and the last in id (= time) order -- without returning a single hit.  "At which sites and on which days does this call
 * occur, how often, from when to when, and which is the best example at each" is one pass over the slab, whatever the number of
 * hits: what crosses the bus is one record per (query, group).  The reference has nothing of the kind; this comment is the contract.
 *
 *   Hit            bn_index_search_above's rule: row r is a hit of query i iff r lies in the id range, r is valid (not stored as
 *                  zeros), for the _ids form r is outside exclude_radius of the query's own id by bn_index_search_ids' rule (< 0: none
 *                  excluded; 0: the row itself), and score(i, r) >= min_score[i] as an IEEE f32 comparison.  min_score holds one value
 *                  per query, [n_queries]: -inf is legal and makes every eligible row a hit, +inf is legal and gives no hit, NaN is
 *                  refused.
 *   Score          the f32 score of bn_index_search, bit for bit.
 *   Query          bn_index_search's rules: a host query is normalised as an appended row is, and one with zero norm or a non-finite
 *                  element has no hits; the _ids form takes stored rows as queries, used as stored, and the id of an invalid row has
 *                  no hits.
 *   Group          the group of a hit is the row's tag as the tag plane holds it at the call; every row of an index that never tagged
 *                  has tag 0.  A hit whose tag is >= n_groups belongs to no group and is counted in other_out[i] only.
 *   Record         of (query i, group g), at i * g_stride + g of each array:
 *                    count_out                     the number of hits of the group (u32);
 *                    best_id_out / best_score_out  the hit with the highest score, ties broken by the lowest id: the index's order,
 *                                                  with -0.0 == +0.0;
 *                    first_id_out / last_id_out    the smallest and the largest id among the hits.
 *                  A group with count 0 gets BN_GROUP_NO_ROW in the three id arrays and 0.0f in best_score_out, so every byte of
 *                  entries [0, n_groups) of a query's rows is determined.  Entries [n_groups, g_stride) are not written.
 *   Totals         total_out[i] is the sum over the groups of count plus other_out[i]; it equals bn_index_search_above's count_out[i]
 *                  for the same arguments.
 *   Optional       each of best_id_out + best_score_out (a pair: both or neither), first_id_out, last_id_out, other_out and
 *                  total_out may be NULL and is then not computed for the caller.  count_out is required when n_queries > 0.
 *   Id range       bn_head_rank_index's convention: rows [first_id, first_id + n_ids), n_ids == 0: to the end.
 *   Limits         1 <= n_groups <= BN_INDEX_TAG_LIMIT, g_stride >= n_groups.
 *   Refusals       BN_ERR_INVALID_ARG with a message, no output written and nothing changed: n_groups outside 1..BN_INDEX_TAG_LIMIT,
 *                  g_stride < n_groups, only one of best_id_out / best_score_out, NULL queries / query_ids, min_score or count_out
 *                  with n_queries > 0, a NaN in min_score (the whole array is checked before any work), a NULL index,
 *                  first_id > bn_index_size or a range that runs past the end, a query id >= bn_index_size.
 *   Empty cases    an empty index, an empty range or n_queries == 0 gives BN_OK; every count, other and total is 0 and every record
 *                  written is the empty record.
 *   No device      without a gfx950 device both calls return BN_ERR_NO_DEVICE and leave the outputs untouched; the refusals that need
 *                  no index (n_groups, g_stride, the pair, the NULLs other than the index, NaN) come before the device is asked for.
 *   Memory         a device table of queries x n_groups records of 20 B, the finished records (as much again) and their pinned
 *                  mirror are allocated by the first call that needs them, grown by a later call that needs more, and stay with the
 *                  index.  A pass over the slab serves up to 64 queries; that number shrinks (48, 32, ...) until the table fits
 *                  64 MiB: 48 queries per pass at n_groups = 65536, 64 up to n_groups = 52428.
 *   Determinism    two calls with the same inputs give the same bytes.  The table is updated with integer atomics whose results do
 *                  not depend on their order (add on counts, max on a packed score-and-id key, min and max on ids); no
 *                  floating-point atomics.
 *   Threading      the index's rule: one thread at a time per index.  The work runs on the index's stream, after a pending
 *                  bn_index_add_ctx; both calls are synchronous.  The index, its tags and every other search's results are unchanged.
 *
 * Outputs are host arrays: count_out / best_id_out / best_score_out / first_id_out / last_id_out [n_queries * g_stride] and
 * other_out / total_out [n_queries].
 */
#define BN_GROUP_NO_ROW UINT64_MAX
bn_status bn_index_group_above(bn_index *x, const float *queries, size_t n_queries, const float *min_score, uint64_t first_id,
                               uint64_t n_ids, size_t n_groups, size_t g_stride, uint32_t *count_out, uint64_t *best_id_out,
                               float *best_score_out, uint64_t *first_id_out, uint64_t *last_id_out, uint32_t *other_out,
                               uint32_t *total_out);
bn_status bn_index_group_above_ids(bn_index *x, const uint64_t *query_ids, size_t n_queries, int64_t exclude_radius,
                                   const float *min_score, uint64_t first_id, uint64_t n_ids, size_t n_groups, size_t g_stride,
                                   uint32_t *count_out, uint64_t *best_id_out, float *best_score_out, uint64_t *first_id_out,
                                   uint64_t *last_id_out, uint32_t *other_out, uint32_t *total_out);

/*
 * Persistence of an index: bn_index_save writes the slab's STORED BITS to a file, bn_index_load makes an index from one.  A loaded
 * index behaves in every call exactly as the saved one did at the time of the save: searches, head fits and ranks, assignment,
 * clustering and IVF views are all stated in the bits of the stored rows, and those are what the file holds.  bn_index_read
 * followed by bn_index_add_host is NOT that: the append normalises again, x / sqrt(sum x^2) of a unit row is not the row in f32,
 * and a fifth to a quarter of the rows come back with other bits (measured at dim 3, 130 and 1536).  Heads (bn_head_read /
 * bn_head_create) and IVF views (bn_ivf_build from the caller's centroids) round-trip through their own entry points; only the
 * index needs a file.
 *
 *   File           version 1, little-endian, fully determined by the index contents and chunk_rows:
 *                    bytes 0..8    magic "BNINDEX1"
 *                          8..12   u32 version = 1
 *                          12..16  u32 dim
 *                          16..24  u64 rows (bn_index_size at the time of the save)
 *                          24..28  u32 chunk_rows (>= 1)
 *                          28..32  u32 n_chunks = ceil(rows / chunk_rows), 0 when rows = 0
 *                          32..40  u64 valid_rows
 *                          40..56  zero
 *                          56..64  u64 header digest
 *                          64..    n_chunks x u64 chunk digests, then rows x dim f32 in id order, row stride dim (no padding)
 *                  The size is exactly 64 + 8 * n_chunks + 4 * rows * dim.  No validity flags are stored: a row is invalid exactly
 *                  when every element is +0.0 or -0.0 ((bits & 0x7fffffff) == 0) -- the index stores the rows it never returns as
 *                  zeros, and a unit row has a non-zero element.
 *   Digest         for the element of row r, component k, with f32 bits b: u = r * dim + k; z = u * 0x9E3779B97F4A7C15 + b;
 *                  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31 (mod 2^64).  A
 *                  chunk's digest is the sum mod 2^64 of z over the elements of its rows [c * chunk_rows, (c + 1) * chunk_rows);
 *                  the header digest is the same sum over the fourteen u32 words of bytes 0..56 (u = the word's number, b = the
 *                  word).  A sum of integers: any order of addition gives the same digest, on the device and on the host.
 *   Save           chunk_rows == 0 takes max(1, 2^21 / dim); a chunk_rows above 2^32 - 1 is refused.  The call waits for a pending
 *                  bn_index_add_ctx as a search does, and leaves the index unchanged.  It writes to a temporary name in the
 *                  directory of `path` ("<path>.tmp.<pid>.<n>", n counted per process: saves from two threads do not collide, and
 *                  a temporary a crashed process left behind is stepped over, never opened) and renames it onto `path` only after
 *                  everything is written and the file flushed (fsync).  The directory is flushed after the rename where the file
 *                  system allows it; a failure of that last flush is not reported, so after a power loss the name may still be
 *                  the old file's, never a partial one.  On any failure the temporary is removed and a file that existed at `path`
 *                  is untouched.  Two saves of the same index with the same chunk_rows give identical bytes.
 *   Load           capacity_rows == 0: the file's row count (1 for an empty file).  The new index has bn_index_size = the file's
 *                  rows, bn_index_read returns the file's payload bytes, invalid rows (by the rule above) are never returned, and
 *                  later appends continue the ids.  Every digest is recomputed on the device while the rows are placed, and every
 *                  element is tested for finiteness; the index exists only if all of it agrees with the file.
 *   Refusals       *out stays NULL, nothing is leaked, the message is in bn_last_error.
 *                  BN_ERR_MODEL_LOAD (the file is unreadable or malformed; bn_index_load, bn_index_file_info and
 *                  bn_index_file_verify alike): a path that cannot be opened, wrong magic, wrong version, a header digest
 *                  mismatch, dim == 0 or above 2^20, rows above 2^32 - 66 (the largest capacity), chunk_rows == 0, an n_chunks not
 *                  ceil(rows / chunk_rows), non-zero reserved bytes, a size other than the header's (truncated or trailing
 *                  bytes); and, from bn_index_load and bn_index_file_verify, which read the payload: a chunk digest mismatch (the
 *                  message names the first bad chunk), a non-finite element, a valid_rows that disagrees with the payload.
 *                  BN_ERR_INVALID_ARG (the caller's mistake): NULL where data is required, a capacity_rows below the file's rows
 *                  or above 2^32 - 66, a struct_size below the struct's, a chunk_rows above 2^32 - 1, and a `path` of
 *                  bn_index_save whose temporary cannot be created (a directory that does not exist or is not writable).
 *                  BN_ERR_BACKEND: a write, flush or rename of bn_index_save that fails after that (a full disk), and runtime errors.
 *   No device      bn_index_file_info and bn_index_file_verify need none.  bn_index_load checks the header and the file size on the
 *                  host FIRST (a malformed file is BN_ERR_MODEL_LOAD on every machine) and then returns BN_ERR_NO_DEVICE without a
 *                  gfx950 device.
 *   Determinism    no floating-point atomics; the digests are integer sums.
 *
 * bn_index_file_verify recomputes every digest on the CPU and applies the finite and valid_rows rules; *first_bad_chunk (may be
 * NULL) receives the first chunk with a digest mismatch or, failing that, a non-finite element, and UINT64_MAX otherwise.
 */
typedef struct bn_index_file_info_t { /* the function of the same stem needs a type name of its own in C */
    uint64_t rows;
    uint64_t valid_rows;
    uint32_t dim;
    uint32_t chunk_rows;
    uint32_t n_chunks;
    uint32_t version;
} bn_index_file_info_t;
bn_status bn_index_save(bn_index *x, const char *path, size_t chunk_rows);
bn_status bn_index_load(int32_t device, const char *path, size_t capacity_rows, bn_index **out);
bn_status bn_index_file_info(const char *path, bn_index_file_info_t *out, size_t struct_size);
bn_status bn_index_file_verify(const char *path, uint64_t *first_bad_chunk);

/*
 * Per-site species priors: the location / date prior of the reference's RangeFilter (src/rangefilter.rs) as an immutable
 * device table P[n_sites][n_species] (f32, row-major), applied to every row of a step.  The reference filters one
 * prediction list at a time on the host, by species name, after the cut to K; a table on the device serves a pool of a
 * thousand recorders at a thousand sites inside the step, and can pick the K best species AMONG THOSE THAT OCCUR at the
 * site.  A table row is the meta model's raw output for (lat, lon, week), not RangeFilter::predict's list, which holds only
 * scores >= threshold: filter_predictions keeps every species absent from its list, so fed its own predict output the
 * reference never drops anything.
 *
 *   Entry p        p >= 0: the meta model's score of the species at the site.  p < 0 (BN_PRIOR_UNKNOWN): the meta model does
 *                  not know the species; it is kept unchanged (rangefilter.rs:368-375).  Non-finite: refused at creation.
 *   Per species    for logit z of species j in a row at site s, p = P[s][j]:
 *                    admitted = p < 0 || p >= threshold
 *                    conf     = sigmoid(z), the step's own (bit-exact to the reference's)
 *                    conf'    = conf * p under BN_PRIOR_RERANK when p >= 0 (one f32 multiply, fused with nothing), else conf
 *   SELECT         (flags without BN_PRIOR_AFTER_TOPK) the row holds the first K = min(top_k, n_species) admitted species in
 *                  the order: descending conf' under f32::total_cmp, ties by ascending species index.  With has_min the
 *                  entries for which conf' >= min_conf fails (IEEE comparison: NaN fails) are then removed.  count may be
 *                  below K: fewer species admitted, or cut by the minimum.  This order is defined by the sort alone; the
 *                  reference has no counterpart to it, and the BinaryHeap tie arrangement the step's own top-K reproduces
 *                  does not apply.  top_k is 1..1024.
 *   AFTER_TOPK     exactly filter_predictions(the step's own top-K row, the site's full score row, threshold, rerank) with
 *                  species matched by index: entries that are not admitted are dropped, the survivors' confidences
 *                  multiplied when reranking, then (when reranking) sorted descending under total_cmp, equal ones keeping
 *                  their order.  K, has_min and min_conf are the step's own; those given at attach are ignored.
 *   Bits           a row's result depends only on the row's logits, its site's table row, threshold, the flags and K / has_min
 *                  / min_conf: not on the batch size, the row's position or the entry point.  No floating-point atomics, no
 *                  order that depends on scheduling; two runs give the same bits.
 *   Step           bn_ctx_attach_prior makes every later bn_step_device / bn_step_windows / bn_step_live of the context also
 *                  produce the prior-filtered rows of that step, on the context's stream, after the plan and the step's own
 *                  top-K and outside the captured plan graph (capture_fallbacks stays 0).  The packed rows reach pinned
 *                  memory as the step's own do; bn_step_prior_results is valid after bn_ctx_synchronize, until the next
 *                  step.  Rows of bn_step_device / bn_step_windows are at the context's site (bn_ctx_prior_site, 0 after
 *                  every attach); row i of bn_step_live is at source_sites[source_out[i]], or at the context's site when
 *                  the map is NULL.  The site ids reach the device in pinned memory the kernel reads in place, without a
 *                  synchronisation.  The step's own outputs are unchanged, bit for bit.  bn_infer*, tickets and bn_group_*
 *                  carry no prior results.
 *   Refusals       BN_ERR_INVALID_ARG with a message, nothing changed (a previous attachment stays): NULL where data is
 *                  required, n_sites == 0, n_species != the model's num_species at attach, a non-finite table entry or
 *                  threshold, unknown flag bits, a prior on another device, top_k outside 1..1024 for SELECT, for AFTER_TOPK
 *                  whatever the step's top-K refuses, a site id outside 0..n_sites, a live step whose pool has more sources
 *                  than the attached map, bn_ctx_prior_site without a prior.  Without a gfx950 device create and apply
 *                  return BN_ERR_NO_DEVICE.
 *   Lifetime       a context that attached a prior keeps it alive: bn_prior_free and bn_ctx_destroy may come in either order.
 *   Threading      a prior is immutable and may be attached to any number of contexts; bn_prior_apply_host / bn_prior_read
 *                  serialise per prior.  A new week or a moved recorder is a new prior and a re-attach (26.7 MB for 1024
 *                  sites x 6522 species).
 */
typedef struct bn_prior bn_prior;
#define BN_PRIOR_UNKNOWN (-1.0f) /* table entry of a species the meta model does not know */
#define BN_PRIOR_SELECT 0u       /* the K best admitted species of all n_species (default) */
#define BN_PRIOR_AFTER_TOPK 1u   /* filter_predictions over the step's own top-K row */
#define BN_PRIOR_RERANK 2u       /* conf' = conf * p for known species */
bn_status bn_prior_create(int32_t device, size_t n_sites, size_t n_species, const float *table, float threshold, uint32_t flags,
                          bn_prior **out);
void bn_prior_free(bn_prior *p);
size_t bn_prior_sites(const bn_prior *p);
size_t bn_prior_species(const bn_prior *p);
float bn_prior_threshold(const bn_prior *p);
uint32_t bn_prior_flags(const bn_prior *p);
/* table rows first_site .. first_site + count back on the host: out [count * n_species] */
bn_status bn_prior_read(const bn_prior *p, size_t first_site, size_t count, float *out);
/* the prior on host logits [rows * n_species], row r at sites[r]; the same kernels as a step runs (for AFTER_TOPK behind the
 * step's top-K kernel under top_k / has_min / min_conf).  idx_out / conf_out [rows * k_stride], k_stride >= min(top_k,
 * n_species); count_out [rows].  Slots past a row's count up to K are zero. */
bn_status bn_prior_apply_host(const bn_prior *p, const float *logits, size_t rows, const int32_t *sites, size_t top_k, int32_t has_min,
                              float min_conf, size_t k_stride, uint32_t *idx_out, float *conf_out, uint32_t *count_out);
/* p == NULL detaches (the other arguments are then ignored).  source_sites [n_source_sites]: the site of every source of
 * the live pools this context steps, or NULL */
bn_status bn_ctx_attach_prior(bn_ctx *c, bn_prior *p, const int32_t *source_sites, size_t n_source_sites, size_t top_k, int32_t has_min,
                              float min_conf);
/* the site of every row of bn_step_device / bn_step_windows (and of bn_step_live without a map) */
bn_status bn_ctx_prior_site(bn_ctx *c, int32_t site);
/* pinned host views of the last step's prior rows: idx / conf [batch, k_stride], count [batch] */
bn_status bn_step_prior_results(const bn_ctx *c, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride);

/*
 * Detection events: a device-resident tracker that turns the per-window logits rows of many sources into DETECTIONS -- species j
 * was heard at source s from window a to window b, h times, with a peak confidence and the window of that peak.  It is the one
 * stage of the live pipeline that carries state from a step to the next: one small record per (source, species), n_sources x
 * n_species fixed at creation, updated by every step of a context it is attached to, like heads and priors.  Only finished
 * events leave the device.  The reference has no counterpart (its CLI prints per-window lists, src/bin/birdnet-analyze.rs:556-650);
 * the definition below is the contract.
 *
 *   Per row        for a row that is window k of source s, and species j with logit z:
 *                    conf = sigmoid(z), the step's own (bit-exact to the reference's)
 *                    under BN_TRACK_PRIOR, with p = P[site][j] of the prior passed with the update or attached to the context:
 *                      a species that is not admitted (bn_prior: p < 0 || p >= threshold) is never a hit;
 *                      conf = conf' of the prior (conf * p under its BN_PRIOR_RERANK for p >= 0)
 *                    hit  = conf >= enter_conf (IEEE comparison: NaN is not a hit)
 *   Open event     (hits > 0, last hit window `last`): misses = (k - last - 1) + (hit ? 0 : 1); misses > max_gap CLOSES the event.
 *                  A closed event is emitted iff hits >= min_hits, otherwise dropped silently.
 *   Hit            opens a new event (first = k, sum = 0, hits = 0, peak = conf, peak_window = k) or extends the open one; then
 *                  last = k, hits += 1, sum += conf (f32, in increasing k: deterministic); conf > peak (strict: the earliest peak
 *                  wins a tie) sets peak and peak_window.
 *   Windows        are absolute numbers below 2^31: a window that never arrives counts as a miss.  Per source they must be
 *                  strictly increasing over the tracker's life, until bn_track_reset.
 *   Flush / reset  bn_track_flush closes every open event of a source (or of all: source -1) under the same min_hits rule: end of
 *                  stream.  The source's last window stays.  bn_track_reset forgets a source's open events and its last window.
 *   Events         an update's (a step's, a flush's) events reach the caller sorted by (source, species, first_window); that key is
 *                  unique.  At most max_events (given at creation) are kept per update: the rest are counted in `dropped` and
 *                  lost, which ones is unspecified; with dropped == 0 the list is fully determined.
 *   Bits           an event depends only on that (source, species)'s sequence of (k, logit, prior row) and the configuration: not
 *                  on how windows were batched into steps, on a row's position, on the context that ran the step or on the entry
 *                  point.  Two runs give the same bytes.  No floating-point atomics; integer atomics only reserve output slots.
 *   Step           bn_ctx_attach_track makes every later bn_step_windows / bn_step_live of the context also update the tracker,
 *                  on the context's stream, after the plan, the step's own top-K, the head and the prior, outside the captured
 *                  plan graph (capture_fallbacks stays 0).  Row i of bn_step_windows is window first_window + i of the context's
 *                  source (bn_ctx_track_source, 0 after every attach); row i of bn_step_live is window window_out[i] of source
 *                  source_out[i].  bn_step_device rows carry no window number and are not tracked.  Sources and windows reach
 *                  the device in pinned memory the kernel reads in place.  Under BN_TRACK_PRIOR the rows' sites are those the
 *                  attached prior gives them.  The step's own outputs, head rows and prior rows are unchanged, bit for bit.
 *   Ordering       updates are applied in the order the step calls are made (a live pool: the scheduling order).  The tracker
 *                  keeps the event of its last update; every update makes its stream wait for it and records a new one, so
 *                  several contexts stepping one pool with sync = 0 serialise their tracker kernels only, not their plans.
 *   Stale rows     a bn_step_live row whose window does not exceed its source's last has already been taken from the pool: it is
 *                  skipped and counted in stale_rows.  This arises only after bn_live_reset without bn_track_reset.
 *   Refusals       BN_ERR_INVALID_ARG with a message, nothing changed: NULL where data is required, zero sizes, a non-finite
 *                  enter_conf, min_hits == 0, unknown flags, n_species != the model's at attach, another device, a source out of
 *                  range, a live pool with more sources than the tracker, BN_TRACK_PRIOR without a prior (passed or attached),
 *                  bn_track_update_host rows that do not increase per source, a bn_step_windows whose first window does not
 *                  exceed the source's last (refused before anything runs).  Without a gfx950 device create, update and flush
 *                  return BN_ERR_NO_DEVICE.
 *   Lifetime       a context that attached a tracker keeps it alive: bn_track_free and bn_ctx_destroy may come in either order.
 *   Threading      one thread at a time per tracker (and the contexts it is attached to).
 */
typedef struct bn_track bn_track;
#define BN_TRACK_PRIOR 1u /* hits are those of admitted species, on the prior's conf' */
typedef struct bn_event {
    int32_t source;
    uint32_t species;
    uint32_t first_window; /* first HIT window */
    uint32_t last_window;  /* last HIT window */
    uint32_t hits;
    uint32_t peak_window;
    float peak_conf;
    float mean_conf; /* sum / (float)hits, one f32 divide */
} bn_event;
bn_status bn_track_create(int32_t device, size_t n_sources, size_t n_species, float enter_conf, uint32_t min_hits, uint32_t max_gap,
                          size_t max_events, uint32_t flags, bn_track **out);
void bn_track_free(bn_track *t);
size_t bn_track_sources(const bn_track *t);
size_t bn_track_species(const bn_track *t);
/* diagnostic: open events of a source (source -1: of all), every pending update waited for; 0 for a NULL tracker or a source out
 * of range */
size_t bn_track_open_events(const bn_track *t, int32_t source);
/* ONE update, by the step's kernel, on host logits [rows * n_species]: row r is window windows[r] of source sources[r], at site
 * sites[r] of `prior` under BN_TRACK_PRIOR (both may be NULL without it).  The first min(events, cap) events of the sorted list go
 * to events_out, *n_out of them; *dropped counts the rest. */
bn_status bn_track_update_host(bn_track *t, const float *logits, size_t rows, const int32_t *sources, const uint64_t *windows,
                               const bn_prior *prior, const int32_t *sites, bn_event *events_out, size_t cap, size_t *n_out,
                               size_t *dropped);
bn_status bn_track_flush(bn_track *t, int32_t source, bn_event *events_out, size_t cap, size_t *n_out, size_t *dropped);
bn_status bn_track_reset(bn_track *t, int32_t source);
/* t == NULL detaches */
bn_status bn_ctx_attach_track(bn_ctx *c, bn_track *t);
/* the source of every row of bn_step_windows */
bn_status bn_ctx_track_source(bn_ctx *c, int32_t source);
/* pinned host view of the events of the last tracked step, sorted; valid after bn_ctx_synchronize until the next step.  Any
 * output may be NULL. */
bn_status bn_step_track_results(bn_ctx *c, const bn_event **events, size_t *n, size_t *dropped, size_t *stale_rows);

/*
 * Live ingest: a device-resident pool of per-source ring buffers for continuous audio (many recorders, each producing a
 * window every `step` seconds).  Callers push PCM as it arrives, in the storage format (i16: half the PCIe bytes, and no
 * overlap sample crosses the bus twice); bn_step_live batches the ready windows of ALL sources into one context batch, cut on
 * the device.  Per source, every window is bit-identical to bn_step_windows over a bn_recording of that source's
 * concatenated pushes.
 *
 *   Windows     chunk_audio's (src/bin/birdnet-analyze.rs:707-743) over everything pushed to a source since its creation or
 *               last reset: window k starts at sample k * step.  Before close window k is ready once k*step + S <= pushed;
 *               at close every remaining window with k*step < pushed becomes ready, samples past the end reading 0.  A
 *               source closed with 0 samples has no windows.  i16 converts as v / 32768.0f.
 *   Geometry    S % 4 == 0, 1 <= step <= S, S + step <= ring_samples < 2^31; otherwise BN_ERR_INVALID_ARG.
 *   Scheduling  FIFO by readiness: a window gets a sequence number when it becomes ready (in k order within a push or close,
 *               in array order within a push_many); a step takes the lowest sequence numbers, its rows in that order.  Every
 *               window is scheduled exactly once, a source's windows in increasing k.
 *   Room        host accounting only: needed_from = min(pushed, next_unscheduled_k * step), room = ring_samples - (pushed -
 *               needed_from).  A push past the room is refused whole (push_many: the whole call, nothing written).
 *   Ordering    the pool has a stream of its own.  A step makes the context's stream wait for the pool's last scatter; a
 *               scatter waits for every gather (of any context) that read ring space it overwrites; pinned staging is
 *               reused only after the scatter that read it completed.  Several contexts may step one pool with sync = 0.
 *   Refusals    BN_ERR_INVALID_ARG (message in bn_last_error, pool unchanged): a source out of range, an unknown format, a
 *               push or close after close (until reset), max_windows > bn_ctx_max_batch, a context on another device or of
 *               another segment length, NULL where data is required.  Without a gfx950 device: BN_ERR_NO_DEVICE.
 *   Threading   one thread at a time per pool, like a context.
 *
 * Resampling pools (bn_live_create_rates): every source declares its own sample rate, and pushes are converted to dst_rate ON
 * THE DEVICE as they arrive, in the scatter, by the polyphase FIR of bn_recording_create_resampled (same table, same fmaf
 * chain; the last T - 1 source samples of every source are carried across pushes on the device).  Per source, every window is
 * bit-identical to bn_step_windows over bn_recording_create_resampled(concatenation of its pushes, src_rate, dst_rate,
 * zero_crossings).  segment / step / ring_samples are in output (dst_rate) samples, pushes and room in source samples.
 *
 *   Ring        f32 at dst_rate, whatever `format` the pushes have.
 *   Finality    output n reads source samples up to (n*M)/L + T/2 (L/M = dst/src reduced, T taps per phase), so after p
 *               pushed samples F(p) = ceil(max(0, p - T/2) * L / M) outputs are final (bn_live_resampled_samples); after
 *               close ceil(p * L / M), the length bn_recording_create_resampled reports, the taps past the end reading 0.
 *   Windows     a plain pool's with "pushed" replaced by the final outputs: window k is ready once k*step + S <= F(pushed);
 *               at close every window with k*step < ceil(pushed * L / M) becomes ready, zero-padded.  A resampling source
 *               is therefore T/2 source samples later than a plain one (0.5 ms at 48 -> 32 kHz).
 *   Room        host accounting only, in source samples: needed_from = min(F(pushed), next_unscheduled_k * step), room =
 *               floor((ring_samples + needed_from) * M / L) - pushed, the largest n for which ceil((pushed + n) * L / M) -
 *               needed_from <= ring_samples.  The ring thus always keeps space for the tail a close flushes (at most
 *               ceil(T/2 * L / M) + 1 outputs): a close is never refused for room.
 *   Geometry    as above, and ring_samples >= S + step + ceil((T/2 + 1) * L / M) for every resampled source, so that a source
 *               without room always has a ready window.  T <= 512 and L * T <= 2^22; a pair beyond that is refused at creation.
 *   Reset       the new stream starts at sample 0 and sees zeros before it, not the old stream's history.
 *   Same rate   a source with src_rate == dst_rate behaves as a plain pool's (i16 -> v / 32768 is exact in f32).
 */
typedef struct bn_live bn_live;
bn_status bn_live_create(int32_t device, int32_t n_sources, int32_t format, size_t segment_samples, size_t step_samples,
                         size_t ring_samples, bn_live **out);
/* a resampling pool: source s delivers `format` PCM at src_rates[s] (> 0), the windows are cut at dst_rate (> 0);
 * zero_crossings as bn_recording_create_resampled (0 => 16).  One table per distinct rate of the pool. */
/* A pool whose pushes carry a PCM layout ("PCM layouts" above): one layout per pool, n_samples of a push counts FRAMES, every
 * window is bit-identical to the mono f32 pool fed the layout rule's samples.  src_rates == NULL: no resampling (dst_rate and
 * zero_crossings are ignored); else one rate per source, as bn_live_create_rates.  Mono int16 / float pushes are stored as they
 * are; for any other layout the ring holds f32 and the scatter converts the frames as they land.  Refusals as
 * bn_recording_create_layout, and those of bn_live_create / bn_live_create_rates. */
bn_status bn_live_create_layout(int32_t device, int32_t n_sources, const bn_pcm_layout *layout, size_t struct_size,
                                size_t segment_samples, size_t step_samples, size_t ring_samples, uint32_t dst_rate,
                                const uint32_t *src_rates, uint32_t zero_crossings, bn_live **out);
bn_status bn_live_create_rates(int32_t device, int32_t n_sources, int32_t format, size_t segment_samples, size_t step_samples,
                               size_t ring_samples, uint32_t dst_rate, const uint32_t *src_rates, uint32_t zero_crossings,
                               bn_live **out);
/* F(pushed) above (closed != 0: ceil(pushed * L / M)); `pushed` itself for src_rate == dst_rate, 0 for a zero rate.  Needs no
 * device. */
size_t bn_live_resampled_samples(uint32_t src_rate, uint32_t dst_rate, uint32_t zero_crossings, uint64_t pushed, int32_t closed);
/* the rate a source of a resampling pool was created with; 0 for a plain pool, a NULL pool or a source out of range */
uint32_t bn_live_source_rate(const bn_live *l, int32_t source);
void bn_live_free(bn_live *l);
/* append samples to one source; the caller's buffer is not referenced after return */
bn_status bn_live_push(bn_live *l, int32_t source, const void *pcm, size_t n_samples);
/* n chunks in one call (one staging block, one scatter launch); chunk i goes to sources[i] */
bn_status bn_live_push_many(bn_live *l, size_t n, const int32_t *sources, const void *const *pcm, const size_t *n_samples);
/* end of stream: the tail windows become ready (zero-padded) */
bn_status bn_live_close(bn_live *l, int32_t source);
/* drop the source's unscheduled windows and start a new stream at sample 0 (steps already taken still complete correctly) */
bn_status bn_live_reset(bn_live *l, int32_t source);
/* ready, unscheduled windows of a source (source < 0: of all sources); 0 for a NULL pool or a source out of range */
size_t bn_live_ready(const bn_live *l, int32_t source);
/* samples a push to this source may add now (source samples of that source in a resampling pool) */
size_t bn_live_room(const bn_live *l, int32_t source);
/* diagnostic: HIP events the pool holds to order scatters after gathers (those of gathers in flight plus recycled ones);
 * completed gathers are retired on every push and step, so this stays bounded by the steps in flight */
size_t bn_live_event_count(const bn_live *l);
/* diagnostic: ready, unscheduled window `window` of a source as host f32 [segment_samples], cut by the step's kernel */
bn_status bn_live_read_window(const bn_live *l, int32_t source, uint64_t window, float *host_out);
/* the hot call: take up to max_windows (<= bn_ctx_max_batch) ready windows, cut them into the context's input buffer and run
 * plan + top-K + D2H exactly as bn_step_windows does (results through bn_step_results / bn_ctx_output_device).  Row i is
 * window window_out[i] of source source_out[i]; *n_out = rows taken (0: nothing ran).  A refusal takes no window.  A backend
 * error of the step itself, after the windows were taken, returns with *n_out and the provenance naming them: they are
 * scheduled and their results are lost. */
bn_status bn_step_live(bn_ctx *c, bn_live *l, size_t max_windows, size_t top_k, int32_t has_min, float min_conf,
                       int32_t *source_out, uint64_t *window_out, size_t *n_out, int32_t sync);

/* Diagnostic, needs no device: parse the file, build the launch plan (all graph
 * outputs when all_outputs != 0, else logits + embeddings only) and write a
 * text description (one line per launch, then totals) into buf.  Returns the
 * number of bytes the full text needs (excluding the NUL); *status receives the
 * outcome of the parse / detection / planning steps. */
/* First contact with a model file, needs no device: opset, graph input / outputs, what detect_model_type decides (detection.rs:15-145),
 * every operator type with its node count and whether the lowering has a rule for it ("NOT MAPPED" + the first such node), and the
 * outcome of planning -- for every graph output and for the audio path (logits + embeddings) -- with the refusal's node and reason.
 * The reference loads whatever ONNX Runtime loads (classifier.rs:340-350); this says in one call what stands between a real export
 * and the native path.  *status: BN_OK, BN_ERR_UNSUPPORTED_MODEL (a plan was refused) or BN_ERR_MODEL_LOAD (unreadable file).
 * Returns the number of bytes the full text needs (excluding the NUL). */
size_t bn_model_survey(const char *onnx_path, char *buf, size_t cap, bn_status *status);

/* How launches size their grids where a choice exists between one launch's latency and the work per block (chunks per block of the
 * small-map MBConv kernels, row tiles of the 1x1-conv GEMMs).  BN_SHARING_ALONE (default): for a device the launch has to itself -- the
 * lowest latency of one batch.  BN_SHARING_SHARED: for a device whose CUs are shared by several batches in flight -- the reference's way
 * to throughput is several BatchInferenceContexts (classifier.rs:826-867); a launch then gets a share of the CUs whatever its grid, and
 * bigger blocks amortise their prologues and weight traffic (BirdNET v2.4, four contexts: +7 % segments/s; one batch alone: +13 % time).
 * BN_SHARING_AUTO: SHARED while more than one context is alive on the device.  Results do not depend on the mode (bit for bit);
 * process-wide; graphs captured under one form are re-captured under the other.  No ort counterpart: ORT has no such notion. */
#define BN_SHARING_AUTO (-1)
#define BN_SHARING_ALONE 0
#define BN_SHARING_SHARED 1
void bn_set_sharing_mode(int32_t mode);
size_t bn_plan_describe(const char *onnx_path, int32_t model_type_override, int32_t all_outputs,
                        char *buf, size_t cap, bn_status *status);

/* Message of the last failing call on this thread; returns its length. */
size_t bn_last_error(char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* BIRDNET_HIP_H */
