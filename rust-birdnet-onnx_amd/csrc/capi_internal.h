// What the translation units of the C ABI share: the plumbing every entry point repeats (the error macro, launch and device checks,
// the packed top-K block TopkRows, results_to_host, the pinned ring PinnedRing, scoped scratch: step_common.cpp), what they need of
// capi.cpp's private state (index.hip: bn_index_* and the host side every search over an index shares; head.hip: bn_head_*; rank.hip: bn_head_rank_index; cluster.hip: bn_index_assign, bn_index_cluster; live.cpp: bn_step_live; recording.cpp: bn_step_window_list) and of each other (prior.hip:
// bn_prior_*; track.hip: bn_track_*; recording.cpp: bn_recording_* and what bn_infer_windows and bn_step_windows need of a recording).  A step's rows reach its stages as an argument (StepRows), never through a context's state.
// Every device buffer, pinned buffer, stream and event is a member of device_mem.h's owner types: a handle's destructor waits, its members free.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/birdnet_hip.h"
#include "device_mem.h"
#include "last_error.h"
#include "pcm_layout.h"
#include "query_source.h"

// a failed runtime call ends the enclosing function with BN_ERR_BACKEND and the call's text in the message
#define BN_HIP_TRY(expr)                                                                                                   \
    do {                                                                                                                   \
        hipError_t e_ = (expr);                                                                                            \
        if (e_ != hipSuccess) return bn::set_last_error(BN_ERR_BACKEND, std::string(#expr) + " failed: " + hipGetErrorString(e_)); \
    } while (0)

namespace bn {
// ---- step_common.cpp ----
// before a launch: drops the thread's pending launcher refusal and the runtime's sticky error, both of unrelated earlier calls
void clear_launch_state();
// after a launch: a launcher's refusal (kernels.h launch_error) is BN_ERR_INVALID_ARG "`what` refused: why", a runtime error
// BN_ERR_BACKEND "`what` launch failed: ..."
bn_status check_launch(const char *what);
// BN_ERR_NO_DEVICE (message set) without a gfx950 device / for an ordinal the runtime does not list
bn_status require_any_device();
bn_status require_device(int32_t device);
// *k = min(top_k, n); refuses k == 0 and a k beyond the top-K heap's LDS
bn_status check_top_k(size_t n, size_t top_k, size_t *k);

// The top-K rows of `batch` rows packed [idx: batch*k][conf: batch*k][count: batch] in one block of 32-bit words, so that they cross
// the bus as ONE region; a device block, a pinned mirror, or both.  The offsets are known here and nowhere else.
struct TopkRows {
    struct View {
        uint32_t *idx;
        float *conf;
        uint32_t *count;
        size_t k;
    };
    struct ConstView {
        const uint32_t *idx;
        const float *conf;
        const uint32_t *count;
        size_t k;
    };
    DeviceBuf<uint32_t> d;
    PinnedBuf<uint32_t> h;
    size_t cap = 0;                     // words
    size_t last_batch = 0, last_k = 0;  // the rows last enqueued into the block (mark); last_k == 0: none since it was (re)allocated

    static size_t words(size_t batch, size_t k) { return batch * (2 * k + 1); }
    static size_t bytes(size_t batch, size_t k) { return words(batch, k) * sizeof(uint32_t); }
    static View view(uint32_t *base, size_t batch, size_t k) { return {base, reinterpret_cast<float *>(base + batch * k), base + 2 * batch * k, k}; }
    static ConstView view(const uint32_t *base, size_t batch, size_t k) {
        return {base, reinterpret_cast<const float *>(base + batch * k), base + 2 * batch * k, k};
    }
    // room for max_batch rows of k; grows by free + allocate after waiting for `drain` (may be NULL: nothing can be using the block),
    // which forgets the marked rows; empty on failure
    bn_status reserve(size_t max_batch, size_t k, hipStream_t drain, bool device, bool pinned);
    void release();
    void mark(size_t batch, size_t k) { last_batch = batch, last_k = k; }
    // the pinned mirror's marked rows for a *_step_results accessor (any output may be NULL); BN_ERR_INVALID_ARG `none_msg` if none
    bn_status results(const char *none_msg, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride) const;
};

// Device results -> pinned host buffers on `stream`, by ONE kernel launch storing straight into the (device-mapped) pinned memory
// (topk.hip, copy_out_kernel) instead of one copy-engine transfer per region; hipMemcpyAsync transfers where a switch asks for them
// or the kernel cannot take a region (step_common.cpp).
struct OutRegion {
    void *host;
    const void *dev;
    size_t bytes;
};
bn_status results_to_host(hipStream_t stream, const OutRegion *regs, int n);
// top-K of `rows` device rows of n logits into a packed block, on `stream`; a launch the heap's LDS refuses is an error
bn_status enqueue_topk_rows(hipStream_t stream, const float *d_logits, size_t rows, size_t n, size_t k, int32_t has_min, float min_conf,
                            const TopkRows::View &out, uint32_t *d_flags);

// Four pinned blocks of one size in rotation, for lists the host writes per step and a kernel reads in place (no copy): a block is
// rewritten only after the work that read it has completed (its event).  acquire, fill, enqueue the reader, commit; a slot that was
// acquired but not committed (the enqueue failed) is the next acquire's.
struct PinnedRing {
    static constexpr int SLOTS = 4;
    PinnedBuf<void> h[SLOTS];
    void *d[SLOTS] = {};  // a block's device alias
    Event ev[SLOTS];
    bool busy[SLOTS] = {};  // ev was recorded behind a reader of the block
    int next = 0;

    hipError_t create(size_t bytes);  // empty on failure
    void release();
    hipError_t acquire(int *slot, void **host);  // waits for the slot's last reader
    void *device_ptr(int slot) const { return d[slot]; }
    hipError_t commit(int slot, hipStream_t stream);  // the event behind what was just enqueued on `stream`; advances the ring
};

// device buffers, one pinned buffer and a stream of one call: on every way out the stream is waited for, the buffers freed and the
// stream, if owned, destroyed
struct Scratch {
    Stream own_stream;              // the stream, if it is the call's own
    hipStream_t stream = nullptr;   // the stream that uses the buffers: own_stream or the caller's
    std::vector<DeviceBuf<void>> bufs;
    PinnedBuf<void> pinned;
    ~Scratch() {
        if (stream) (void)hipStreamSynchronize(stream);
    }
    hipError_t create_stream(unsigned flags) {
        hipError_t e = own_stream.create(flags);
        stream = own_stream;
        return e;
    }
    template <class T>
    hipError_t alloc(T **p, size_t bytes, bool zero = false) {
        DeviceBuf<void> b;
        hipError_t e = b.alloc(bytes);
        if (e != hipSuccess) return e;
        *p = static_cast<T *>(b.get());
        bufs.push_back(std::move(b));
        return zero ? hipMemsetAsync(*p, 0, bytes, stream) : hipSuccess;  // on the stream that uses the buffer: ordered before every kernel
    }
};

// ---- capi.cpp ----
// the embedding output of a context's last run: device, stream, rows [last_batch, row_elems]; BN_ERR_INVALID_ARG (message set)
// for a model without embeddings
struct CtxEmbedding {
    int device = 0;
    hipStream_t stream = nullptr;
    const float *d_rows = nullptr;
    size_t row_elems = 0;
    size_t last_batch = 0;
};
bn_status ctx_embedding(const bn_ctx *c, CtxEmbedding *out);
// The identity of a step's rows, for the stages that need it (prior: the site of a row; tracker: its source and window)
struct StepRows {
    size_t batch;
    bool numbered;            // false: plain bn_step_device, the tracker is not run
    const int32_t *sources;   // NULL: every row belongs to the attachment's source / the context's site
    const uint64_t *windows;  // NULL: row i is window first_window + i
    uint64_t first_window;
};
// the body of bn_step_device, bn_step_windows, bn_step_window_list and bn_step_live
bn_status step_device(bn_ctx *c, const float *d_pcm, const StepRows &rows, size_t top_k, int32_t has_min, float min_conf, int32_t sync);
// the refusals of bn_step_windows (n_sources == 0) and bn_step_live (count == 0) that the attached prior and tracker make, before
// anything is enqueued or taken from a pool: prior_step_check, track_step_check
bn_status ctx_step_check(const bn_ctx *c, size_t n_sources, uint64_t first_window, size_t count);
// what bn_step_live and bn_step_window_list need of a context: its device, stream and input buffer [max_batch, sample_count]; BN_ERR_INVALID_ARG
// (message set) for a top_k that bn_step_device would refuse
struct CtxStepInput {
    int device = 0;
    hipStream_t stream = nullptr;
    float *d_input = nullptr;
    size_t sample_count = 0;
    size_t max_batch = 0;
    bool tracked = false;  // a tracker is attached: its refusals of a row's own window number apply
};
bn_status ctx_step_input(const bn_ctx *c, size_t top_k, CtxStepInput *out);
// index.hip -> head.hip (bn_head_fit_index): the stored rows of an index, every pending append waited for
struct IndexRows {
    int device = 0;
    const float *slab = nullptr;   // [size, dpad], rows normalised, zero-padded to dpad (a multiple of 128)
    const uint8_t *valid = nullptr;  // [size]: 0 for a row stored as zeros
    size_t dim = 0, dpad = 0, size = 0;
};
bn_status index_rows(bn_index *x, IndexRows *out);
// index.hip -> rank.hip (bn_head_rank_index): what a scan of the slab on the index's own stream needs.  The device is made current
// and the stream ordered after a pending bn_index_add_ctx, without waiting; the buffers are the search's own (one thread at a time
// per index): candidates [max_wg][lists][256] + lengths [max_wg][lists], results [out_lists][256] + counts with pinned mirrors
namespace topm {
struct Cand;
}
struct IndexScan {
    int device = 0;
    hipStream_t stream = nullptr;
    const float *slab = nullptr;     // rows padded to a multiple of 64, [.., dpad]
    const uint8_t *valid = nullptr;  // likewise
    size_t dim = 0, dpad = 0, size = 0, cap_pad = 0;  // cap_pad: the rows the slab has room for
    int max_wg = 0;
    size_t lists = 0, out_lists = 0;
    topm::Cand *d_cand = nullptr, *d_out = nullptr, *h_out = nullptr;
    int *d_cand_len = nullptr;
    uint32_t *d_count = nullptr, *h_count = nullptr;
    const uint16_t *tags = nullptr;  // [cap_pad] row tags; NULL until a tag is first set: every tag is 0
};
bn_status index_scan_state(bn_index *x, IndexScan *out);
// index.hip -> subset.hip, peaks.hip, seq.hip, rank.hip: index_merge_kernel enqueued on `stream`: one wave per query walks the n_wg workgroups' sorted
// lists cand[g][q][256] (lengths cand_len[g][q]; a workgroup's lists are ALWAYS index_scan.h's LP = 64 apart, whatever IndexScan::lists
// says: that only sets how many lists a pass of run_scan_passes takes) into out[q][M], count[q]
bn_status index_enqueue_merge(hipStream_t stream, const topm::Cand *cand, const int *cand_len, size_t n_queries, int n_wg, int M, topm::Cand *out,
                              uint32_t *count);
// ---- index.hip: the host side that the searches over an index share (index, subset, peaks, seq, above, group, ivf, sq8; rank
// all but the queries) ----
// A search is its own refusals (the shared ones: check_top_m, check_search_buffers, query_source.h's check_query_ids), its own empty
// case, its own state or plan, and ONE for_each_round whose function runs the round's passes (run_scan_passes, or its own pass loop
// ending in copy_back_results; run_threshold_passes for the threshold searches) and copies out (scatter_results).
// The dynamic-LDS opt-in of a file's scan kernels beyond 64 KB, once per device, under the capture gate (it may not overlap a
// capture).  One object per file, with static storage.
struct LdsOptIn {
    struct Kernel {
        const void *fn;
        size_t bytes;
    };
    std::mutex mu;
    uint64_t ready = 0;  // devices (ordinal < 64) on which the kernels have been opted in
    hipError_t prepare(int dev, std::initializer_list<Kernel> kernels);
};
// The refusals of a top-M search's arguments that need neither a handle nor a device, in bn_index_search's order and words: top_m
// outside 1..256, then m_stride < top_m (check_top_m); a call with queries that lacks them or an output (check_search_buffers).  Two
// calls, since bn_index_search_peaks refuses its radius between them
bn_status check_top_m(size_t top_m, size_t m_stride);
bn_status check_search_buffers(const void *queries, size_t n_queries, const uint64_t *id_out, const float *score_out, const uint32_t *count_out);
// n_tiles >= 1 tiles in contiguous runs of tiles_per_wg, at most max_wg workgroups, none of them empty
struct WgSplit {
    uint32_t tiles_per_wg, n_wg;
};
inline WgSplit split_tiles(uint32_t n_tiles, size_t max_wg) {
    const uint32_t tpw = (uint32_t)((n_tiles + max_wg - 1) / max_wg);
    return {tpw, (n_tiles + tpw - 1) / tpw};
}
// f(std::integral_constant<int, NB>) for the NB = ceil(n / 16) in 1..4 blocks of 16 lists that a pass of n <= 64 lists fills: the
// choice of a scan kernel's instantiation
template <class F>
inline void by_blocks(int n, F &&f) {
    switch ((n + 15) / 16) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}
// The queries of a round, made ready in the index's own query buffers on its stream: host rows normalised as appended rows are, or
// stored rows gathered by id.  d_q [n, dpad], d_qvalid [n], d_qid [n] (NULL for host rows) stay the index's; radius is the source's
struct StagedQueries {
    const float *d_q = nullptr;
    const uint8_t *d_qvalid = nullptr;
    const uint32_t *d_qid = nullptr;
    int64_t radius = -1;
    size_t dpad = 0;
    // from query row p0 on: what the launch of a pass takes
    StagedQueries at(size_t p0) const { return {d_q + p0 * dpad, d_qvalid + p0, d_qid ? d_qid + p0 : nullptr, radius, dpad}; }
};
// The round loop of every search over an index (query_source.h, each_round over IndexScan::out_lists rows): the round's `count`
// queries from `first` on (`unit` rows each; ids checked by the caller) are staged, then fn runs its passes and copies out.  The
// staging orders the stream after a pending bn_index_add_ctx and waits for it before it overwrites a buffer the round before has read
using RoundFn = std::function<bn_status(size_t first, size_t count, const StagedQueries &q)>;
bn_status for_each_round(bn_index *x, const QuerySource &src, size_t n, size_t unit, const RoundFn &fn);
// One round of a scan over n_lists <= out_lists staged lists with the index's own buffers, synchronous: per pass of s.lists lists
// launch_scan(p0, np) enqueues the scan of lists [p0, p0 + np) on s.stream (n_wg workgroups, candidates into s.d_cand /
// s.d_cand_len) and is checked as the launch `what` (seq.hip passes a copy of the state with fewer lists per pass: a list is a sequence
// there, and a pass holds as many as fit the 64 query rows); `merge` (index_enqueue_merge's signature) then finishes the pass's lists
// into s.d_out / s.d_count.  After the last pass copy_back_results
using MergeEnqueue = bn_status (*)(hipStream_t, const topm::Cand *, const int *, size_t, int, int, topm::Cand *, uint32_t *);
bn_status run_scan_passes(const IndexScan &s, size_t n_lists, uint32_t n_wg, int M, const char *what,
                          const std::function<void(size_t p0, int np)> &launch_scan, MergeEnqueue merge = index_enqueue_merge);
// s.d_out [n][M] / s.d_count [n] into the pinned mirrors s.h_out / s.h_count; the stream is waited for
bn_status copy_back_results(const IndexScan &s, size_t n, int M);
// rows [n][M] of a round's results in the pinned mirrors (h_count[i] entries each) -> rows [first, first + n) of the caller's arrays
// at stride m_stride; entries past a count stay
void scatter_results(const IndexScan &s, size_t first, size_t n, size_t M, size_t m_stride, uint64_t *id_out, float *score_out, uint32_t *count_out);
// A round of a threshold search (above.hip, group.hip): min_score[0 .. nq) into d_thr once the stream has run dry (the last pass of
// the round before has read it), then pass(p0, np) for each pass of `width` queries
bn_status run_threshold_passes(hipStream_t stream, float *d_thr, const float *min_score, size_t nq, size_t width,
                               const std::function<bn_status(size_t p0, int np)> &pass);
// ivf.hip -> sq8.hip (bn_sq8_search's re-rank): the gathered scan and the multi-wave merge, enqueued on `stream`.  The scan runs
// n_queries x nprobe x segments units; unit (q, p, seg) scans tiles [seg * seg_tiles, + seg_tiles) of the list probes[q * nprobe + p]
// (members[offsets[c] .. + counts[c]), ids of stored rows; BN_CLUSTER_NONE: no list) for query row q of `q`, with bn_index_search's
// score bits, into cand[unit][256] (sorted, first M kept) and cand_len[unit].  The merge gives query q the first M of its `units`
// consecutive sorted lists: out[q][M], count[q].  Every pointer is device memory
struct IvfGather {
    const float *slab = nullptr, *q = nullptr;  // [.., dpad]
    uint32_t dpad = 0;
    const uint32_t *qid = nullptr;  // with radius >= 0: rows within radius of qid[q] are left out
    int64_t radius = -1;
    const uint32_t *probes = nullptr, *counts = nullptr, *offsets = nullptr, *members = nullptr;
    uint32_t nprobe = 1, seg_tiles = 1, segments = 1;
};
bn_status ivf_enqueue_scan(hipStream_t stream, const IvfGather &g, size_t n_queries, int M, topm::Cand *cand, int *cand_len);
bn_status ivf_enqueue_merge(hipStream_t stream, const topm::Cand *cand, const int *cand_len, size_t n_queries, size_t units, int M, topm::Cand *out,
                            uint32_t *count);
// index.hip <-> index_io.hip (bn_index_save, bn_index_load): the slab itself.  index_io_state makes the device current and orders the
// index's stream after a pending bn_index_add_ctx, without waiting.  index_adopt_rows ends a load: rows [0, n) of an EMPTY index
// (n <= its capacity) were written, with their valid bytes and zeroed pad columns, by work that has completed
struct IndexIo {
    int device = 0;
    hipStream_t stream = nullptr;
    float *slab = nullptr;     // [cap, dpad]
    uint8_t *valid = nullptr;  // [cap]
    size_t dim = 0, dpad = 0, size = 0, cap = 0;
};
bn_status index_io_state(bn_index *x, IndexIo *out);
bn_status index_adopt_rows(bn_index *x, size_t n);
// index.hip <-> index_copy.hip (bn_index_append_rows, bn_index_append_subset): both slabs of a copy of n rows of src to the end of
// dst (dst != src, same device and dim, n >= 1).  index_copy_begin refuses an append past dst's capacity as every append does, makes the
// device current, orders dst's stream after a pending bn_index_add_ctx of EITHER index without waiting, and gives dst a tag plane
// (zeroed on that stream) when src has one and dst has none.  The dst pointers name the first new row.  index_copy_commit ends the
// copy: the n rows, their valid bytes and, where dst has a plane, their tags were written by work that has completed.
// index_copy_shape is the part of index_copy_begin that changes nothing: the capacity refusal, and what the plan of a copy needs
struct IndexCopy {
    int device = 0;
    hipStream_t stream = nullptr;  // dst's
    size_t dpad = 0, first = 0;    // first: dst's size, the id of the first new row
    int max_wg = 0;
    const float *src_slab = nullptr;    // [size, dpad]
    const uint8_t *src_valid = nullptr;
    const uint16_t *src_tags = nullptr;  // NULL: src never tagged
    float *dst_slab = nullptr;
    uint8_t *dst_valid = nullptr;
    uint16_t *dst_tags = nullptr;  // NULL: neither index has a plane
};
bn_status index_copy_shape(const bn_index *dst, size_t n, size_t *dpad, int *max_wg);
bn_status index_copy_begin(bn_index *dst, const bn_index *src, size_t n, IndexCopy *out);
void index_copy_commit(bn_index *dst, size_t n);
// subset.hip -> index_copy.hip: the index a subset borrows and its list on the device ([n] ascending ids; NULL for an empty subset)
struct SubsetList {
    bn_index *x = nullptr;
    size_t n = 0;
    const uint32_t *d_ids = nullptr;
};
SubsetList subset_list(const bn_subset *s);
// index.hip <-> cluster.hip (bn_index_assign, bn_index_cluster): the clustering buffers of an index, owned by cluster.hip, NULL until
// a call first needs them; bn_index_free hands them to cluster_state_free with the index's stream idle
struct ClusterState;
ClusterState **index_cluster_state(bn_index *x);
void cluster_state_free(ClusterState *s);
// index.hip <-> above.hip (bn_index_search_above and its _ids form): the threshold search's buffers of an index, owned by above.hip, NULL
// until a call first needs them; bn_index_free hands them to above_state_free with the index's stream idle
struct AboveState;
AboveState **index_above_state(bn_index *x);
void above_state_free(AboveState *s);
// index.hip <-> group.hip (bn_index_group_above and its _ids form): the grouped threshold search's buffers of an index, owned by
// group.hip, NULL until a call first needs them; bn_index_free hands them to group_state_free with the index's stream idle
struct GroupState;
GroupState **index_group_state(bn_index *x);
void group_state_free(GroupState *s);
// index.hip -> match.hip: a reference on an index (bn_index_free drops the caller's; the slab lives until the last is gone), its
// device and stream, the current tag plane ([capacity] u16 on the device, NULL until a tag is first set), and index_normalise_kernel
// enqueued on `stream`: n rows at d_src (row stride src_stride floats) -> d_dst [n, dpad] + d_valid [n], the index's rule and bits
void index_ref(bn_index *x);
void index_unref(bn_index *x);
int index_device(const bn_index *x);
hipStream_t index_stream(const bn_index *x);
const uint16_t *index_tags(const bn_index *x);
bn_status index_enqueue_normalise(hipStream_t stream, const float *d_src, size_t src_stride, size_t n, size_t dim, float *d_dst, size_t dpad,
                                  uint8_t *d_valid);
// match.hip -> capi.cpp: an index attached to a context (a snapshot of its rows, its own scratch and result buffers; holds a reference
// to the index).  match_ranges: the row ranges (workgroups per query pass) of a snapshot of n_tiles 64-row tiles
struct MatchAttach;
WgSplit match_ranges(uint32_t n_tiles);
bn_status match_attach(bn_index *x, int device, bool has_embedding, size_t embedding_dim, size_t max_batch, size_t top_m, int32_t has_min,
                       float min_score, MatchAttach **out);
void match_detach(MatchAttach *a);  // the context's stream must be idle
// normalise + scan + merge-and-pack + results to pinned memory, enqueued on the context's stream behind the step's own work
bn_status match_step(MatchAttach *a, hipStream_t stream, const float *d_emb, size_t batch);
bn_status match_step_results(const MatchAttach *a, const uint64_t **id, const float **score, const uint32_t **tag, const uint32_t **count,
                             size_t *m_stride, size_t *rows_searched);
// head.hip -> rank.hip: what a kernel needs of a head (weights [cpad = classes rounded up to 16][dpad], bias [cpad], padding zero)
struct HeadView {
    int device;
    size_t dim, dpad, classes, cpad;
    uint32_t flags;
    const float *d_W, *d_b;
};
HeadView head_view(const bn_head *h);
// head.hip -> capi.cpp: a head attached to a context (its own result buffers; holds a reference to the head)
struct HeadAttach;
bn_status head_attach(bn_head *h, int device, bool has_embedding, size_t embedding_dim, size_t max_batch, size_t top_k, int32_t has_min,
                      float min_conf, HeadAttach **out);
void head_detach(HeadAttach *a);  // the context's stream must be idle
// prep + apply + top-K + results to pinned memory, enqueued on the context's stream behind the step's own work
bn_status head_step(HeadAttach *a, hipStream_t stream, const float *d_emb, size_t batch);
bn_status head_step_results(const HeadAttach *a, const float **logits, const uint32_t **idx, const float **conf, const uint32_t **count,
                            size_t *k_stride, size_t *n_classes);
// prior.hip -> capi.cpp: a prior attached to a context (its own result buffers; holds a reference to the prior)
struct PriorAttach;
bn_status prior_attach(bn_prior *p, int device, size_t num_species, size_t max_batch, const int32_t *source_sites, size_t n_source_sites, size_t top_k,
                       int32_t has_min, float min_conf, PriorAttach **out);
void prior_detach(PriorAttach *a);  // the context's stream must be idle
bn_status prior_set_site(PriorAttach *a, int32_t site);
// refuses a pool with more sources than the attached map
bn_status prior_step_check(const PriorAttach *a, size_t n_sources);
// the prior kernel + results to pinned memory, enqueued on the context's stream behind the step's own top-K; under a site map the
// rows of a live step (rows.sources) run at their sources' sites, every other row at the context's site;
// step_rows: the step's own rows on the device (AFTER_TOPK filters them)
bn_status prior_step(PriorAttach *a, hipStream_t stream, const float *d_logits, const TopkRows::ConstView &step_rows, const StepRows &rows);
bn_status prior_step_results(const PriorAttach *a, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride);
// prior.hip -> track.hip: what a kernel needs of a prior's table (rows padded to tstride floats)
struct PriorView {
    int device;
    const float *d_table;
    size_t n_sites, n_species, tstride;
    float threshold;
    int rerank;
};
PriorView prior_view(const bn_prior *p);
// the prior of an attachment (NULL attachment: NULL) and the site of one of its rows: the map's for `source` of a live step under a
// map, else the context's site
const bn_prior *prior_of(const PriorAttach *a);
int32_t prior_site_of(const PriorAttach *a, int32_t source);
// track.hip -> capi.cpp: a tracker attached to a context (its own pinned row lists and event lists; holds a reference)
struct TrackAttach;
bn_status track_attach(bn_track *t, int device, size_t num_species, size_t max_batch, TrackAttach **out);
void track_detach(TrackAttach *a);  // the context's stream must be idle
bn_status track_set_source(TrackAttach *a, int32_t source);
// the refusals of a step that need nothing of the step: BN_TRACK_PRIOR without an attached prior; bn_step_live (n_sources > 0): a pool
// with more sources than the tracker; bn_step_windows (count > 0): a first window that does not exceed the source's last
bn_status track_step_check(const TrackAttach *a, const PriorAttach *prior, size_t n_sources, uint64_t first_window, size_t count);
// the tracker's update for the step's rows + its event list to pinned memory, enqueued on the context's stream behind the step's own
// work; only for numbered rows: row i is window rows.windows[i] of rows.sources[i] (bn_step_live) or, with sources == NULL, window
// rows.first_window + i of the attachment's source (bn_step_windows)
bn_status track_step(TrackAttach *a, hipStream_t stream, const float *d_logits, const StepRows &rows, const PriorAttach *prior);
bn_status track_step_results(TrackAttach *a, const bn_event **events, size_t *n, size_t *dropped, size_t *stale_rows);
// ---- recording.cpp ----
// the polyphase table of the resampler (design in include/birdnet_hip.h): L/M = dst/src reduced, T taps per phase; zc 0 => 16
struct ResampleTable {
    uint32_t L = 1, M = 1, T = 0;
    std::vector<float> coef;  // [L][T]
};
// L, M and T alone (coef left empty): what the table would be, without building it
ResampleTable resample_factors(uint32_t src_rate, uint32_t dst_rate, uint32_t zc);
ResampleTable make_resample_table(uint32_t src_rate, uint32_t dst_rate, uint32_t zc);
// a caller's bn_pcm_layout read through the size it was compiled with (a longer struct of a later header: its first fields);
// BN_ERR_INVALID_ARG for NULL or a struct shorter than this header's.  The layout itself is checked by
// pcm_layout_problem (pcm_layout.h)
bn_status read_pcm_layout(const bn_pcm_layout *layout, size_t struct_size, PcmLayout *out);
// recording.cpp -> capi.cpp (bn_infer_windows, bn_step_windows): the refusals of windows [first, first + count) of S samples every
// `step` of a recording (a null recording, the segment, the step, the range), then the wait for the last sample they read of an
// asynchronous upload; *device (may be NULL): where the recording lives
bn_status check_windows(const bn_recording *r, size_t S, size_t step, size_t first, size_t count, int32_t *device);
// those windows, checked, into dst [count, S] by the window kernel enqueued on `stream` of `device` (the thread's device); a
// recording on another device is refused
bn_status enqueue_windows(hipStream_t stream, int32_t device, float *dst, const bn_recording *r, size_t S, size_t step, size_t first, size_t count);
}  // namespace bn
