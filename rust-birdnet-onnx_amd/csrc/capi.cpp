// C ABI of libbirdnet_hip.so (include/birdnet_hip.h).
#include "../../include/birdnet_hip.h"

#include <hip/hip_runtime.h>

#include "hip_gate.h"

#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "capi_internal.h"
#include "detect.h"
#include "engine.h"
#include "kernels.h"
#include "plan_rules.h"

using namespace bn;

namespace {

thread_local std::string g_err;

bn_status fail(bn_status st, const std::string &msg) {
    g_err = msg;
    return st;
}

struct PlanDev {
    std::unique_ptr<Plan> plan;
    DeviceBuf<float> d_consts;
};

bool device_is_gfx950(int dev) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
    return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

// ---- persistent host staging pool ----
// The reference's prepare_input copies every caller slice into one contiguous buffer on the calling thread
// (batch_context.rs:199-211).  At 10 000+ segments per second that copy is 6+ GB/s -- more than one core moves -- so
// the copies of a batch are handed to a small pool of long-lived threads (one task per segment) while the calling
// thread copies too and puts each finished chunk on the wire.  Started on first use, joined at library unload; no
// thread is created per call.  BN_STAGE_THREADS overrides the worker count (0 = the caller copies alone).
struct StageTask {
    const void *src;
    void *dst;
    size_t bytes;
    std::atomic<uint32_t> *done;  // incremented (release) when the copy has landed
};
class StagePool {
   public:
    static StagePool &get() {
        static StagePool pool;
        return pool;
    }
    void push(const StageTask *tasks, size_t n) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (size_t k = 0; k < n; k++) q_.push_back(tasks[k]);
        }
        if (n > 1) cv_.notify_all();
        else cv_.notify_one();
    }
    // the caller helps: run one queued task if there is one
    bool try_run_one() {
        StageTask t;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (q_.empty()) return false;
            t = q_.front();
            q_.pop_front();
        }
        run(t);
        return true;
    }
    size_t workers() const { return th_.size(); }

   private:
    StagePool() {
        unsigned hw = std::thread::hardware_concurrency();
        long n = hw > 2 ? std::min<long>(6, (long)hw / 2) : 0;
        if (sw_is_set(sw::BN_STAGE_THREADS)) n = std::max<long>(0, std::min<long>(64, (long)sw_i64(sw::BN_STAGE_THREADS)));
        for (long k = 0; k < n; k++) th_.emplace_back([this] { loop(); });
    }
    ~StagePool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_) t.join();
    }
    static void run(const StageTask &t) {
        memcpy(t.dst, t.src, t.bytes);
        t.done->fetch_add(1, std::memory_order_release);
    }
    void loop() {
        for (;;) {
            StageTask t;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return stop_ || !q_.empty(); });
                if (q_.empty()) return;  // stop_
                t = q_.front();
                q_.pop_front();
            }
            run(t);
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<StageTask> q_;
    std::vector<std::thread> th_;
    bool stop_ = false;
};

}  // namespace

struct bn_model {
    // one reference for the handle bn_model_load returned + one per context created from it: a context may outlive
    // the caller's bn_model_free (the reference's BatchInferenceContext is an owned value with no lifetime tie to
    // the Classifier, src/batch_context.rs:70-85), the model goes when the last holder does
    std::atomic<int> refs{1};
    int device = 0;
    OnnxModel onnx;  // kept for the lazily built all-outputs plan
    bn_model_config cfg{};
    IoMeta io;
    std::unique_ptr<PlanDev> main_plan;  // computes logits (+ embeddings) only
    std::unique_ptr<PlanDev> full_plan;  // every graph output
    std::mutex mu;
};

struct bn_ctx {
    bn_model *model = nullptr;
    PlanDev *pd = nullptr;
    size_t max_batch = 0;
    uint32_t flags = 0;
    bn::Stream stream, copy_stream;  // before every buffer their work touches: they go last (device_mem.h)
    DeviceBuf<float> d_arena;
    DeviceBuf<float> d_input;
    PinnedBuf<float> h_out;  // pinned staging for logits + embeddings
    size_t h_out_elems = 0;
    size_t device_bytes = 0;
    bool holds_model = false;  // counted in model->refs (set once creation succeeded)
    bool counted = false;      // counted in the device's live-context count (kernels.h device_shared)
    bool in_flight = false;  // a cancelled/timed-out run may still be executing
    size_t last_batch = 0;
    // top-K scratch
    DeviceBuf<uint32_t> d_tk_idx, d_tk_cnt, d_tk_flags;
    DeviceBuf<float> d_tk_conf;
    size_t tk_cap = 0;  // elements of idx/conf
    // bn_step_device: the top-K rows of a step in one device block and one pinned mirror, so they cross the bus as ONE copy (each
    // async copy is a ~7 us blit launch); bn_infer_submit fills the device block too, its mirror is the slot's
    bn::TopkRows step;
    bn::HeadAttach *head = nullptr;  // bn_ctx_attach_head: run after every step's own work (head.hip)
    bn::PriorAttach *prior = nullptr;  // bn_ctx_attach_prior: the same, on the step's logits rows (prior.hip)
    bn::TrackAttach *track = nullptr;  // bn_ctx_attach_track: the same, for the steps whose rows carry window numbers (track.hip)
    bn::MatchAttach *match = nullptr;  // bn_ctx_attach_index: the step's embedding rows matched against an index's snapshot (match.hip)
    // ---- asynchronous host-slice path (bn_infer_submit / bn_infer_collect): a ring of two batches per context.
    // Both slots own their device input, pinned input and pinned output buffers (allocated on first use), so a ticket
    // in flight shares nothing with the synchronous entry points (bn_infer_windows / bn_step_*) but the arena and the
    // top-K block, and those are ordered by the context's stream.
    struct HostSlot {
        DeviceBuf<float> d_input;
        PinnedBuf<float> h_input, h_out;
        bn::TopkRows tk;  // pinned only
        bn::Event h2d_done, plan_done, out_done;
        bool used = false, busy = false;
        uint64_t ticket = 0;
        size_t batch = 0, k = 0;
    };
    HostSlot slots[2];
    uint64_t next_ticket = 1;
    struct GraphKey {
        size_t batch;
        bool shared;  // the grid form the launches were captured in (kernels.h device_shared)
        bool operator<(const GraphKey &o) const { return batch != o.batch ? batch < o.batch : shared < o.shared; }
    };
    std::map<GraphKey, hipGraphExec_t> graphs;
    std::map<GraphKey, uint64_t> graph_used;  // replay counter value at each graph's last launch (least recently used goes first)
    uint64_t graph_tick = 0;
    // bn_ctx_get_stats: how the plan reached the stream
    uint64_t n_captures = 0, n_instantiates = 0, n_replays = 0, n_eager_runs = 0, n_capture_fallbacks = 0, n_evictions = 0, n_input_copies = 0;
    std::string last_fallback;  // why the most recent capture did not become a graph
    ~bn_ctx();  // waits, detaches and drops the model reference; the members free themselves
};

namespace {

float *resolve(const bn_ctx *c, const Ref &r, const float *d_in) {
    const Plan &p = *c->pd->plan;
    switch (r.space) {
        case Space::INPUT: return const_cast<float *>(d_in) + r.offset;
        case Space::ARENA: return c->d_arena + p.storages[r.id].arena_off * (int64_t)c->max_batch + r.offset;
        case Space::CONSTS: return c->pd->d_consts + p.const_off[r.id] + r.offset;
        default: return nullptr;
    }
}

// The squeeze-excite a launch carries (PlanOp::se_fused), as the kernels take it: finished by a DWCONV / MBCONV ...
SeTail se_tail_of(const bn_ctx *c, const PlanOp &op, const float *d_in) {
    SeTail t{};
    if (!op.se_fused) return t;
    const auto &se = op.r.se;
    t.on = 1;
    t.se = op.se;
    t.w1 = resolve(c, se.w1, d_in);
    t.b1 = resolve(c, se.b1, d_in);
    t.w2t = resolve(c, se.w2t, d_in);
    t.b2 = resolve(c, se.b2, d_in);
    t.gate = resolve(c, se.gate, d_in);
    t.counter = reinterpret_cast<uint32_t *>(resolve(c, se.counter, d_in));  // one ticket word per sample
    t.cnt_bs = c->pd->plan->storages[se.counter.id].elems;
    return t;
}
// ... or computed in a GEMM's prologue
SeInline se_inline_of(const bn_ctx *c, const PlanOp &op, const float *d_in) {
    const auto &se = op.r.se;
    SeInline si{};
    si.se = op.se;
    si.partial = resolve(c, se.partial, d_in);
    si.w1 = resolve(c, se.w1, d_in);
    si.b1 = resolve(c, se.b1, d_in);
    si.w2t = resolve(c, se.w2t, d_in);
    si.b2 = resolve(c, se.b2, d_in);
    return si;
}

void launch_op(const bn_ctx *c, const PlanOp &op, const float *d_in, int64_t batch) {
    const PlanOp::Operands &r = op.r;
    auto at = [&](const Ref &ref) { return resolve(c, ref, d_in); };
    float *out = at(r.out);
    const float *a = at(r.a);
    switch (op.kind) {
        case OpKind::ELT: {
            const float *eb[ELT_MAX_STAGES];
            for (int k = 0; k < ELT_MAX_STAGES; k++) eb[k] = at(r.chain[k]);
            launch_eltwise(c->stream, op.elt, out, a, eb, batch);
            break;
        }
        case OpKind::REDUCE: launch_reduce(c->stream, op.red, out, a, batch, op.red.pair ? at(r.pair_out) : nullptr); break;
        case OpKind::GEMM:
            if (op.se_fused) {  // squeeze-excite in the GEMM's prologue: only the LDS-DMA kernel carries it (planner rule I)
                const SeInline si = se_inline_of(c, op, d_in);
                if (!(op.gemm.w3 ? launch_gemm_dma3 : launch_gemm_dma)(c->stream, op.gemm, out, a, at(r.w), at(r.bias), at(r.residual), at(r.gate), batch, &si))
                    launch_error("GEMM with inline squeeze-excite: operands are not 16-byte aligned");
                break;
            }
            {
                FramePre pre = op.pre;  // the signal chain a framing GEMM applies while it loads its span (planner rule G)
                for (int k = 0; k < ELT_MAX_STAGES; k++) pre.sc[k] = k < pre.n ? at(r.chain[k]) : nullptr;
                if (op.gemm.fold == 2) {  // quarter-folded cosine bank
                    launch_gemm_fold2(c->stream, op.gemm, out, a, at(r.w), at(r.bias), at(r.fold2.tables),
                                      reinterpret_cast<const int32_t *>(at(r.fold2.colmap)), batch, &pre);  // int32 bits in a constant of floats
                    break;
                }
                launch_gemm(c->stream, op.gemm, out, a, at(r.w), at(r.bias), at(r.residual), at(r.gate), batch, &pre);
            }
            break;
        case OpKind::CONV: launch_conv(c->stream, op.conv, out, a, at(r.w), at(r.bias), at(r.residual), batch); break;
        case OpKind::DWCONV: {
            SeTail tail = se_tail_of(c, op, d_in);
            launch_dwconv(c->stream, op.dw, out, a, at(r.w), at(r.bias), at(r.gap_out), batch, tail.on ? &tail : nullptr);
            break;
        }
        case OpKind::GAP: launch_gap_partial(c->stream, op.gap, out, a, batch); break;
        case OpKind::POOL: launch_pool(c->stream, op.pool, out, a, batch); break;
        case OpKind::MBCONV: {
            SeTail tail = se_tail_of(c, op, d_in);
            launch_mbconv(c->stream, op.mb, out, a, at(r.w), at(r.bias), at(r.w2), at(r.bias2), at(r.gap_out), batch, tail.on ? &tail : nullptr);
            break;
        }
        case OpKind::FFT: {
            StftPtrs sp{};
            sp.out = out;
            sp.in = a;
            sp.window = at(r.fft.window);
            sp.tw = reinterpret_cast<const float2 *>(at(r.fft.twiddles));  // (cos, sin) pairs
            sp.otab = at(r.fft.otab);
            sp.bias = at(r.bias);
            for (int k = 0; k < ELT_MAX_STAGES; k++) sp.pre[k] = at(r.chain[k]);
            sp.mstart = at(r.mel.start);
            sp.mcol = at(r.mel.entries);  // (column, value) pairs; mval stays unused
            sp.mel_bias = at(r.mel.bias);
            launch_stft(c->stream, op.fft, sp, batch);
            break;
        }
        case OpKind::SEFC: launch_se_fc(c->stream, op.se, out, at(r.hidden), a, at(r.w), at(r.bias), at(r.w2), at(r.bias2), batch); break;
    }
}

// Enqueue the whole plan for `batch` segments on the context's stream.
bn_status enqueue_plan(bn_ctx *c, const float *d_in, size_t batch, const volatile int32_t *cancel) {
    const Plan &p = *c->pd->plan;
    bool use_graph = !(c->flags & BN_CTX_NO_GRAPH);
    // the grids of some launches depend on whether the device is shared: decided here, once, for every launch of this batch -- captured
    // or not -- and for the graph's key
    const bool shared = bn::device_shared();
    const bn::SharedFormPin pin(shared);
    // The plan always reads the batch from the CONTEXT'S OWN input buffer: a captured graph then depends on the batch
    // size alone (one capture + instantiate per batch size, whatever buffers the caller cycles through), and a caller
    // that wants no copy at all writes its batch into that buffer (bn_ctx_input_device).  Any other device pointer is
    // copied in on the context's stream, ahead of the plan: 18 MB at batch 32, about 10 us.
    if (d_in != c->d_input) {
        static const bool runtime_copy = sw_int(sw::BN_INPUT_MEMCPY) != 0;
        if (runtime_copy) BN_HIP_TRY(hipMemcpyAsync(c->d_input, d_in, batch * (size_t)p.sample_count * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        else {
            launch_copy_dev(c->stream, c->d_input, d_in, batch * (size_t)p.sample_count * sizeof(float));
            bn_status st = check_launch("input copy");
            if (st != BN_OK) return st;
        }
        c->n_input_copies++;
        d_in = c->d_input;
    }
    if (use_graph) {
        bn_ctx::GraphKey key{batch, shared};  // one graph per (batch, form)
        auto it = c->graphs.find(key);
        if (it == c->graphs.end()) {
            hipGraph_t g = nullptr;
            // What sits between Begin and End is kernel launches on this stream and nothing else: the LDS opt-ins and
            // device queries the launchers used to make on first use (hipFuncSetAttribute on the first > 64 KB launch of
            // a plan -- the op the one-in-six invalidated capture of round 2 named) happen in prepare_device() at
            // context creation.  Captures of one process are still serialised (they are rare -- one per context and
            // batch size -- and a capture is not the place to find out what two of them do to each other), in the
            // thread-local mode so that what OTHER threads do to the device meanwhile (uploads, allocations of sibling
            // ranks) is none of this capture's business.
            std::unique_lock<std::shared_mutex> capture_lock(capture_gate());  // hip_gate.h: no allocation / free / synchronous copy of the library overlaps a capture
            (void)hipGetLastError();  // drop stale sticky errors of unrelated earlier calls
            BN_HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            c->n_captures++;
            hipError_t le = hipSuccess;
            std::string bad;
            (void)take_launch_error();
            std::string refused;
            for (auto &op : p.ops) {
                launch_op(c, op, d_in, (int64_t)batch);
                if (le == hipSuccess && (le = hipGetLastError()) != hipSuccess) bad = op.name;
                if (refused.empty())
                    if (const char *why = take_launch_error()) refused = "launch of '" + op.name + "' refused: " + why;
            }
            hipError_t e = hipStreamEndCapture(c->stream, &g);
            if (!refused.empty()) {
                if (g) (void)hipGraphDestroy(g);
                return fail(BN_ERR_INVALID_ARG, refused);
            }
            hipGraphExec_t ge = nullptr;
            hipError_t ie = hipSuccess;
            if (le == hipSuccess && e == hipSuccess) {
                ie = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
                c->n_instantiates++;
                if (ie != hipSuccess) ge = nullptr;
            }
            if (g) (void)hipGraphDestroy(g);
            if (!ge) {
                // The capture did not become a graph.  Nothing was enqueued, so the batch can still run launch by launch
                // below -- but never silently: the event is counted (bn_ctx_get_stats.capture_fallbacks), its cause kept
                // (.last_fallback) and reported on stderr once per context; BN_STRICT_GRAPH=1 turns it into an error.
                (void)hipGetLastError();
                c->n_capture_fallbacks++;
                c->last_fallback = le != hipSuccess ? "launch of '" + bad + "' failed during capture: " + hipGetErrorString(le)
                                   : e != hipSuccess ? std::string("hipStreamEndCapture: ") + hipGetErrorString(e)
                                                     : std::string("hipGraphInstantiate: ") + hipGetErrorString(ie);
                if (c->n_capture_fallbacks == 1)
                    fprintf(stderr, "libbirdnet_hip: graph capture for batch %zu failed (%s); running the plan launch by launch\n", batch,
                            c->last_fallback.c_str());
                static const bool strict = sw_int(sw::BN_STRICT_GRAPH) != 0;
                if (strict) return fail(BN_ERR_BACKEND, "graph capture failed: " + c->last_fallback);
                use_graph = false;
            } else {
                if (c->graphs.size() >= 16) {
                    // bounded cache: the least recently replayed graph goes (a caller cycling through up to 16 input
                    // buffers or batch sizes never re-captures; the whole cache used to be dropped at once); nothing of
                    // this context may still be replaying it
                    auto victim = c->graph_used.begin();
                    for (auto u = c->graph_used.begin(); u != c->graph_used.end(); ++u)
                        if (u->second < victim->second) victim = u;
                    (void)hipStreamSynchronize(c->stream);
                    auto g_old = c->graphs.find(victim->first);
                    if (g_old != c->graphs.end()) {
                        (void)hipGraphExecDestroy(g_old->second);  // (the gate is held exclusively here)
                        c->graphs.erase(g_old);
                    }
                    c->graph_used.erase(victim);
                    c->n_evictions++;
                }
                it = c->graphs.emplace(key, ge).first;
            }
        }
        if (use_graph) {
            c->graph_used[it->first] = ++c->graph_tick;
            BN_HIP_TRY(hipGraphLaunch(it->second, c->stream));
            c->n_replays++;
        }
    }
    if (!use_graph) {
        (void)hipGetLastError();  // drop stale sticky errors of unrelated earlier calls
        (void)take_launch_error();
        c->n_eager_runs++;
        for (auto &op : p.ops) {
            if (cancel && *cancel) return fail(BN_ERR_CANCELLED, "inference was cancelled");
            launch_op(c, op, d_in, (int64_t)batch);
            if (const char *why = take_launch_error()) return fail(BN_ERR_INVALID_ARG, "launch of '" + op.name + "' refused: " + why);
            hipError_t le = hipGetLastError();
            if (le != hipSuccess) return fail(BN_ERR_BACKEND, "launch of '" + op.name + "' failed: " + hipGetErrorString(le));
        }
    }
    return BN_OK;
}

bn_status drain_if_needed(bn_ctx *c) {
    if (c->in_flight) {
        BN_HIP_TRY(hipStreamSynchronize(c->stream));
        c->in_flight = false;
    }
    return BN_OK;
}

// the tail of an attach: `fresh` (NULL: detach only) takes the place of *slot once the context's stream is idle -- the previous
// attachment's buffers may still be read by a step in flight
template <class A>
bn_status install_attachment(hipStream_t stream, A *&slot, A *fresh, void (*detach)(A *)) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        detach(fresh);
        return fail(BN_ERR_BACKEND, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    detach(slot);
    slot = fresh;
    return BN_OK;
}

// Wait for the stream while honouring cancel / deadline (classifier.rs:527-554 polls every
// 10 ms; here the stream is polled, so a finished batch is never reported as timed out).
bn_status wait_stream(bn_ctx *c, const volatile int32_t *cancel, uint64_t timeout_ns) {
    if (!cancel && timeout_ns == 0) {
        BN_HIP_TRY(hipStreamSynchronize(c->stream));
        return BN_OK;
    }
    const auto start = std::chrono::steady_clock::now();
    int spins = 0;
    while (true) {
        hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return BN_OK;
        if (q != hipErrorNotReady) return fail(BN_ERR_BACKEND, std::string("hipStreamQuery: ") + hipGetErrorString(q));
        if (cancel && *cancel) {
            c->in_flight = true;
            return fail(BN_ERR_CANCELLED, "inference was cancelled");
        }
        if (timeout_ns) {
            const uint64_t el = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - start).count();
            if (el >= timeout_ns) {
                c->in_flight = true;
                return fail(BN_ERR_TIMEOUT, "inference timed out after " + std::to_string(timeout_ns) + " ns");
            }
        }
        if (++spins > 200) std::this_thread::sleep_for(std::chrono::microseconds(50));
        else std::this_thread::yield();
    }
}

bn_status make_plan(bn_model *m, const std::vector<int> &wanted, std::unique_ptr<PlanDev> &out) {
    auto pd = std::make_unique<PlanDev>();
    try {
        pd->plan = build_plan(m->onnx, wanted);
    } catch (const UnsupportedModel &e) {
        return fail(BN_ERR_UNSUPPORTED_MODEL, e.what());
    } catch (const std::exception &e) {
        return fail(BN_ERR_MODEL_LOAD, e.what());
    }
    BN_HIP_TRY(bn::use_device(m->device));
    if (!prepare_device(m->device)) return fail(BN_ERR_BACKEND, "device " + std::to_string(m->device) + " refused the kernels' dynamic-LDS opt-in");
    const Plan &p = *pd->plan;
    BN_HIP_TRY(pd->d_consts.alloc((size_t)p.consts_elems * sizeof(float)));
    for (size_t k = 0; k < p.consts.size(); k++)
        if (!p.consts[k].empty())
            BN_HIP_TRY(gated::Memcpy(pd->d_consts + p.const_off[k], p.consts[k].data(), p.consts[k].size() * sizeof(float), hipMemcpyHostToDevice));
    out = std::move(pd);
    return BN_OK;
}

bn_status finish_load(std::unique_ptr<bn_model> m, int32_t device, int32_t model_type_override, bn_model **out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(BN_ERR_NO_DEVICE, "no HIP device is visible; this path has no CPU fallback");
    if (device < 0 || device >= n) return fail(BN_ERR_NO_DEVICE, "device index " + std::to_string(device) + " out of range (" + std::to_string(n) + " visible)");
    if (!device_is_gfx950(device) && !sw_present(sw::BN_ALLOW_ANY_ARCH)) return fail(BN_ERR_NO_DEVICE, "device " + std::to_string(device) + " is not gfx950 (MI355X)");
    m->device = device;
    m->io = read_io_meta(m->onnx);
    if (m->onnx.inputs.size() != 1) return fail(BN_ERR_MODEL_DETECTION, "model has " + std::to_string(m->onnx.inputs.size()) + " inputs, expected 1");
    // Output shapes missing from the file: infer them by planning every output once.
    bool missing = false;
    for (auto &s : m->io.output_shapes) missing |= s.empty();
    if (missing) {
        std::vector<int> all;
        for (size_t k = 0; k < m->onnx.outputs.size(); k++) all.push_back((int)k);
        try {
            auto p = build_plan(m->onnx, all);
            for (size_t k = 0; k < p->outputs.size(); k++)
                if (m->io.output_shapes[k].empty()) {
                    m->io.output_shapes[k].push_back(-1);
                    for (auto d : p->outputs[k].dims) m->io.output_shapes[k].push_back(d);
                }
        } catch (const UnsupportedModel &e) {
            return fail(BN_ERR_UNSUPPORTED_MODEL, e.what());
        } catch (const std::exception &e) {
            return fail(BN_ERR_MODEL_LOAD, e.what());
        }
    }
    std::string reason;
    if (model_type_override == BN_MODEL_GENERIC) {
        // the range filter's meta model (rangefilter.rs:250-262): any single-input graph; output 0 is the result
        if (m->io.output_shapes.empty() || m->io.output_shapes[0].empty() || m->io.output_shapes[0].back() <= 0)
            return fail(BN_ERR_MODEL_DETECTION, "empty output shape");
        bn_model_config &c = m->cfg;
        memset(&c, 0, sizeof(c));
        c.model_type = BN_MODEL_GENERIC;
        c.sample_count = 1;
        for (size_t k = 1; k < m->io.input_shape.size(); k++) {
            if (m->io.input_shape[k] <= 0) return fail(BN_ERR_MODEL_DETECTION, "generic model needs a static per-row input shape");
            c.sample_count *= (uint64_t)m->io.input_shape[k];
        }
        c.num_species = (uint64_t)m->io.output_shapes[0].back();
        c.logits_output = 0;
        c.embedding_output = -1;
    } else if (!detect_model_type(m->io.input_shape, m->io.output_shapes, model_type_override, m->cfg, reason)) {
        return fail(BN_ERR_MODEL_DETECTION, reason);
    }
    std::vector<int> wanted{m->cfg.logits_output};
    if (m->cfg.embedding_output >= 0) wanted.push_back(m->cfg.embedding_output);
    bn_status st = make_plan(m.get(), wanted, m->main_plan);
    if (st != BN_OK) return st;
    if ((uint64_t)m->main_plan->plan->sample_count != m->cfg.sample_count) return fail(BN_ERR_MODEL_DETECTION, "input element count disagrees with the detected sample count");
    *out = m.release();
    return BN_OK;
}

}  // namespace

extern "C" {

int32_t bn_abi_version(void) { return BN_ABI_VERSION; }

int32_t bn_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < n; d++) ok += device_is_gfx950(d) ? 1 : 0;
    return ok;
}

bn_status bn_model_load(const char *onnx_path, int32_t device, int32_t model_type_override, bn_model **out) {
    if (!onnx_path || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    auto m = std::make_unique<bn_model>();
    try {
        m->onnx = parse_onnx_file(onnx_path);
    } catch (const std::exception &e) {
        return fail(BN_ERR_MODEL_LOAD, e.what());
    }
    return finish_load(std::move(m), device, model_type_override, out);
}

bn_status bn_model_load_buffer(const void *bytes, size_t len, int32_t device, int32_t model_type_override, bn_model **out) {
    if (!bytes || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    auto m = std::make_unique<bn_model>();
    try {
        m->onnx = parse_onnx(static_cast<const uint8_t *>(bytes), len);
    } catch (const std::exception &e) {
        return fail(BN_ERR_MODEL_LOAD, e.what());
    }
    return finish_load(std::move(m), device, model_type_override, out);
}

static void model_unref(bn_model *m) {
    if (m && m->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) {
        (void)bn::use_device(m->device);
        delete m;
    }
}
void bn_model_free(bn_model *m) { model_unref(m); }

int32_t bn_model_device(const bn_model *m) { return m ? m->device : -1; }

bn_status bn_model_io_info(const bn_model *m, bn_io_info *out) {
    if (!m || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    memset(out, 0, sizeof(*out));
    out->input_rank = (int32_t)std::min<size_t>(m->io.input_shape.size(), BN_MAX_RANK);
    for (int k = 0; k < out->input_rank; k++) out->input_shape[k] = m->io.input_shape[k];
    snprintf(out->input_name, BN_NAME_LEN, "%s", m->io.input_name.c_str());
    out->n_outputs = (int32_t)std::min<size_t>(m->io.output_names.size(), BN_MAX_OUTPUTS);
    for (int o = 0; o < out->n_outputs; o++) {
        out->output_rank[o] = (int32_t)std::min<size_t>(m->io.output_shapes[o].size(), BN_MAX_RANK);
        for (int k = 0; k < out->output_rank[o]; k++) out->output_shape[o][k] = m->io.output_shapes[o][k] <= 0 && k == 0 ? -1 : m->io.output_shapes[o][k];
        snprintf(out->output_name[o], BN_NAME_LEN, "%s", m->io.output_names[o].c_str());
    }
    return BN_OK;
}

bn_status bn_model_get_config(const bn_model *m, bn_model_config *out) {
    if (!m || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = m->cfg;
    return BN_OK;
}

bn_status bn_model_get_cost(const bn_model *m, bn_model_cost *out, size_t struct_size) {
    if (!m || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    const Plan &p = *m->main_plan->plan;
    bn_model_cost c{};
    c.macs_mfma = p.macs_mfma;
    c.macs_valu = p.macs_valu;
    c.weight_bytes = p.weight_bytes;
    c.activation_bytes = p.act_bytes;
    c.n_launches = (int32_t)p.ops.size();
    c.dft_gemm_macs = p.dft_gemm_macs;
    c.fft_flops = p.fft_flops;
    c.dft_performed_macs = p.dft_performed_macs;
    c.dft_fft_equiv_flops = p.dft_fft_equiv_flops;
    c.recompute_macs = p.recompute_macs;
    memcpy(out, &c, std::min(struct_size, sizeof(c)));  // never writes past the caller's struct (ABI 2: the struct grew in ABI 1 without a version bump)
    return BN_OK;
}

bn_status bn_detect_model_type(const int64_t *in_shape, size_t in_rank, const int64_t *out_shapes, const size_t *out_ranks, size_t n_out,
                               int32_t model_type_override, bn_model_config *out) {
    if (!in_shape || !out || (n_out && (!out_shapes || !out_ranks))) return fail(BN_ERR_INVALID_ARG, "null argument");
    std::vector<int64_t> in(in_shape, in_shape + in_rank);
    std::vector<std::vector<int64_t>> outs;
    size_t off = 0;
    for (size_t k = 0; k < n_out; k++) {
        outs.emplace_back(out_shapes + off, out_shapes + off + out_ranks[k]);
        off += out_ranks[k];
    }
    std::string reason;
    if (!detect_model_type(in, outs, model_type_override, *out, reason)) return fail(BN_ERR_MODEL_DETECTION, reason);
    return BN_OK;
}

static bn_status ensure_step_block(bn_ctx *c, size_t k);

void bn_set_sharing_mode(int32_t mode) { bn::device_sharing_mode(mode); }

// ---- the stream a context runs its plans on --------------------------------------------------------------------
// The runtime maps a process's streams onto hardware queues, GPU_MAX_HW_QUEUES (4 unless the caller exports more) PER PRIORITY LEVEL:
// a level's pool is filled up to that budget before two of its streams share a queue.  The null stream -- torch's, and most callers'
// -- and every default-priority stream of the process live in the default level's pool, so the fourth of four default-priority
// contexts shares a queue with a sibling and its steps wait behind that sibling's (0.63 ms per step against 0.46 ms).
// Streams that run plans are therefore created at ONE other level, the same for every context: they fill a pool of their own and
// leave the default pool to the null stream, the caller's streams and the library's helper streams (group ranks, uploads, live
// ingest, index / head / prior / tracker calls of their own), none of which runs plan-sized work next to the steps.  The greatest
// priority is the level taken: where a context's step meets default-priority work of the same process (a copy in front of a
// batch-1 request), the step is the work somebody waits for.  All contexts share the level, so nothing is prioritised AMONG them.
enum class PlanStreamLevel { Default, Greatest };
static constexpr PlanStreamLevel kPlanStreamLevel = PlanStreamLevel::Greatest;

static hipError_t create_plan_stream(bn::Stream &s, int dev) {  // the thread's device is `dev`
    static const bool own_pool = sw_on(sw::BN_CTX_STREAM_PRIO) && kPlanStreamLevel != PlanStreamLevel::Default;
    if (!own_pool) return s.create(hipStreamNonBlocking);
    struct Range {
        int least, greatest;
    };
    static std::mutex mu;
    static std::map<int, Range> ranges;  // asked once per device
    Range r{};
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = ranges.find(dev);
        if (it == ranges.end()) {
            hipError_t e = hipDeviceGetStreamPriorityRange(&r.least, &r.greatest);
            if (e != hipSuccess) return e;
            it = ranges.emplace(dev, r).first;
        }
        r = it->second;
    }
    if (r.least == r.greatest) return s.create(hipStreamNonBlocking);  // one level: there is no second pool to take
    return s.create(hipStreamNonBlocking, r.greatest);
}

bn_status bn_ctx_create(bn_model *m, size_t max_batch, uint32_t flags, bn_ctx **out) {
    if (!m || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (max_batch == 0 || max_batch > 65535) return fail(BN_ERR_INVALID_ARG, "max_batch must be in 1..65535");
    PlanDev *pd = m->main_plan.get();
    if (flags & BN_CTX_ALL_OUTPUTS) {
        std::lock_guard<std::mutex> lk(m->mu);
        if (!m->full_plan) {
            std::vector<int> all;
            for (size_t k = 0; k < m->onnx.outputs.size(); k++) all.push_back((int)k);
            bn_status st = make_plan(m, all, m->full_plan);
            if (st != BN_OK) return st;
        }
        pd = m->full_plan.get();
    }
    if (sw_present(sw::BN_NO_GRAPH)) flags |= BN_CTX_NO_GRAPH;
    auto c = std::make_unique<bn_ctx>();
    c->model = m;
    c->pd = pd;
    c->max_batch = max_batch;
    c->flags = flags;
    const Plan &p = *pd->plan;
    BN_HIP_TRY(bn::use_device(m->device));
    if (!prepare_device(m->device)) return fail(BN_ERR_BACKEND, "device " + std::to_string(m->device) + " refused the kernels' dynamic-LDS opt-in");
    BN_HIP_TRY(create_plan_stream(c->stream, m->device));
    const size_t arena_b = (size_t)p.arena_elems * max_batch * sizeof(float);
    const size_t in_b = (size_t)p.sample_count * max_batch * sizeof(float);
    BN_HIP_TRY(c->d_arena.alloc(arena_b));
    // the squeeze-excite ticket counters live here and must start at zero; on the context's OWN stream (a legacy-stream
    // hipMemset would serialise against -- and be seen by -- whatever sibling contexts are capturing or running)
    BN_HIP_TRY(hipMemsetAsync(c->d_arena, 0, arena_b, c->stream));
    BN_HIP_TRY(c->d_input.alloc(in_b));
    {
        size_t row = (size_t)p.outputs[m->cfg.logits_output].row_elems;
        if (m->cfg.embedding_output >= 0) row += (size_t)p.outputs[m->cfg.embedding_output].row_elems;
        c->h_out_elems = row * max_batch;
    }
    BN_HIP_TRY(c->h_out.alloc(c->h_out_elems * sizeof(float)));
    c->device_bytes = arena_b + in_b;
    m->refs.fetch_add(1, std::memory_order_relaxed);
    c->holds_model = true;
    // top-K / step buffers for the usual k (<= 32) are part of the context from the start: the step path allocates
    // nothing (a larger top_k still grows them on first use, behind a stream drain)
    if (m->cfg.model_type != BN_MODEL_GENERIC) {
        const size_t n = (size_t)p.outputs[m->cfg.logits_output].row_elems;
        bn_status st = ensure_step_block(c.get(), std::min<size_t>(32, n));
        if (st != BN_OK) return st;
    }
    BN_HIP_TRY(hipStreamSynchronize(c->stream));  // arena zeroed before anyone captures or launches
    bn::device_context_count_add(m->device, 1);
    c->counted = true;
    *out = c.release();
    return BN_OK;
}

bn_ctx::~bn_ctx() {
    if (counted) bn::device_context_count_add(model->device, -1);
    if (model) (void)bn::use_device(model->device);
    if (stream) (void)hipStreamSynchronize(stream);
    bn::head_detach(head);
    bn::prior_detach(prior);
    bn::track_detach(track);
    bn::match_detach(match);
    for (auto &kv : graphs) (void)gated::GraphExecDestroy(kv.second);
    if (copy_stream) (void)hipStreamSynchronize(copy_stream);
    if (holds_model) model_unref(model);
}

void bn_ctx_destroy(bn_ctx *c) { delete c; }

size_t bn_ctx_max_batch(const bn_ctx *c) { return c ? c->max_batch : 0; }

bn_status bn_ctx_get_stats(const bn_ctx *c, bn_ctx_stats *out, size_t struct_size) {
    if (!c || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    bn_ctx_stats st{};
    st.captures = c->n_captures;
    st.instantiates = c->n_instantiates;
    st.replays = c->n_replays;
    st.eager_runs = c->n_eager_runs;
    st.capture_fallbacks = c->n_capture_fallbacks;
    st.evictions = c->n_evictions;
    st.cached_graphs = c->graphs.size();
    st.input_copies = c->n_input_copies;
    snprintf(st.last_fallback, sizeof(st.last_fallback), "%s", c->last_fallback.c_str());
    memcpy(out, &st, std::min(struct_size, sizeof(st)));  // a caller built against an older, shorter struct gets its prefix
    return BN_OK;
}
size_t bn_ctx_device_bytes(const bn_ctx *c) { return c ? c->device_bytes : 0; }
void *bn_ctx_stream(const bn_ctx *c) { return c ? (void *)c->stream : nullptr; }

bn_status bn_ctx_input_device(const bn_ctx *c, float **d_ptr, size_t *capacity_floats) {
    if (!c || !d_ptr) return fail(BN_ERR_INVALID_ARG, "null argument");
    *d_ptr = c->d_input;
    if (capacity_floats) *capacity_floats = (size_t)c->pd->plan->sample_count * c->max_batch;
    return BN_OK;
}

bn_status bn_ctx_synchronize(bn_ctx *c) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    BN_HIP_TRY(bn::use_device(c->model->device));
    BN_HIP_TRY(hipStreamSynchronize(c->stream));
    c->in_flight = false;
    return BN_OK;
}

bn_status bn_infer_device(bn_ctx *c, const float *d_pcm, size_t batch, int32_t sync) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (batch == 0) return BN_OK;
    if (!d_pcm) return fail(BN_ERR_INVALID_ARG, "null input");
    if (reinterpret_cast<uintptr_t>(d_pcm) & 15u) return fail(BN_ERR_INVALID_ARG, "device input must be 16-byte aligned");
    if (batch > c->max_batch) return fail(BN_ERR_INVALID_ARG, "batch size " + std::to_string(batch) + " exceeds context max " + std::to_string(c->max_batch));
    BN_HIP_TRY(bn::use_device(c->model->device));
    bn_status st = drain_if_needed(c);
    if (st != BN_OK) return st;
    st = enqueue_plan(c, d_pcm, batch, nullptr);
    if (st != BN_OK) return st;
    c->last_batch = batch;
    if (sync) BN_HIP_TRY(hipStreamSynchronize(c->stream));
    return BN_OK;
}

// Tail shared by bn_infer_windows once the plan is enqueued on d_input: output copies to
// pinned staging, wait with cancel / timeout polling, copy out.
static bn_status finish_infer(bn_ctx *c, size_t batch, float *logits_out, float *emb_out, const volatile int32_t *cancel, uint64_t timeout_ns) {
    const Plan &p = *c->pd->plan;
    const bn_model_config &cfg = c->model->cfg;
    bn_status st = BN_OK;
    c->last_batch = batch;
    const OutputInfo &lo = p.outputs[cfg.logits_output];
    const size_t N = (size_t)lo.row_elems;
    float *h_logits = c->h_out;
    float *h_emb = c->h_out + N * c->max_batch;
    OutRegion regs[2] = {{h_logits, resolve(c, lo.ref, c->d_input), batch * N * sizeof(float)}, {nullptr, nullptr, 0}};
    int nreg = 1;
    size_t E = 0;
    if (emb_out && cfg.embedding_output >= 0) {
        const OutputInfo &eo = p.outputs[cfg.embedding_output];
        E = (size_t)eo.row_elems;
        regs[nreg++] = OutRegion{h_emb, resolve(c, eo.ref, c->d_input), batch * E * sizeof(float)};
    }
    st = results_to_host(c->stream, regs, nreg);
    if (st != BN_OK) return st;
    st = wait_stream(c, cancel, timeout_ns);
    if (st != BN_OK) return st;
    memcpy(logits_out, h_logits, batch * N * sizeof(float));
    if (E) memcpy(emb_out, h_emb, batch * E * sizeof(float));
    return BN_OK;
}

// ---- asynchronous host-slice path ------------------------------------------------------------------------------
static bn_status ensure_step_block(bn_ctx *c, size_t k);

static bn_status ensure_slot(bn_ctx *c, bn_ctx::HostSlot &sl, int index) {
    const Plan &p = *c->pd->plan;
    if (!c->copy_stream) BN_HIP_TRY(c->copy_stream.create(hipStreamNonBlocking));
    if (!sl.out_done) {  // the last of the three: a failed attempt is made again
        BN_HIP_TRY(sl.h2d_done.create(hipEventDisableTiming));
        BN_HIP_TRY(sl.plan_done.create(hipEventDisableTiming));
        BN_HIP_TRY(sl.out_done.create(hipEventDisableTiming));
    }
    if (sl.h_out) return BN_OK;  // the last of the three, likewise
    (void)index;
    const size_t in_b = (size_t)p.sample_count * c->max_batch * sizeof(float);
    BN_HIP_TRY(sl.d_input.alloc(in_b));
    BN_HIP_TRY(sl.h_input.alloc(in_b));
    BN_HIP_TRY(sl.h_out.alloc(c->h_out_elems * sizeof(float)));
    c->device_bytes += in_b;
    return BN_OK;
}

bn_status bn_infer_submit(bn_ctx *c, const float *const *segs, size_t batch, size_t top_k, int32_t has_min, float min_conf, uint64_t *ticket) {
    if (!c || !ticket) return fail(BN_ERR_INVALID_ARG, "null argument");
    *ticket = 0;
    if (batch == 0) return BN_OK;  // nothing to run (classifier.rs:681-683); ticket 0 collects to nothing
    if (!segs) return fail(BN_ERR_INVALID_ARG, "null argument");
    if (batch > c->max_batch) return fail(BN_ERR_INVALID_ARG, "batch size " + std::to_string(batch) + " exceeds context max " + std::to_string(c->max_batch));
    for (size_t b = 0; b < batch; b++)
        if (!segs[b]) return fail(BN_ERR_INVALID_ARG, "segment " + std::to_string(b) + " is null");
    const Plan &p = *c->pd->plan;
    const bn_model_config &cfg = c->model->cfg;
    const OutputInfo &lo = p.outputs[cfg.logits_output];
    const size_t N = (size_t)lo.row_elems;
    size_t k = std::min(top_k, N);  // 0: no top-K rows wanted
    if (k) {
        bn_status kst = check_top_k(N, top_k, &k);
        if (kst != BN_OK) return kst;
    }
    BN_HIP_TRY(bn::use_device(c->model->device));
    bn_ctx::HostSlot *slp = nullptr;
    int index = 0;
    for (int q = 0; q < 2 && !slp; q++) {
        const int cand = (int)((c->next_ticket + q) & 1u);
        if (!c->slots[cand].busy) { slp = &c->slots[cand]; index = cand; }
    }
    if (!slp) return fail(BN_ERR_INVALID_ARG, "two batches are already in flight on this context: collect one first");
    bn_ctx::HostSlot &sl = *slp;
    bn_status st = ensure_slot(c, sl, index);
    if (st != BN_OK) return st;
    if (c->in_flight) {  // a timed-out / cancelled batch may still be running: let everything settle first
        BN_HIP_TRY(hipStreamSynchronize(c->stream));
        BN_HIP_TRY(hipStreamSynchronize(c->copy_stream));
        c->in_flight = false;
    }
    if (k) {
        st = ensure_step_block(c, k);
        if (st != BN_OK) return st;
        st = sl.tk.reserve(c->max_batch, k, nullptr, false, true);  // (the slot is not busy: nothing writes its block)
        if (st != BN_OK) return st;
    }
    const size_t S = (size_t)p.sample_count;
    if (sl.used) {
        BN_HIP_TRY(hipEventSynchronize(sl.h2d_done));                      // the pinned buffer's last upload has left it
        BN_HIP_TRY(hipStreamWaitEvent(c->copy_stream, sl.plan_done, 0));  // the plan that read the device buffer is through
    }
    // stage + upload in chunks: pool threads (and this one) copy segment by segment; a chunk goes on the wire as soon
    // as its segments have landed in pinned memory, while the later chunks are still being copied
    {
        const size_t bytes_total = batch * S * sizeof(float);
        const size_t nchunk = bytes_total >= (2u << 20) ? std::min<size_t>(8, batch) : 1;
        StagePool &pool = StagePool::get();
        std::vector<StageTask> tasks(batch);
        std::atomic<uint32_t> done[8];
        size_t clo[9];
        for (size_t q = 0; q <= nchunk; q++) clo[q] = batch * q / nchunk;
        for (size_t q = 0; q < nchunk; q++) {
            done[q].store(0, std::memory_order_relaxed);
            for (size_t b = clo[q]; b < clo[q + 1]; b++) tasks[b] = StageTask{segs[b], sl.h_input + b * S, S * sizeof(float), &done[q]};
        }
        if (pool.workers() && batch > 1) pool.push(tasks.data(), batch);
        else
            for (size_t b = 0; b < batch; b++) {
                memcpy(tasks[b].dst, tasks[b].src, tasks[b].bytes);
                tasks[b].done->fetch_add(1, std::memory_order_release);
            }
        hipError_t e = hipSuccess;
        for (size_t q = 0; q < nchunk; q++) {
            const uint32_t want = (uint32_t)(clo[q + 1] - clo[q]);
            while (done[q].load(std::memory_order_acquire) < want)
                if (!pool.try_run_one()) std::this_thread::yield();
            if (e == hipSuccess && want)
                e = hipMemcpyAsync(sl.d_input + clo[q] * S, sl.h_input + clo[q] * S, (size_t)want * S * sizeof(float), hipMemcpyHostToDevice, c->copy_stream);
        }
        // (every task of this call has completed here: `tasks` and `done` may go out of scope)
        if (e != hipSuccess) return fail(BN_ERR_BACKEND, std::string("input upload failed: ") + hipGetErrorString(e));
    }
    sl.used = true;
    BN_HIP_TRY(hipEventRecord(sl.h2d_done, c->copy_stream));
    BN_HIP_TRY(hipStreamWaitEvent(c->stream, sl.h2d_done, 0));
    st = enqueue_plan(c, sl.d_input, batch, nullptr);
    if (st != BN_OK) {
        c->in_flight = true;
        return st;
    }
    BN_HIP_TRY(hipEventRecord(sl.plan_done, c->stream));
    c->last_batch = batch;
    const float *d_logits = resolve(c, lo.ref, sl.d_input);
    if (k) {
        st = enqueue_topk_rows(c->stream, d_logits, batch, N, k, has_min, min_conf, TopkRows::view(c->step.d, batch, k), c->d_tk_flags);
        if (st != BN_OK) return st;
    }
    {
        OutRegion regs[3] = {{sl.h_out, d_logits, batch * N * sizeof(float)}, {nullptr, nullptr, 0}, {nullptr, nullptr, 0}};
        int nreg = 1;
        if (cfg.embedding_output >= 0) {
            const OutputInfo &eo = p.outputs[cfg.embedding_output];
            regs[nreg++] = OutRegion{sl.h_out + N * c->max_batch, resolve(c, eo.ref, sl.d_input), batch * (size_t)eo.row_elems * sizeof(float)};
        }
        if (k) regs[nreg++] = OutRegion{sl.tk.h, c->step.d, TopkRows::bytes(batch, k)};
        st = results_to_host(c->stream, regs, nreg);
        if (st != BN_OK) {
            c->in_flight = true;
            return st;
        }
    }
    BN_HIP_TRY(hipEventRecord(sl.out_done, c->stream));
    sl.busy = true;
    sl.batch = batch;
    sl.k = k;
    sl.ticket = c->next_ticket++;
    *ticket = sl.ticket;
    return BN_OK;
}

bn_status bn_infer_collect(bn_ctx *c, uint64_t ticket, float *logits_out, float *emb_out, size_t k_stride, uint32_t *idx_out, float *conf_out,
                           uint32_t *count_out, const volatile int32_t *cancel, uint64_t timeout_ns) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (ticket == 0) return BN_OK;  // the empty batch
    bn_ctx::HostSlot *slp = nullptr;
    for (auto &q : c->slots)
        if (q.busy && q.ticket == ticket) slp = &q;
    if (!slp) return fail(BN_ERR_INVALID_ARG, "unknown or already collected ticket");
    bn_ctx::HostSlot &sl = *slp;
    // batches complete in submission order: collecting the younger one first simply waits for both
    BN_HIP_TRY(bn::use_device(c->model->device));
    const auto start = std::chrono::steady_clock::now();
    int spins = 0;
    while (true) {
        hipError_t q = hipEventQuery(sl.out_done);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) {
            sl.busy = false;
            c->in_flight = true;
            return fail(BN_ERR_BACKEND, std::string("hipEventQuery: ") + hipGetErrorString(q));
        }
        if (cancel && *cancel) {
            sl.busy = false;
            c->in_flight = true;
            return fail(BN_ERR_CANCELLED, "inference was cancelled");
        }
        if (timeout_ns) {
            const uint64_t el = (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - start).count();
            if (el >= timeout_ns) {
                sl.busy = false;
                c->in_flight = true;
                return fail(BN_ERR_TIMEOUT, "inference timed out after " + std::to_string(timeout_ns) + " ns");
            }
        }
        if (!cancel && !timeout_ns) {  // nothing to poll for: block
            hipError_t e = hipEventSynchronize(sl.out_done);
            if (e != hipSuccess) {
                sl.busy = false;
                c->in_flight = true;
                return fail(BN_ERR_BACKEND, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
            }
            break;
        }
        if (++spins > 200) std::this_thread::sleep_for(std::chrono::microseconds(50));
        else std::this_thread::yield();
    }
    const Plan &p = *c->pd->plan;
    const bn_model_config &cfg = c->model->cfg;
    const size_t N = (size_t)p.outputs[cfg.logits_output].row_elems;
    const size_t batch = sl.batch, k = sl.k;
    if (logits_out) memcpy(logits_out, sl.h_out, batch * N * sizeof(float));
    if (emb_out && cfg.embedding_output >= 0) {
        const size_t E = (size_t)p.outputs[cfg.embedding_output].row_elems;
        memcpy(emb_out, sl.h_out + N * c->max_batch, batch * E * sizeof(float));
    }
    if (count_out) {
        if (k == 0) {
            for (size_t r = 0; r < batch; r++) count_out[r] = 0;
        } else {
            if (!idx_out || !conf_out || k_stride < k) {
                sl.busy = false;
                return fail(BN_ERR_INVALID_ARG, "top-K outputs need idx / conf buffers with k_stride >= min(top_k, num_species)");
            }
            const TopkRows::ConstView v = TopkRows::view(static_cast<const uint32_t *>(sl.tk.h), batch, k);
            for (size_t r = 0; r < batch; r++) {
                count_out[r] = v.count[r];
                for (size_t j = 0; j < v.count[r]; j++) {
                    idx_out[r * k_stride + j] = v.idx[r * k + j];
                    conf_out[r * k_stride + j] = v.conf[r * k + j];
                }
            }
        }
    }
    sl.busy = false;
    return BN_OK;
}

bn_status bn_infer(bn_ctx *c, const float *const *segs, size_t batch, float *logits_out, float *emb_out, const volatile int32_t *cancel,
                   uint64_t timeout_ns) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (batch == 0) return BN_OK;
    if (!segs || !logits_out) return fail(BN_ERR_INVALID_ARG, "null argument");
    if (cancel && *cancel) return fail(BN_ERR_CANCELLED, "inference was cancelled");
    uint64_t ticket = 0;
    bn_status st = bn_infer_submit(c, segs, batch, 0, 0, 0.0f, &ticket);
    if (st != BN_OK) return st;
    return bn_infer_collect(c, ticket, logits_out, emb_out, 0, nullptr, nullptr, nullptr, cancel, timeout_ns);
}

bn_status bn_ctx_output_device(const bn_ctx *c, int32_t index, const float **d_ptr, size_t *row_elems) {
    if (!c || !d_ptr || !row_elems) return fail(BN_ERR_INVALID_ARG, "null argument");
    const Plan &p = *c->pd->plan;
    if (index < 0 || index >= (int)p.outputs.size()) return fail(BN_ERR_INVALID_ARG, "output index out of range");
    if (!p.outputs[index].computed) return fail(BN_ERR_INVALID_ARG, "output " + std::to_string(index) + " is not computed by this context (create it with BN_CTX_ALL_OUTPUTS)");
    *d_ptr = resolve(c, p.outputs[index].ref, c->d_input);
    *row_elems = (size_t)p.outputs[index].row_elems;
    return BN_OK;
}

bn_status bn_ctx_read_output(bn_ctx *c, int32_t index, size_t batch, float *host_out) {
    const float *d = nullptr;
    size_t row = 0;
    bn_status st = bn_ctx_output_device(c, index, &d, &row);
    if (st != BN_OK) return st;
    if (!host_out || batch > c->max_batch) return fail(BN_ERR_INVALID_ARG, "bad host buffer / batch");
    BN_HIP_TRY(bn::use_device(c->model->device));
    BN_HIP_TRY(hipStreamSynchronize(c->stream));
    c->in_flight = false;
    BN_HIP_TRY(gated::Memcpy(host_out, d, batch * row * sizeof(float), hipMemcpyDeviceToHost));
    return BN_OK;
}

size_t bn_ctx_time_kernels(bn_ctx *c, size_t batch, char (*names)[BN_NAME_LEN], float *usec, double *macs, double *bytes, size_t cap) {
    if (!c || batch == 0 || batch > c->max_batch) return 0;
    const Plan &p = *c->pd->plan;
    if (bn::use_device(c->model->device) != hipSuccess) return 0;
    (void)hipStreamSynchronize(c->stream);
    std::vector<bn::Event> ev(p.ops.size() + 1);
    for (auto &e : ev) (void)e.create();
    // warm (instruction caches, clocks) then measure
    for (auto &op : p.ops) launch_op(c, op, c->d_input, (int64_t)batch);
    (void)hipEventRecord(ev[0], c->stream);
    for (size_t k = 0; k < p.ops.size(); k++) {
        launch_op(c, p.ops[k], c->d_input, (int64_t)batch);
        (void)hipEventRecord(ev[k + 1], c->stream);
    }
    // calibration: the same event-to-event interval around an EMPTY kernel.  rocprofv3's kernel trace
    // reports 3.6 us for that empty kernel on MI355X (profiles/r01_v6_kernel_stats_1stream.csv,
    // null_kernel); the rest of its interval is command-processor and event overhead that every
    // interval above also contains, so it is subtracted -- the reported times are then on rocprofv3's
    // scale (family averages agree within a few percent).
    float overhead_us = 0.0f;
    {
        constexpr int NCAL = 16;
        bn::Event ce[NCAL + 1];
        for (auto &e : ce) (void)e.create();
        launch_null(c->stream);
        (void)hipEventRecord(ce[0], c->stream);
        for (int k = 0; k < NCAL; k++) {
            launch_null(c->stream);
            (void)hipEventRecord(ce[k + 1], c->stream);
        }
        (void)hipStreamSynchronize(c->stream);
        std::vector<float> iv;
        for (int k = 0; k < NCAL; k++) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, ce[k], ce[k + 1]);
            iv.push_back(ms * 1000.0f);
        }
        std::sort(iv.begin(), iv.end());
        overhead_us = std::max(0.0f, iv[NCAL / 2] - 3.6f);
    }
    (void)hipStreamSynchronize(c->stream);
    for (size_t k = 0; k < p.ops.size() && k < cap; k++) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
        if (usec) usec[k] = std::max(0.5f, ms * 1000.0f - overhead_us);
        if (names) snprintf(names[k], BN_NAME_LEN, "%s", p.ops[k].name.c_str());
        // every multiply-add the launch PERFORMS: a fused MBConv launch carries its expand conv on the matrix cores beside the
        // depthwise taps (macs_mfma_extra, halo / band recompute included), a GEMM with the squeeze-excite products in its
        // prologue carries those on the vector ALU -- so that the launches sum to the plan's macs_mfma + macs_valu
        if (macs) macs[k] = (p.ops[k].macs + p.ops[k].macs_mfma_extra + p.ops[k].macs_valu_extra) * (double)batch;
        if (bytes) bytes[k] = p.ops[k].bytes * (double)batch + p.ops[k].weight_bytes;
    }
    return p.ops.size();
}

size_t bn_ctx_launch_costs(const bn_ctx *c, size_t batch, double *macs_mfma, double *macs_valu, double *macs_recompute, double *bytes, size_t cap) {
    if (!c || batch == 0 || batch > c->max_batch) return 0;
    const Plan &p = *c->pd->plan;
    for (size_t k = 0; k < p.ops.size() && k < cap; k++) {
        const auto &op = p.ops[k];
        if (macs_mfma) macs_mfma[k] = ((op.mfma ? op.macs : 0.0) + op.macs_mfma_extra) * (double)batch;
        if (macs_valu) macs_valu[k] = ((op.mfma ? 0.0 : op.macs) + op.macs_valu_extra) * (double)batch;
        if (macs_recompute) macs_recompute[k] = op.macs_recompute * (double)batch;
        if (bytes) bytes[k] = op.bytes * (double)batch + op.weight_bytes;
    }
    return p.ops.size();
}

static bn_status topk_run(int device, hipStream_t stream, const float *d_logits, size_t rows, size_t n, size_t top_k, int32_t has_min,
                          float min_conf, size_t k_stride, uint32_t *d_idx, float *d_conf, uint32_t *d_cnt, uint32_t *d_flags,
                          uint32_t *idx_out, float *conf_out, uint32_t *count_out) {
    (void)device;
    size_t k = 0;  // (not 0 below: the callers answer an empty selection themselves)
    bn_status st = check_top_k(n, top_k, &k);
    if (st != BN_OK) return st;
    if (k_stride < k) return fail(BN_ERR_INVALID_ARG, "k_stride smaller than min(top_k, n)");
    if ((st = enqueue_topk_rows(stream, d_logits, rows, n, k, has_min, min_conf, TopkRows::View{d_idx, d_conf, d_cnt, k}, d_flags)) != BN_OK) return st;
    std::vector<uint32_t> h_idx(rows * k), h_cnt(rows);
    std::vector<float> h_conf(rows * k);
    BN_HIP_TRY(hipMemcpyAsync(h_cnt.data(), d_cnt, rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    BN_HIP_TRY(hipMemcpyAsync(h_idx.data(), d_idx, rows * k * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    BN_HIP_TRY(hipMemcpyAsync(h_conf.data(), d_conf, rows * k * sizeof(float), hipMemcpyDeviceToHost, stream));
    BN_HIP_TRY(hipStreamSynchronize(stream));
    for (size_t r = 0; r < rows; r++) {
        count_out[r] = h_cnt[r];
        for (size_t j = 0; j < h_cnt[r]; j++) {
            idx_out[r * k_stride + j] = h_idx[r * k + j];
            conf_out[r * k_stride + j] = h_conf[r * k + j];
        }
    }
    return BN_OK;
}

static bn_status ensure_topk_buffers(bn_ctx *c, size_t k);

bn_status bn_topk(bn_ctx *c, size_t batch, size_t top_k, int32_t has_min, float min_conf, size_t k_stride, uint32_t *idx_out, float *conf_out,
                  uint32_t *count_out) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (batch == 0) return BN_OK;
    if (!count_out || batch > c->max_batch) return fail(BN_ERR_INVALID_ARG, "bad arguments");
    const Plan &p = *c->pd->plan;
    const OutputInfo &lo = p.outputs[c->model->cfg.logits_output];
    const size_t n = (size_t)lo.row_elems;
    const size_t k = std::min(top_k, n);
    if (k == 0) {
        for (size_t r = 0; r < batch; r++) count_out[r] = 0;
        return BN_OK;
    }
    if (!idx_out || !conf_out) return fail(BN_ERR_INVALID_ARG, "null output");
    BN_HIP_TRY(bn::use_device(c->model->device));
    {
        bn_status est = ensure_topk_buffers(c, k);
        if (est != BN_OK) return est;
    }
    return topk_run(c->model->device, c->stream, resolve(c, lo.ref, c->d_input), batch, n, top_k, has_min, min_conf, k_stride, c->d_tk_idx,
                    c->d_tk_conf, c->d_tk_cnt, c->d_tk_flags, idx_out, conf_out, count_out);
}

static bn_status ensure_topk_buffers(bn_ctx *c, size_t k) {
    const size_t need = c->max_batch * k;
    if (need > c->tk_cap) {
        c->d_tk_idx.reset();  // both go before either comes back, as ever
        c->d_tk_conf.reset();
        BN_HIP_TRY(c->d_tk_idx.alloc(need * sizeof(uint32_t)));
        BN_HIP_TRY(c->d_tk_conf.alloc(need * sizeof(float)));
        c->tk_cap = need;
    }
    if (!c->d_tk_cnt) BN_HIP_TRY(c->d_tk_cnt.alloc(c->max_batch * sizeof(uint32_t)));
    if (!c->d_tk_flags) BN_HIP_TRY(c->d_tk_flags.alloc(c->max_batch * sizeof(uint32_t)));
    return BN_OK;
}

// device + pinned blocks of the packed top-K rows of one step (grown on demand; nothing of this context may be in
// flight when they grow: the stream is drained first)
static bn_status ensure_step_block(bn_ctx *c, size_t k) {
    bn_status st = ensure_topk_buffers(c, k);
    if (st != BN_OK) return st;
    return c->step.reserve(c->max_batch, k, c->stream, true, true);
}

}  // extern "C"

bn_status bn::step_device(bn_ctx *c, const float *d_pcm, const StepRows &rows, size_t top_k, int32_t has_min, float min_conf, int32_t sync) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    const size_t batch = rows.batch;
    if (batch == 0) return BN_OK;
    if (!d_pcm || batch > c->max_batch) return fail(BN_ERR_INVALID_ARG, "bad input / batch size exceeds context max");
    if (reinterpret_cast<uintptr_t>(d_pcm) & 15u) return fail(BN_ERR_INVALID_ARG, "device input must be 16-byte aligned");
    const Plan &p = *c->pd->plan;
    const OutputInfo &lo = p.outputs[c->model->cfg.logits_output];
    const size_t n = (size_t)lo.row_elems;
    size_t k = 0;
    bn_status st = check_top_k(n, top_k, &k);
    if (st != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(c->model->device));
    st = drain_if_needed(c);
    if (st != BN_OK) return st;
    st = ensure_step_block(c, k);
    if (st != BN_OK) return st;
    st = enqueue_plan(c, d_pcm, batch, nullptr);
    if (st != BN_OK) return st;
    c->last_batch = batch;
    const float *d_logits = resolve(c, lo.ref, d_pcm);
    st = enqueue_topk_rows(c->stream, d_logits, batch, n, k, has_min, min_conf, TopkRows::view(c->step.d, batch, k), c->d_tk_flags);
    if (st != BN_OK) return st;
    {
        const OutRegion regs[2] = {{c->h_out, d_logits, batch * n * sizeof(float)}, {c->step.h, c->step.d, TopkRows::bytes(batch, k)}};
        st = results_to_host(c->stream, regs, 2);
        if (st != BN_OK) return st;
    }
    c->step.mark(batch, k);
    if (c->head) {
        const OutputInfo &eo = p.outputs[c->model->cfg.embedding_output];
        st = bn::head_step(c->head, c->stream, resolve(c, eo.ref, d_pcm), batch);
        if (st != BN_OK) return st;
    }
    if (c->prior) {
        st = bn::prior_step(c->prior, c->stream, d_logits, TopkRows::view(static_cast<const uint32_t *>(c->step.d), batch, k), rows);
        if (st != BN_OK) return st;
    }
    if (c->track && rows.numbered) {
        st = bn::track_step(c->track, c->stream, d_logits, rows, c->prior);
        if (st != BN_OK) return st;
    }
    if (c->match) {
        const OutputInfo &eo = p.outputs[c->model->cfg.embedding_output];
        st = bn::match_step(c->match, c->stream, resolve(c, eo.ref, d_pcm), batch);
        if (st != BN_OK) return st;
    }
    if (sync) BN_HIP_TRY(hipStreamSynchronize(c->stream));
    return BN_OK;
}

extern "C" {

bn_status bn_step_device(bn_ctx *c, const float *d_pcm, size_t batch, size_t top_k, int32_t has_min, float min_conf, int32_t sync) {
    return bn::step_device(c, d_pcm, bn::StepRows{batch, false, nullptr, nullptr, 0}, top_k, has_min, min_conf, sync);
}

bn_status bn_ctx_attach_head(bn_ctx *c, bn_head *h, size_t top_k, int32_t has_min, float min_conf) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    const bn_model_config &cfg = c->model->cfg;
    BN_HIP_TRY(bn::use_device(c->model->device));
    bn::HeadAttach *a = nullptr;
    if (h) {
        const bool has_emb = cfg.has_embedding && cfg.embedding_output >= 0 && c->pd->plan->outputs[cfg.embedding_output].computed;
        bn_status st = bn::head_attach(h, c->model->device, has_emb, has_emb ? (size_t)c->pd->plan->outputs[cfg.embedding_output].row_elems : 0,
                                       c->max_batch, top_k, has_min, min_conf, &a);
        if (st != BN_OK) return st;
    }
    return install_attachment(c->stream, c->head, a, bn::head_detach);
}

bn_status bn_step_head_results(const bn_ctx *c, const float **logits, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride,
                               size_t *n_classes) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (!c->head) return fail(BN_ERR_INVALID_ARG, "no head is attached to this context");
    return bn::head_step_results(c->head, logits, idx, conf, count, k_stride, n_classes);
}

bn_status bn_ctx_attach_index(bn_ctx *c, bn_index *x, size_t top_m, int32_t has_min, float min_score) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    const bn_model_config &cfg = c->model->cfg;
    BN_HIP_TRY(bn::use_device(c->model->device));
    bn::MatchAttach *a = nullptr;
    if (x) {
        const bool has_emb = cfg.has_embedding && cfg.embedding_output >= 0 && c->pd->plan->outputs[cfg.embedding_output].computed;
        bn_status st = bn::match_attach(x, c->model->device, has_emb, has_emb ? (size_t)c->pd->plan->outputs[cfg.embedding_output].row_elems : 0,
                                        c->max_batch, top_m, has_min, min_score, &a);
        if (st != BN_OK) return st;
    }
    return install_attachment(c->stream, c->match, a, bn::match_detach);
}

bn_status bn_step_index_results(const bn_ctx *c, const uint64_t **id, const float **score, const uint32_t **tag, const uint32_t **count, size_t *m_stride,
                                size_t *rows_searched) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (!c->match) return fail(BN_ERR_INVALID_ARG, "no index is attached to this context");
    return bn::match_step_results(c->match, id, score, tag, count, m_stride, rows_searched);
}

bn_status bn_ctx_attach_prior(bn_ctx *c, bn_prior *p, const int32_t *source_sites, size_t n_source_sites, size_t top_k, int32_t has_min, float min_conf) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    BN_HIP_TRY(bn::use_device(c->model->device));
    bn::PriorAttach *a = nullptr;
    if (p) {
        const size_t n = (size_t)c->pd->plan->outputs[c->model->cfg.logits_output].row_elems;
        bn_status st = bn::prior_attach(p, c->model->device, n, c->max_batch, source_sites, n_source_sites, top_k, has_min, min_conf, &a);
        if (st != BN_OK) return st;
    }
    return install_attachment(c->stream, c->prior, a, bn::prior_detach);
}

bn_status bn_ctx_prior_site(bn_ctx *c, int32_t site) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (!c->prior) return fail(BN_ERR_INVALID_ARG, "no prior is attached to this context");
    return bn::prior_set_site(c->prior, site);
}

bn_status bn_step_prior_results(const bn_ctx *c, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (!c->prior) return fail(BN_ERR_INVALID_ARG, "no prior is attached to this context");
    return bn::prior_step_results(c->prior, idx, conf, count, k_stride);
}

bn_status bn_ctx_attach_track(bn_ctx *c, bn_track *t) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    BN_HIP_TRY(bn::use_device(c->model->device));
    bn::TrackAttach *a = nullptr;
    if (t) {
        const size_t n = (size_t)c->pd->plan->outputs[c->model->cfg.logits_output].row_elems;
        bn_status st = bn::track_attach(t, c->model->device, n, c->max_batch, &a);
        if (st != BN_OK) return st;
    }
    return install_attachment(c->stream, c->track, a, bn::track_detach);
}

bn_status bn_ctx_track_source(bn_ctx *c, int32_t source) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (!c->track) return fail(BN_ERR_INVALID_ARG, "no tracker is attached to this context");
    return bn::track_set_source(c->track, source);
}

bn_status bn_step_track_results(bn_ctx *c, const bn_event **events, size_t *n, size_t *dropped, size_t *stale_rows) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    if (!c->track) return fail(BN_ERR_INVALID_ARG, "no tracker is attached to this context");
    return bn::track_step_results(c->track, events, n, dropped, stale_rows);
}

bn_status bn_step_results(const bn_ctx *c, const float **logits, const uint32_t **idx, const float **conf, const uint32_t **count, size_t *k_stride) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "no step has run on this context");
    bn_status st = c->step.results("no step has run on this context", idx, conf, count, k_stride);
    if (st == BN_OK && logits) *logits = c->h_out;
    return st;
}

bn_status bn_ctx_step_device_rows(const bn_ctx *c, const uint32_t **d_rows) {
    if (!c || !d_rows) return fail(BN_ERR_INVALID_ARG, "null argument");
    if (!c->step.d) return fail(BN_ERR_INVALID_ARG, "no step has run on this context");
    *d_rows = c->step.d;
    return BN_OK;
}

bn_status bn_topk_device(int32_t device, const float *d_logits, size_t rows, size_t n, size_t top_k, int32_t has_min, float min_conf,
                         size_t k_stride, uint32_t *idx_out, float *conf_out, uint32_t *count_out) {
    if (rows == 0) return BN_OK;
    if (!count_out) return fail(BN_ERR_INVALID_ARG, "null output");
    const size_t k = std::min(top_k, n);
    if (k == 0) {
        for (size_t r = 0; r < rows; r++) count_out[r] = 0;
        return BN_OK;
    }
    if (!d_logits || !idx_out || !conf_out) return fail(BN_ERR_INVALID_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(BN_ERR_NO_DEVICE, "no HIP device is visible; this path has no CPU fallback");
    BN_HIP_TRY(bn::use_device(device));
    if (!prepare_device(device)) return fail(BN_ERR_BACKEND, "device refused the kernels' dynamic-LDS opt-in");
    DeviceBuf<uint32_t> d_idx, d_cnt, d_flags;
    DeviceBuf<float> d_conf;
    BN_HIP_TRY(d_idx.alloc(rows * k * sizeof(uint32_t)));
    BN_HIP_TRY(d_conf.alloc(rows * k * sizeof(float)));
    BN_HIP_TRY(d_cnt.alloc(rows * sizeof(uint32_t)));
    BN_HIP_TRY(d_flags.alloc(rows * sizeof(uint32_t)));
    return topk_run(device, nullptr, d_logits, rows, n, top_k, has_min, min_conf, k_stride, d_idx, d_conf, d_cnt, d_flags, idx_out, conf_out, count_out);
}

bn_status bn_topk_host(int32_t device, const float *logits, size_t rows, size_t n, size_t top_k, int32_t has_min, float min_conf,
                       size_t k_stride, uint32_t *idx_out, float *conf_out, uint32_t *count_out) {
    if (rows == 0) return BN_OK;
    if (!count_out) return fail(BN_ERR_INVALID_ARG, "null output");
    if (n == 0 || top_k == 0) {
        for (size_t r = 0; r < rows; r++) count_out[r] = 0;
        return BN_OK;
    }
    if (!logits) return fail(BN_ERR_INVALID_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(BN_ERR_NO_DEVICE, "no HIP device is visible; this path has no CPU fallback");
    BN_HIP_TRY(bn::use_device(device));
    DeviceBuf<float> d;
    BN_HIP_TRY(d.alloc(rows * n * sizeof(float)));
    hipError_t e = gated::Memcpy(d, logits, rows * n * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(BN_ERR_BACKEND, std::string("hipMemcpy: ") + hipGetErrorString(e));
    return bn_topk_device(device, d, rows, n, top_k, has_min, min_conf, k_stride, idx_out, conf_out, count_out);
}

// what bn_infer_windows and bn_step_windows both refuse of a checked, non-empty range of a recording (recording.cpp)
static bn_status check_window_batch(const bn_ctx *c, size_t count, int32_t rec_device) {
    if (count > c->max_batch) return fail(BN_ERR_INVALID_ARG, "batch size " + std::to_string(count) + " exceeds context max " + std::to_string(c->max_batch));
    if (rec_device != c->model->device) return fail(BN_ERR_INVALID_ARG, "recording and context live on different devices");
    return BN_OK;
}

bn_status bn_infer_windows(bn_ctx *c, const bn_recording *r, size_t step_samples, size_t first_window, size_t count, float *logits_out, float *emb_out,
                           const volatile int32_t *cancel, uint64_t timeout_ns) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    const size_t S = (size_t)c->pd->plan->sample_count;
    int32_t rec_device = 0;
    bn_status st = check_windows(r, S, step_samples, first_window, count, &rec_device);
    if (st != BN_OK) return st;
    if (count == 0) return BN_OK;
    if (!logits_out) return fail(BN_ERR_INVALID_ARG, "null argument");
    if ((st = check_window_batch(c, count, rec_device)) != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(c->model->device));
    st = drain_if_needed(c);
    if (st != BN_OK) return st;
    if (cancel && *cancel) return fail(BN_ERR_CANCELLED, "inference was cancelled");
    if ((st = enqueue_windows(c->stream, c->model->device, c->d_input, r, S, step_samples, first_window, count)) != BN_OK) return st;
    st = enqueue_plan(c, c->d_input, count, cancel);
    if (st != BN_OK) {
        c->in_flight = true;
        return st;
    }
    return finish_infer(c, count, logits_out, emb_out, cancel, timeout_ns);
}

bn_status bn_step_windows(bn_ctx *c, const bn_recording *r, size_t step_samples, size_t first_window, size_t count, size_t top_k, int32_t has_min,
                          float min_conf, int32_t sync) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    const size_t S = (size_t)c->pd->plan->sample_count;
    int32_t rec_device = 0;
    bn_status st = check_windows(r, S, step_samples, first_window, count, &rec_device);
    if (st != BN_OK) return st;
    if (count == 0) return BN_OK;
    if ((st = check_window_batch(c, count, rec_device)) != BN_OK) return st;
    if ((st = bn::ctx_step_check(c, 0, first_window, count)) != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(c->model->device));
    // stream order keeps this behind whatever the context still has in flight
    if ((st = enqueue_windows(c->stream, c->model->device, c->d_input, r, S, step_samples, first_window, count)) != BN_OK) return st;
    // row i is window first_window + i of the tracker attachment's source
    return bn::step_device(c, c->d_input, bn::StepRows{count, true, nullptr, nullptr, first_window}, top_k, has_min, min_conf, sync);
}

size_t bn_model_survey(const char *onnx_path, char *buf, size_t cap, bn_status *status) {
    bn_status dummy;
    if (!status) status = &dummy;
    *status = BN_OK;
    std::string text;
    char line[1024];
    try {
        if (!onnx_path) throw std::runtime_error("null path");
        OnnxModel om = parse_onnx_file(onnx_path);
        IoMeta io = read_io_meta(om);
        auto shape_str = [](const std::vector<int64_t> &s) {
            std::string r = "[";
            for (size_t k = 0; k < s.size(); k++) r += (k ? ", " : "") + (s[k] < 0 ? std::string("?") : std::to_string(s[k]));
            return r + "]";
        };
        snprintf(line, sizeof(line), "opset %lld, %zu nodes, %zu initializers\n", (long long)om.opset, om.nodes.size(), om.initializers.size());
        text += line;
        text += "input  " + io.input_name + " " + shape_str(io.input_shape) + "\n";
        for (size_t k = 0; k < io.output_names.size(); k++) text += "output " + std::to_string(k) + " " + io.output_names[k] + " " + shape_str(io.output_shapes[k]) + "\n";
        bn_model_config cfg{};
        std::string reason;
        const bool detected = detect_model_type(io.input_shape, io.output_shapes, -1, cfg, reason);
        if (detected) {
            snprintf(line, sizeof(line), "detected model_type=%d sample_rate=%u sample_count=%llu num_species=%llu embedding_dim=%llu logits_output=%d embedding_output=%d\n",
                     cfg.model_type, cfg.sample_rate, (unsigned long long)cfg.sample_count, (unsigned long long)cfg.num_species,
                     (unsigned long long)cfg.embedding_dim, cfg.logits_output, cfg.embedding_output);
            text += line;
        } else text += "detection FAILED: " + reason + "\n";
        // operator types: count, and whether the lowering has a rule for the type at all
        std::map<std::string, std::pair<int, std::string>> hist;
        for (const auto &nd : om.nodes) {
            auto &h = hist[nd.op_type];
            if (h.first++ == 0) h.second = nd.name.empty() ? (nd.outputs.empty() ? std::string("?") : nd.outputs[0]) : nd.name;
        }
        int unmapped_types = 0, unmapped_nodes = 0;
        for (const auto &kv : hist) {
            const bool ok = op_type_mapped(kv.first);
            if (!ok) { unmapped_types++; unmapped_nodes += kv.second.first; }
            snprintf(line, sizeof(line), "op %-24s x%-5d %s%s\n", kv.first.c_str(), kv.second.first, ok ? "mapped" : "NOT MAPPED   first: ", ok ? "" : kv.second.second.c_str());
            text += line;
        }
        snprintf(line, sizeof(line), "unmapped: %d operator types, %d nodes\n", unmapped_types, unmapped_nodes);
        text += line;
        // the plan itself (every graph output, so that no refusal hides in a branch the audio path does not read; then the audio path)
        for (int all = 1; all >= 0; all--) {
            std::vector<int> wanted;
            if (all) for (size_t k = 0; k < om.outputs.size(); k++) wanted.push_back((int)k);
            else if (detected) { wanted.push_back(cfg.logits_output); if (cfg.embedding_output >= 0) wanted.push_back(cfg.embedding_output); }
            else continue;
            try {
                auto p = build_plan(om, wanted);
                snprintf(line, sizeof(line), "plan (%s): OK, %zu launches, %.4g MMAC/segment on the matrix cores, %.4g on the vector ALU, arena %.3g MB/segment, weights %.3g MB\n",
                         all ? "every graph output" : "logits + embeddings", p->ops.size(), p->macs_mfma / 1e6, p->macs_valu / 1e6, p->arena_elems * 4.0 / 1e6, p->weight_bytes / 1e6);
                text += line;
            } catch (const std::exception &e) {
                if (*status == BN_OK || !all) *status = BN_ERR_UNSUPPORTED_MODEL;
                text += std::string("plan (") + (all ? "every graph output" : "logits + embeddings") + "): REFUSED: " + e.what() + "\n";
                if (!all) (void)fail(BN_ERR_UNSUPPORTED_MODEL, e.what());
            }
        }
    } catch (const std::exception &e) {
        *status = fail(BN_ERR_MODEL_LOAD, e.what());
        return 0;
    }
    if (buf && cap) {
        const size_t n = std::min(cap - 1, text.size());
        memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return text.size();
}

size_t bn_plan_describe(const char *onnx_path, int32_t model_type_override, int32_t all_outputs, char *buf, size_t cap, bn_status *status) {
    bn_status dummy;
    if (!status) status = &dummy;
    *status = BN_OK;
    std::string text;
    try {
        if (!onnx_path) throw std::runtime_error("null path");
        OnnxModel om = parse_onnx_file(onnx_path);
        IoMeta io = read_io_meta(om);
        std::vector<int> wanted;
        bn_model_config cfg{};
        std::string reason;
        if (all_outputs) {
            for (size_t k = 0; k < om.outputs.size(); k++) wanted.push_back((int)k);
        } else {
            if (!detect_model_type(io.input_shape, io.output_shapes, model_type_override, cfg, reason)) {
                *status = fail(BN_ERR_MODEL_DETECTION, reason);
                return 0;
            }
            wanted.push_back(cfg.logits_output);
            if (cfg.embedding_output >= 0) wanted.push_back(cfg.embedding_output);
        }
        auto p = build_plan(om, wanted);
        static const char *kinds[] = {"ELT", "REDUCE", "GEMM", "CONV", "DWCONV", "GAP", "SEFC", "MBCONV", "POOL", "FFT"};
        char line[512];
        for (size_t k = 0; k < p->ops.size(); k++) {
            const PlanOp &op = p->ops[k];
            std::string extra;
            if (op.kind == OpKind::GEMM) {
                snprintf(line, sizeof(line), " rows=%lld K=%d N=%d lda=%lld act=%d bias=%d res=%d gate=%d", (long long)op.gemm.rows, op.gemm.K, op.gemm.N, (long long)op.gemm.lda, op.gemm.act, op.gemm.has_bias, op.gemm.has_res, op.gemm.has_scale);
                extra = line;
                if (op.gemm.fold) { snprintf(line, sizeof(line), " fold=%d/%d", op.gemm.fold, op.gemm.fold_n); extra += line; }
                if (op.pre.n) { snprintf(line, sizeof(line), " pre=%d", op.pre.n); extra += line; }
                if (op.gemm.gap) extra += " gap=1";
                if (op.gemm.se_inline) { snprintf(line, sizeof(line), " se_inline=%d/%d", op.se.C, op.se.Cr); extra += line; }
                // which of the three matrix kernels the launcher picks (the LDS-resident framing kernel may still fall back to
                // the generic one at launch: BN_FRAMELDS=0 or a span that does not fit)
                extra += op.gemm.fold == 2 ? (op.gemm.fold_wpk == 2 ? " kernel=frame_fold2q" : op.gemm.fold_wpk ? " kernel=frame_fold2p" : " kernel=frame_fold2") : op.gemm.fold ? " kernel=frame_fold" : op.gemm.w3 == 2 ? " kernel=b3" : op.gemm.w3 ? " kernel=dma3" : gemm_dma_shape(op.gemm) ? " kernel=dma" : (!(op.gemm.npost || op.gemm.out_strided) && gemm_use_splitk(op.gemm) ? " kernel=splitk" : " kernel=tiled");
                if (op.gemm.npost || op.gemm.out_strided) {
                    snprintf(line, sizeof(line), " post=%d out_rs=%lld out_cs=%lld", op.gemm.npost, (long long)op.gemm.out_rs, (long long)op.gemm.out_cs);
                    extra += line;
                }
            } else if (op.kind == OpKind::DWCONV) {
                snprintf(line, sizeof(line), " %dx%dx%d->%dx%d k=%dx%d s=%d act=%d tiled=%d squeeze=%d nblk=%d se=%d", op.dw.H, op.dw.W, op.dw.C, op.dw.OH, op.dw.OW, op.dw.kh, op.dw.kw, op.dw.sh, op.dw.act, op.dw.tiled, op.dw.has_gap, op.dw.nblk, op.se_fused);
                extra = line;
            } else if (op.kind == OpKind::CONV) {
                snprintf(line, sizeof(line), " %dx%dx%d->%dx%dx%d k=%dx%d s=%d g=%d act=%d", op.conv.H, op.conv.W, op.conv.Cin, op.conv.OH, op.conv.OW, op.conv.Cout, op.conv.kh, op.conv.kw, op.conv.sh, op.conv.groups, op.conv.act);
                extra = line;
            } else if (op.kind == OpKind::ELT) {
                int w = snprintf(line, sizeof(line), " n=%lld nd=%d stages=%d bin0=%d act0=%d size/so/sa=", (long long)op.elt.per_sample, op.elt.nd, op.elt.nstages, op.elt.st[0].bin, op.elt.st[0].act);
                for (int q = 0; q < op.elt.nd && w < (int)sizeof(line) - 40; q++)
                    w += snprintf(line + w, sizeof(line) - w, "%s%lld/%lld/%lld", q ? "," : "", (long long)op.elt.size[q], (long long)op.elt.so[q], (long long)op.elt.sa[q]);
                extra = line;
            } else if (op.kind == OpKind::MBCONV) {
                snprintf(line, sizeof(line), " %dx%dx%d->(%d)->%dx%dx%d k=%d s=%d tiles=%dx%d squeeze=%d se=%d%s rows=%d%s", op.mb.H, op.mb.W, op.mb.Cin, op.mb.C, op.mb.OH, op.mb.OW, op.mb.C, op.mb.k, op.mb.s, op.mb.tiles_y, op.mb.tiles_x, op.mb.has_gap, op.se_fused,
                         op.mb.row_mode && op.mb.row_b3 ? " row_b3" : "",  // (the row kernel's expand on the bf16 matrix pipe; in front of rows=, which readers parse to the end of the line)
                         op.mb.row_mode ? op.mb.toh : 0, op.mb.row_mode && op.mb.row_tr ? "(columns)" : "");
                extra = line;
                if (op.mb.whole_map == 2) {  // mbmap.hip: configuration, bands, transposition, padded k
                    snprintf(line, sizeof(line), " map=cfg%d%s%s%s kpad=%d", mbmap_config(op.mb), op.mb.map_bands > 1 ? ",bands" : "", op.mb.map_tr ? ",transposed" : "", op.mb.map_ws ? ",ws" : op.mb.map_b3 ? ",b3" : "", op.mb.cin_pad);
                    extra += line;
                }
            } else if (op.kind == OpKind::POOL) {
                snprintf(line, sizeof(line), " %dx%dx%d->%dx%d k=%dx%d s=%dx%d max=%d", op.pool.H, op.pool.W, op.pool.C, op.pool.OH, op.pool.OW, op.pool.kh, op.pool.kw,
                         op.pool.sh, op.pool.sw, op.pool.is_max);
                extra = line;
            } else if (op.kind == OpKind::GAP) {
                snprintf(line, sizeof(line), " HW=%lld C=%d splits=%d", (long long)op.gap.HW, op.gap.C, op.gap.splits);
                extra = line;
            } else if (op.kind == OpKind::SEFC) {
                snprintf(line, sizeof(line), " C=%d Cr=%d act1=%d act2=%d", op.se.C, op.se.Cr, op.se.act1, op.se.act2);
                extra = line;
            } else if (op.kind == OpKind::FFT) {
                snprintf(line, sizeof(line), " frames=%d L=%d hop=%d bins=%d power=%d tpb=%d mel=%d%s pre=%d post=%d out_rs=%lld out_cs=%lld fft_flops=%.3g", op.fft.frames, op.fft.L,
                         op.fft.hop, op.fft.nout, op.fft.power, op.fft.tpb, op.fft.nmel, op.fft.nmel ? (op.fft.mel_mode == 1 ? "(mfma)" : "(csr)") : "", op.fft.npre, op.fft.npost, (long long)op.fft.out_rs, (long long)op.fft.out_cs, op.flops_fft);
                extra = line;
            } else {
                snprintf(line, sizeof(line), " kept=%lld red=%lld op=%d inner_kept=%d", (long long)op.red.kept, (long long)op.red.red, op.red.op, op.red.inner_kept);
                extra = line;
            }
            snprintf(line, sizeof(line), "%3zu %-6s %-40s macs=%.3g bytes=%.3g", k, kinds[(int)op.kind], op.name.c_str(), op.macs, op.bytes);
            text += line + extra + "\n";
        }
        snprintf(line, sizeof(line), "TOTAL launches=%zu macs_mfma=%.6g macs_valu=%.6g act_bytes=%.6g weight_bytes=%.6g arena_bytes_per_sample=%lld consts_bytes=%lld dft_gemm_macs=%.6g fft_flops=%.6g\n",
                 p->ops.size(), p->macs_mfma, p->macs_valu, p->act_bytes, p->weight_bytes, (long long)p->arena_elems * 4, (long long)p->consts_elems * 4, p->dft_gemm_macs, p->fft_flops);
        text += line;
        for (size_t k = 0; k < p->outputs.size(); k++) {
            snprintf(line, sizeof(line), "OUTPUT %zu %s computed=%d row_elems=%lld\n", k, p->outputs[k].name.c_str(), (int)p->outputs[k].computed, (long long)p->outputs[k].row_elems);
            text += line;
        }
    } catch (const UnsupportedModel &e) {
        *status = fail(BN_ERR_UNSUPPORTED_MODEL, e.what());
        return 0;
    } catch (const std::exception &e) {
        *status = fail(BN_ERR_MODEL_LOAD, e.what());
        return 0;
    }
    if (buf && cap) snprintf(buf, cap, "%s", text.c_str());
    return text.size();
}

size_t bn_last_error(char *buf, size_t cap) {
    if (buf && cap) snprintf(buf, cap, "%s", g_err.c_str());
    return g_err.size();
}

}  // extern "C"

bn_status bn::set_last_error(bn_status st, const std::string &msg) { return fail(st, msg); }

bn_status bn::ctx_step_check(const bn_ctx *c, size_t n_sources, uint64_t first_window, size_t count) {
    bn_status st = c->prior ? bn::prior_step_check(c->prior, n_sources) : BN_OK;
    if (st == BN_OK && c->track) st = bn::track_step_check(c->track, c->prior, n_sources, first_window, count);
    return st;
}

bn_status bn::ctx_embedding(const bn_ctx *c, CtxEmbedding *out) {
    if (!c || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    const bn_model_config &cfg = c->model->cfg;
    if (!cfg.has_embedding || cfg.embedding_output < 0) return fail(BN_ERR_INVALID_ARG, "the context's model has no embedding output");
    bn_status st = bn_ctx_output_device(c, cfg.embedding_output, &out->d_rows, &out->row_elems);
    if (st != BN_OK) return st;
    out->device = c->model->device;
    out->stream = c->stream;
    out->last_batch = c->last_batch;
    return BN_OK;
}

bn_status bn::ctx_step_input(const bn_ctx *c, size_t top_k, CtxStepInput *out) {
    if (!c || !out) return fail(BN_ERR_INVALID_ARG, "null argument");
    const Plan &p = *c->pd->plan;
    const size_t n = (size_t)p.outputs[c->model->cfg.logits_output].row_elems;
    size_t k = 0;
    bn_status st = check_top_k(n, top_k, &k);
    if (st != BN_OK) return st;
    out->device = c->model->device;
    out->stream = c->stream;
    out->d_input = c->d_input;
    out->sample_count = (size_t)p.sample_count;
    out->max_batch = c->max_batch;
    out->tracked = c->track != nullptr;
    return BN_OK;
}
