// Recordings of the C ABI (include/birdnet_hip.h): bn_recording_*, the resampler's table, and the explicit window lists
// (bn_recording_window_list, bn_step_window_list: of a context they need what bn_step_live does).  bn_recording is private to this
// file; capi.cpp's bn_infer_windows and bn_step_windows reach a recording through check_windows and enqueue_windows (capi_internal.h).
// Every launch is clear_launch_state, the launcher, check_launch; results reach the host through launch_and_read or rows_in_pieces.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "band_levels.h"
#include "capi_internal.h"
#include "kernels.h"
#include "levels.h"
#include "window_list_plan.h"

using namespace bn;

// ---- recording-level ingest (birdnet-analyze.rs:683-687, 707-743) ----
// The device bytes of a recording, in the format they were uploaded in, and their upload: shared by the recording that uploaded
// them and its channel views (bn_recording_view_channel), freed -- the upload joined -- with the last of them.
struct RecStore {
    int32_t device = 0;
    DeviceBuf<void> d_pcm;
    size_t n_frames = 0;
    // asynchronous upload (bn_recording_create_async): a thread of the store's own copies the caller's buffer chunk by chunk
    // (synchronous copies under the capture gate, like every other copy of the library); chunks_done chunks are on the device.
    // A chunk is a whole number of FRAMES (pcm_layout.h), so "has frame i arrived" is i / chunk_frames
    size_t chunk_frames = 0;  // 0: the whole recording was uploaded at creation
    size_t n_chunks = 0;
    std::atomic<size_t> chunks_done{0};
    std::atomic<int> upload_error{0};
    std::thread uploader;
    std::mutex mu;
    std::condition_variable cv;
    RecStore(int32_t dev, size_t n) : device(dev), n_frames(n) {}
    ~RecStore() {
        if (uploader.joinable()) uploader.join();  // (the caller's buffer is read until here at the latest)
        (void)bn::use_device(device);
    }
};
struct bn_recording {
    int32_t device = 0;
    PcmLayout layout;        // how the store's bytes are read: frame -> f32 sample (pcm_read.h)
    bool any_format = false;  // created with a layout: bn_recording_read_f32 converts whatever the format
    bool resampled = false;   // the store holds the resampler's mono f32 output: no storage-format bytes are left
    std::shared_ptr<RecStore> store;
    size_t n_samples = 0;  // frames
    PcmSrc src() const { return PcmSrc{store->d_pcm.get(), layout}; }
};

namespace {
bn_status fail(bn_status st, const std::string &msg) { return set_last_error(st, msg); }

// blocks until frame `last` of the recording is on the device (kernels launched afterwards may read it); false if the upload failed
bool recording_wait_samples(const bn_recording *rc, size_t last) {
    RecStore *r = rc->store.get();
    if (!r->chunk_frames || r->n_chunks == 0) return true;
    const size_t need = pcm_chunks_for_frame(last, r->chunk_frames, r->n_chunks);
    if (r->chunks_done.load(std::memory_order_acquire) >= need) return r->upload_error.load() == 0;
    std::unique_lock<std::mutex> lk(r->mu);
    r->cv.wait(lk, [&] { return r->chunks_done.load(std::memory_order_acquire) >= need || r->upload_error.load() != 0; });
    return r->upload_error.load() == 0;
}

// One launch on the null stream, checked as `what`, then `bytes` of what it wrote at `dev` copied to `host`; `failed` words a copy
// that fails (a fault of the kernel shows there)
template <class Launch>
bn_status launch_and_read(const char *what, const char *failed, void *host, const void *dev, size_t bytes, Launch &&launch) {
    bn::clear_launch_state();
    launch();
    if (bn_status st = bn::check_launch(what); st != BN_OK) return st;
    const hipError_t e = gated::Memcpy(host, dev, bytes, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(BN_ERR_BACKEND, std::string(failed) + hipGetErrorString(e));
    return BN_OK;
}

// `count` rows of Row into the caller's `out` (rows struct_size >= sizeof(Row) apart; the bytes behind a Row are left alone), at
// most `piece` per launch: launch(done, n, d) writes rows [done, done + n) to the device block d
template <class Row, class Launch>
bn_status rows_in_pieces(const char *what, const char *failed, size_t count, size_t piece, void *out, size_t struct_size, Launch &&launch) {
    DeviceBuf<Row> d;
    BN_HIP_TRY(d.alloc(std::min(piece, count) * sizeof(Row)));
    std::vector<Row> rows;  // only for a caller whose struct is longer than this header's
    if (struct_size != sizeof(Row)) rows.resize(std::min(piece, count));
    for (size_t done = 0; done < count; done += piece) {
        const size_t n = std::min(piece, count - done);
        char *at = static_cast<char *>(out) + done * struct_size;
        void *host = rows.empty() ? static_cast<void *>(at) : static_cast<void *>(rows.data());
        if (bn_status st = launch_and_read(what, failed, host, d, n * sizeof(Row), [&] { launch(done, n, d.get()); }); st != BN_OK) return st;
        for (size_t i = 0; i < rows.size() && i < n; i++) memcpy(at + i * struct_size, &rows[i], sizeof(Row));
    }
    return BN_OK;
}

// The format argument of a create entry point, read: the layout it names, whether the recording converts any format
// (bn_recording_read_f32), and what is wrong with the argument or the layout (pcm_layout_problem; NULL: nothing)
struct PcmArg {
    PcmLayout layout;
    bool any_format;
    const char *problem;
};
// the mono entry points take I16 and F32 only
PcmArg mono_pcm(int32_t format) { return {PcmLayout{format, 1, 0}, false, format != BN_PCM_I16 && format != BN_PCM_F32 ? "unknown PCM format" : nullptr}; }
const char *read_layout(const bn_pcm_layout *layout, size_t struct_size, PcmLayout *out) {
    if (!layout) return "null PCM layout";
    if (struct_size < sizeof(bn_pcm_layout)) return "struct_size is below sizeof(bn_pcm_layout)";
    *out = PcmLayout{layout->format, layout->channels, layout->channel};
    return nullptr;
}
PcmArg layout_pcm(const bn_pcm_layout *layout, size_t struct_size) {
    PcmLayout l;
    const char *why = read_layout(layout, struct_size, &l);
    return {l, true, why ? why : pcm_layout_problem(l)};
}

// every bn_recording_create*: the argument's problem refused, the bytes uploaded at once or by the store's thread
bn_status recording_create(int32_t device, const void *pcm, size_t n_frames, const PcmArg &arg, bool async, bn_recording **out) {
    if (!out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (arg.problem) return fail(BN_ERR_INVALID_ARG, arg.problem);
    const PcmLayout layout = pcm_normalised(arg.layout);
    if (n_frames && !pcm) return fail(BN_ERR_INVALID_ARG, "null PCM buffer");
    size_t bytes = 0;
    if (!pcm_bytes(layout, n_frames, &bytes) || bytes > SIZE_MAX - 16) return fail(BN_ERR_INVALID_ARG, "n_frames * channels * bytes per sample exceeds the address space");
    if (bn_status dst = require_any_device(); dst != BN_OK) return dst;
    BN_HIP_TRY(bn::use_device(device));
    std::unique_ptr<bn_recording> r(new bn_recording{device, layout, arg.any_format, false, std::make_shared<RecStore>(device, n_frames), n_frames});
    RecStore *st = r->store.get();
    BN_HIP_TRY(st->d_pcm.alloc(std::max<size_t>(bytes + PCM_READ_SLACK, 16)));
    if (!async) {
        if (bytes) {
            hipError_t e = gated::Memcpy(st->d_pcm, pcm, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) return fail(BN_ERR_BACKEND, std::string("recording upload failed: ") + hipGetErrorString(e));
        }
        *out = r.release();
        return BN_OK;
    }
    // the uploader holds the capture gate (shared) for one chunk's synchronous copy and a context's first-time graph capture takes it
    // exclusively: 4 MiB keeps a capture's wait behind a chunk well under a millisecond (32 MiB chunks stalled exactly the first
    // windows' captures the overlap was meant to help)
    const size_t chunk_mb = (size_t)std::max(1, sw_int(sw::BN_UPLOAD_CHUNK_MB));
    const size_t fb = pcm_frame_bytes(layout);
    st->chunk_frames = pcm_chunk_frames(layout, chunk_mb << 20);
    st->n_chunks = pcm_chunk_count(n_frames, st->chunk_frames);
    if (st->n_chunks) try {
        st->uploader = std::thread([st, pcm, fb]() {
            if (bn::use_device(st->device) != hipSuccess) st->upload_error.store(1);
            for (size_t k = 0; k < st->n_chunks && st->upload_error.load() == 0; k++) {
                const size_t a = k * st->chunk_frames, n = std::min(st->chunk_frames, st->n_frames - a);
                // a synchronous copy of its own kind (null stream; the contexts' streams are non-blocking and do not wait for it)
                if (gated::Memcpy(static_cast<char *>(st->d_pcm.get()) + a * fb, static_cast<const char *>(pcm) + a * fb, n * fb, hipMemcpyHostToDevice) != hipSuccess) {
                    (void)hipGetLastError();
                    st->upload_error.store(1);
                }
                {
                    std::lock_guard<std::mutex> lk(st->mu);
                    st->chunks_done.store(k + 1, std::memory_order_release);
                }
                st->cv.notify_all();
            }
            if (st->upload_error.load()) {  // wake every waiter
                std::lock_guard<std::mutex> lk(st->mu);
                st->chunks_done.store(st->n_chunks, std::memory_order_release);
                st->cv.notify_all();
            }
        });
    } catch (const std::exception &e) {  // std::system_error from the thread constructor must not cross the C boundary
        return fail(BN_ERR_BACKEND, std::string("could not start the upload thread: ") + e.what());
    }
    *out = r.release();
    return BN_OK;
}
}  // namespace

bn_status bn::read_pcm_layout(const bn_pcm_layout *layout, size_t struct_size, PcmLayout *out) {
    const char *why = read_layout(layout, struct_size, out);
    return why ? fail(BN_ERR_INVALID_ARG, why) : BN_OK;
}

// ---- polyphase resampler (no reference counterpart; design documented in include/birdnet_hip.h) ----
static double bessel_i0(double x) {
    double sum = 1.0, term = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
// shared with the live pool's streaming resampler (live.cpp): one table design, one implementation
ResampleTable bn::resample_factors(uint32_t src_rate, uint32_t dst_rate, uint32_t zc) {
    ResampleTable t;
    if (zc == 0) zc = 16;
    uint32_t a = dst_rate, b = src_rate;
    while (b) { const uint32_t r = a % b; a = b; b = r; }
    t.L = dst_rate / a;
    t.M = src_rate / a;
    const double ratio = (double)t.L / (double)t.M;
    const double fc = 0.5 * std::min(1.0, ratio);        // cutoff in cycles per SOURCE sample
    const double half = (double)zc / (2.0 * fc);          // support half-width in source samples
    const double taps = 2.0 * std::ceil(half);            // taps per phase (even)
    t.T = taps < 4294967295.0 ? (uint32_t)taps : 0xffffffffu;
    return t;
}
ResampleTable bn::make_resample_table(uint32_t src_rate, uint32_t dst_rate, uint32_t zc) {
    ResampleTable t = resample_factors(src_rate, dst_rate, zc);
    if (zc == 0) zc = 16;
    const double ratio = (double)t.L / (double)t.M;
    const double fc = 0.5 * std::min(1.0, ratio);
    const double half = (double)zc / (2.0 * fc);
    const double beta = 8.6, i0b = bessel_i0(beta), pi = 3.14159265358979323846;
    t.coef.assign((size_t)t.L * t.T, 0.0f);
    for (uint32_t p = 0; p < t.L; p++) {
        // output sample sits at source position base + p/L; tap j reads source index base + j - (T/2 - 1)
        std::vector<double> h(t.T);
        double sum = 0.0;
        for (uint32_t j = 0; j < t.T; j++) {
            const double tau = (double)p / (double)t.L - ((double)j - (double)(t.T / 2 - 1));  // output time - tap time
            const double u = tau / half;
            double w = 0.0;
            if (std::fabs(u) < 1.0) w = bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b;
            const double xarg = 2.0 * fc * tau;
            const double sinc = std::fabs(xarg) < 1e-12 ? 1.0 : std::sin(pi * xarg) / (pi * xarg);
            h[j] = 2.0 * fc * sinc * w;
            sum += h[j];
        }
        for (uint32_t j = 0; j < t.T; j++) t.coef[(size_t)p * t.T + j] = (float)(h[j] / sum);
    }
    return t;
}

namespace {
// bn_recording_create_resampled / bn_recording_create_layout_resampled: upload in the storage layout, convert on the device
bn_status recording_create_resampled(int32_t device, const void *pcm, size_t n_frames, const PcmArg &arg, uint32_t src_rate, uint32_t dst_rate,
                                     uint32_t zero_crossings, bn_recording **out) {
    if (!out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    // the layout form reads and checks its layout before it looks at the rates; the mono form looks at its rates before its format
    const char *rates = src_rate && dst_rate ? nullptr : "sample rates must be positive";
    const char *why = arg.any_format ? (arg.problem ? arg.problem : rates) : (rates ? rates : arg.problem);
    if (why) return fail(BN_ERR_INVALID_ARG, why);
    bn_recording *src = nullptr;
    bn_status st = recording_create(device, pcm, n_frames, arg, false, &src);
    if (st != BN_OK || src_rate == dst_rate) return *out = src, st;  // equal rates: the recording as uploaded
    std::unique_ptr<bn_recording> src_owner(src);
    const ResampleTable t = make_resample_table(src_rate, dst_rate, zero_crossings);
    const size_t n_dst = (size_t)(((unsigned __int128)n_frames * t.L + t.M - 1) / t.M);
    std::unique_ptr<bn_recording> r(new bn_recording{device, PcmLayout{BN_PCM_F32, 1, 0}, arg.any_format, true, std::make_shared<RecStore>(device, n_dst), n_dst});
    DeviceBuf<float> d_table;
    hipError_t e = r->store->d_pcm.alloc(std::max<size_t>(n_dst * sizeof(float), 16));
    if (e == hipSuccess) e = d_table.alloc(t.coef.size() * sizeof(float));
    if (e == hipSuccess) e = gated::Memcpy(d_table, t.coef.data(), t.coef.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(BN_ERR_BACKEND, std::string("resampling failed: ") + hipGetErrorString(e));
    bn::clear_launch_state();
    launch_resample(nullptr, static_cast<float *>(r->store->d_pcm.get()), src->src(), d_table, n_frames, n_dst, t.L, t.M, t.T);
    if ((st = bn::check_launch("resample")) != BN_OK) return st;
    if ((e = gated::DeviceSynchronize()) != hipSuccess) return fail(BN_ERR_BACKEND, std::string("resampling failed: ") + hipGetErrorString(e));
    *out = r.release();
    return BN_OK;
}

// the refusals of a window range, without the wait of check_windows
bn_status check_window_range(const bn_recording *r, size_t S, size_t step, size_t first, size_t count) {
    if (!r) return fail(BN_ERR_INVALID_ARG, "null recording");
    if (S == 0 || S % 4 != 0 || S > 0xffffffffull) return fail(BN_ERR_INVALID_ARG, "segment_samples must be a positive multiple of 4");
    if (step == 0) return fail(BN_ERR_INVALID_ARG, "step_samples must be positive (overlap shorter than the segment)");
    const size_t total = bn_chunk_count(r->n_samples, step);
    if (first > total || count > total - first) return fail(BN_ERR_INVALID_ARG, "window range [" + std::to_string(first) + ", " + std::to_string(first + count) + ") exceeds the " + std::to_string(total) + " windows of the recording");
    return BN_OK;
}
}  // namespace

bn_status bn::check_windows(const bn_recording *r, size_t S, size_t step, size_t first, size_t count, int32_t *device) {
    if (bn_status st = check_window_range(r, S, step, first, count); st != BN_OK) return st;
    // an asynchronously uploaded recording: the last sample these windows read must have arrived before their kernel is launched
    if (count && r->n_samples && !recording_wait_samples(r, std::min(r->n_samples - 1, (first + count - 1) * step + S - 1)))
        return fail(BN_ERR_BACKEND, "recording upload failed");
    if (device) *device = r->device;
    return BN_OK;
}

bn_status bn::enqueue_windows(hipStream_t stream, int32_t device, float *dst, const bn_recording *r, size_t S, size_t step, size_t first, size_t count) {
    if (r->device != device) return fail(BN_ERR_INVALID_ARG, "recording and context live on different devices");
    bn::clear_launch_state();
    launch_windows(stream, dst, r->src(), r->n_samples, (uint64_t)first * step, step, (uint32_t)S, (uint32_t)count);
    return bn::check_launch("window kernel");
}

namespace {
// a caller's list of bn_window_ref, read and refused: its distinct recordings, its rows, and the plan of its gather
struct WindowList {
    std::vector<const bn_recording *> recs;
    std::vector<wlist::Row> rows;
    std::vector<int32_t> sources;
    std::vector<uint64_t> windows;
    wlist::Plan plan;
};

// `device` < 0: every recording lies where the first one does
bn_status read_window_list(const bn_window_ref *refs, size_t count, size_t struct_size, size_t S, int32_t device, WindowList *out) {
    if (!refs) return fail(BN_ERR_INVALID_ARG, "null window list");
    if (struct_size < sizeof(bn_window_ref)) return fail(BN_ERR_INVALID_ARG, "struct_size is below sizeof(bn_window_ref)");
    if (S == 0 || S % 4 != 0 || S > 0xffffffffull) return fail(BN_ERR_INVALID_ARG, "segment_samples must be a positive multiple of 4");
    // before anything is sized by the caller's count (build() repeats the first for the stand-alone plan check)
    if (count > 0xffffffffull) return fail(BN_ERR_INVALID_ARG, "a window list holds fewer than 2^32 rows");
    if (count > SIZE_MAX / sizeof(float) / S) return fail(BN_ERR_INVALID_ARG, "count * segment_samples exceeds the address space");
    const bool of_ctx = device >= 0;
    std::map<const bn_recording *, uint32_t> seen;
    std::vector<wlist::Rec> infos;
    try {
        out->rows.resize(count);
        out->sources.resize(count);
        out->windows.resize(count);
    } catch (const std::exception &) {  // must not cross the C boundary
        return fail(BN_ERR_INVALID_ARG, "no host memory for a window list of " + std::to_string(count) + " rows");
    }
    for (size_t i = 0; i < count; i++) {
        bn_window_ref ref;  // through the caller's stride, whatever its alignment
        memcpy(&ref, reinterpret_cast<const char *>(refs) + i * struct_size, sizeof(ref));
        if (!ref.recording) return fail(BN_ERR_INVALID_ARG, "row " + std::to_string(i) + ": null recording");
        if (device < 0) device = ref.recording->device;
        if (ref.recording->device != device)
            return fail(BN_ERR_INVALID_ARG, "row " + std::to_string(i) + ": its recording lives on device " + std::to_string(ref.recording->device) +
                                                ", the " + (of_ctx ? "context" : "list's first recording") + " on device " + std::to_string(device));
        auto it = seen.find(ref.recording);
        if (it == seen.end()) {
            it = seen.emplace(ref.recording, (uint32_t)out->recs.size()).first;
            out->recs.push_back(ref.recording);
            infos.push_back(wlist::Rec{ref.recording->layout, (uint64_t)ref.recording->n_samples});
        }
        out->rows[i] = wlist::Row{it->second, ref.start};
        out->sources[i] = ref.source;
        out->windows[i] = ref.window;
    }
    return wlist::build(infos, out->rows.data(), count, S, &out->plan);
}

// an asynchronous recording: the last frame any of its rows reads must have arrived before the gather is launched
bn_status wait_window_list(const WindowList &wl) {
    for (size_t r = 0; r < wl.recs.size(); r++)
        if (wl.plan.used[r] && !recording_wait_samples(wl.recs[r], (size_t)wl.plan.last[r])) return fail(BN_ERR_BACKEND, "recording upload failed");
    return BN_OK;
}

// the gather of a read list on `s`: one launch per reader kind and 128 rows, row i of the list to row i of dst [count, S]
void launch_list_rows(hipStream_t s, float *dst, uint32_t S, const WindowList &wl) {
    std::vector<WindowListSrc> rows;
    for (const wlist::Launch &ln : wl.plan.launches) {
        rows.resize(ln.count);
        for (size_t j = 0; j < ln.count; j++) {
            const uint32_t i = wl.plan.order[ln.first + j];
            const bn_recording *rc = wl.recs[wl.rows[i].rec];
            const char *at = static_cast<const char *>(rc->store->d_pcm.get()) + pcm_frame_offset(rc->layout, (size_t)wl.rows[i].start);
            rows[j] = WindowListSrc{PcmSrc{at, rc->layout}, (uint32_t)wlist::valid_frames(wl.rows[i].start, rc->n_samples, S), i};
        }
        launch_window_list(s, dst, S, rows.data(), (uint32_t)ln.count);  // the reader, and its fields per row, are pcm_visit's
    }
}
}  // namespace

extern "C" {

// the six create forms: the caller's format read by mono_pcm / layout_pcm, then the worker
bn_status bn_recording_create(int32_t device, const void *pcm, size_t n_samples, int32_t format, bn_recording **out) {
    return recording_create(device, pcm, n_samples, mono_pcm(format), false, out);
}
bn_status bn_recording_create_async(int32_t device, const void *pcm, size_t n_samples, int32_t format, bn_recording **out) {
    return recording_create(device, pcm, n_samples, mono_pcm(format), true, out);
}
bn_status bn_recording_create_layout(int32_t device, const void *pcm, size_t n_frames, const bn_pcm_layout *layout, size_t struct_size, bn_recording **out) {
    return recording_create(device, pcm, n_frames, layout_pcm(layout, struct_size), false, out);
}
bn_status bn_recording_create_layout_async(int32_t device, const void *pcm, size_t n_frames, const bn_pcm_layout *layout, size_t struct_size,
                                           bn_recording **out) {
    return recording_create(device, pcm, n_frames, layout_pcm(layout, struct_size), true, out);
}
bn_status bn_recording_create_resampled(int32_t device, const void *pcm, size_t n_samples, int32_t format, uint32_t src_rate, uint32_t dst_rate,
                                        uint32_t zero_crossings, bn_recording **out) {
    return recording_create_resampled(device, pcm, n_samples, mono_pcm(format), src_rate, dst_rate, zero_crossings, out);
}
bn_status bn_recording_create_layout_resampled(int32_t device, const void *pcm, size_t n_frames, const bn_pcm_layout *layout, size_t struct_size,
                                               uint32_t src_rate, uint32_t dst_rate, uint32_t zero_crossings, bn_recording **out) {
    return recording_create_resampled(device, pcm, n_frames, layout_pcm(layout, struct_size), src_rate, dst_rate, zero_crossings, out);
}

bn_status bn_recording_view_channel(const bn_recording *r, int32_t channel, bn_recording **out) {
    if (!out) return fail(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (!r) return fail(BN_ERR_INVALID_ARG, "null recording");
    PcmLayout l = r->layout;
    l.channel = channel;
    if (const char *why = pcm_layout_problem(l)) {
        if (r->resampled)
            return fail(BN_ERR_INVALID_ARG, "a resampled recording has no storage-format bytes left: it is mono f32 and takes channel 0 or BN_PCM_MIX only");
        return fail(BN_ERR_INVALID_ARG, std::string(why) + " (channel " + std::to_string(channel) + " of " + std::to_string(l.channels) + ")");
    }
    *out = new bn_recording{r->device, pcm_normalised(l), true, r->resampled, r->store, r->n_samples};
    return BN_OK;
}

bn_status bn_recording_wait(const bn_recording *r) {
    if (!r) return fail(BN_ERR_INVALID_ARG, "null recording");
    if (!recording_wait_samples(r, r->n_samples ? r->n_samples - 1 : 0)) return fail(BN_ERR_BACKEND, "recording upload failed");
    return BN_OK;
}

size_t bn_resample_table(uint32_t src_rate, uint32_t dst_rate, uint32_t zero_crossings, float *table, size_t cap, uint32_t *L_out, uint32_t *M_out,
                         uint32_t *T_out) {
    if (src_rate == 0 || dst_rate == 0) return 0;
    const ResampleTable t = make_resample_table(src_rate, dst_rate, zero_crossings);
    if (L_out) *L_out = t.L;
    if (M_out) *M_out = t.M;
    if (T_out) *T_out = t.T;
    if (table) memcpy(table, t.coef.data(), std::min(cap, t.coef.size()) * sizeof(float));
    return t.coef.size();
}

bn_status bn_recording_read_f32(const bn_recording *r, size_t first, size_t count, float *host_out) {
    if (!r || (count && !host_out)) return fail(BN_ERR_INVALID_ARG, "null argument");
    if (r->layout.format != BN_PCM_F32 && !r->any_format) return fail(BN_ERR_INVALID_ARG, "recording is not f32");
    if (first > r->n_samples || count > r->n_samples - first) return fail(BN_ERR_INVALID_ARG, "sample range exceeds the recording");
    if (count == 0) return BN_OK;
    if (!recording_wait_samples(r, first + count - 1)) return fail(BN_ERR_BACKEND, "recording upload failed");
    BN_HIP_TRY(bn::use_device(r->device));
    if (pcm_is_plain(r->layout) && r->layout.format == BN_PCM_F32) {
        BN_HIP_TRY(gated::Memcpy(host_out, static_cast<const float *>(r->store->d_pcm.get()) + first, count * sizeof(float), hipMemcpyDeviceToHost));
        return BN_OK;
    }
    // any other layout: the window kernel over [first, first + count), one window of up to 2^24 frames at a time
    const size_t piece = (size_t)1 << 24;
    DeviceBuf<float> d;
    BN_HIP_TRY(d.alloc(std::min(piece, (count + 3) / 4 * 4) * sizeof(float)));
    for (size_t done = 0; done < count; done += piece) {
        const size_t n = std::min(piece, count - done);
        bn_status st = launch_and_read("sample read", "sample read failed: ", host_out + done, d, n * sizeof(float), [&] {
            launch_windows(nullptr, d, r->src(), r->n_samples, (uint64_t)(first + done), 1, (uint32_t)((n + 3) / 4 * 4), 1);
        });
        if (st != BN_OK) return st;
    }
    return BN_OK;
}

void bn_recording_free(bn_recording *r) { delete r; }

size_t bn_recording_samples(const bn_recording *r) { return r ? r->n_samples : 0; }

size_t bn_chunk_count(size_t n_samples, size_t step_samples) {
    if (n_samples == 0 || step_samples == 0) return 0;
    return (n_samples + step_samples - 1) / step_samples;  // one window for every pos = k*step < n_samples
}

bn_status bn_recording_windows(const bn_recording *r, size_t segment_samples, size_t step_samples, size_t first_window, size_t count, float *host_out) {
    bn_status st = bn::check_windows(r, segment_samples, step_samples, first_window, count, nullptr);
    if (st != BN_OK) return st;
    if (count == 0) return BN_OK;
    if (!host_out) return fail(BN_ERR_INVALID_ARG, "null host buffer");
    BN_HIP_TRY(bn::use_device(r->device));
    DeviceBuf<float> d;
    BN_HIP_TRY(d.alloc(count * segment_samples * sizeof(float)));
    return launch_and_read("window kernel", "window kernel failed: ", host_out, d, count * segment_samples * sizeof(float), [&] {
        launch_windows(nullptr, d, r->src(), r->n_samples, (uint64_t)first_window * step_samples, step_samples, (uint32_t)segment_samples, (uint32_t)count);
    });
}

// ---- window levels and list steps (include/birdnet_hip.h, "Window levels and list steps"; kernels in levels.hip) ----
bn_status bn_recording_levels(const bn_recording *r, size_t segment_samples, size_t step_samples, size_t first_window, size_t count,
                              bn_window_level *out, size_t struct_size) {
    if (struct_size < sizeof(bn_window_level)) return fail(BN_ERR_INVALID_ARG, "struct_size is below sizeof(bn_window_level)");
    bn_status st = bn::check_windows(r, segment_samples, step_samples, first_window, count, nullptr);
    if (st != BN_OK) return st;
    if (count == 0) return BN_OK;
    if (!out) return fail(BN_ERR_INVALID_ARG, "null output buffer");
    BN_HIP_TRY(bn::use_device(r->device));
    // one workgroup per window, at most 2^20 windows per launch
    return rows_in_pieces<WindowLevel>("levels", "level kernel failed: ", count, (size_t)1 << 20, out, struct_size, [&](size_t done, size_t n, WindowLevel *d) {
        launch_levels(nullptr, d, r->src(), r->n_samples, (uint64_t)(first_window + done) * step_samples, step_samples, (uint32_t)segment_samples, (uint32_t)n);
    });
}

// ---- band-limited window levels (include/birdnet_hip.h, "bn_recording_band_levels"; kernel in band_levels.hip, arithmetic in band_plan.h) ----
bn_status bn_recording_band_levels(const bn_recording *r, size_t segment_samples, size_t step_samples, size_t first_window, size_t count,
                                   const bn_band_spec *spec, size_t spec_size, bn_window_bands *out, size_t struct_size) {
    if (struct_size < sizeof(bn_window_bands)) return fail(BN_ERR_INVALID_ARG, "struct_size is below sizeof(bn_window_bands)");
    bn_status st = check_window_range(r, segment_samples, step_samples, first_window, count);
    if (st != BN_OK) return st;
    band::Plan plan;
    if ((st = band::check_spec(spec, spec_size, segment_samples, &plan)) != BN_OK) return st;
    if (count == 0) return BN_OK;
    if (!out) return fail(BN_ERR_INVALID_ARG, "null output buffer");
    // an asynchronously uploaded recording: the last sample any frame of these windows reads must have arrived
    uint64_t last = 0;
    if (band::last_sample_read(r->n_samples, first_window + count - 1, step_samples, plan.span, &last) && !recording_wait_samples(r, (size_t)last))
        return fail(BN_ERR_BACKEND, "recording upload failed");
    BN_HIP_TRY(bn::use_device(r->device));
    const float *tab = nullptr;
    float scale = 0.0f;
    BN_HIP_TRY(band_tables(r->device, plan.N, &tab, &scale));
    // one workgroup per window, at most 2^20 windows per launch
    return rows_in_pieces<WindowBands>("band levels", "band level kernel failed: ", count, (size_t)1 << 20, out, struct_size, [&](size_t done, size_t n, WindowBands *d) {
        launch_band_levels(nullptr, d, r->src(), r->n_samples, (uint64_t)(first_window + done) * step_samples, step_samples, (uint32_t)segment_samples,
                           (uint32_t)n, plan, tab, scale);
    });
}

bn_status bn_band_bins(uint32_t sample_rate, uint32_t frame, double lo_hz, double hi_hz, uint32_t *bin_lo, uint32_t *bin_hi) {
    return band::bins(sample_rate, frame, lo_hz, hi_hz, bin_lo, bin_hi);
}

bn_status bn_recording_window_list(const bn_window_ref *refs, size_t count, size_t struct_size, size_t segment_samples, float *host_out) {
    if (count == 0) return BN_OK;
    WindowList wl;
    bn_status st = read_window_list(refs, count, struct_size, segment_samples, -1, &wl);
    if (st != BN_OK) return st;
    if (!host_out) return fail(BN_ERR_INVALID_ARG, "null host buffer");
    if ((st = wait_window_list(wl)) != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(wl.recs[0]->device));
    DeviceBuf<float> d;
    BN_HIP_TRY(d.alloc(count * segment_samples * sizeof(float)));
    return launch_and_read("window list gather", "window list gather failed: ", host_out, d, count * segment_samples * sizeof(float),
                           [&] { launch_list_rows(nullptr, d, (uint32_t)segment_samples, wl); });
}

bn_status bn_step_window_list(bn_ctx *c, const bn_window_ref *refs, size_t count, size_t struct_size, size_t top_k, int32_t has_min, float min_conf,
                              int32_t sync) {
    if (!c) return fail(BN_ERR_INVALID_ARG, "null context");
    bn::CtxStepInput ci;
    bn_status st = bn::ctx_step_input(c, top_k, &ci);
    if (st != BN_OK) return st;
    if (count == 0) return fail(BN_ERR_INVALID_ARG, "an empty window list");
    if (count > ci.max_batch) return fail(BN_ERR_INVALID_ARG, "batch size " + std::to_string(count) + " exceeds context max " + std::to_string(ci.max_batch));
    WindowList wl;
    if ((st = read_window_list(refs, count, struct_size, ci.sample_count, ci.device, &wl)) != BN_OK) return st;
    size_t n_sources = 0;
    for (size_t i = 0; i < count; i++) {
        if (wl.sources[i] < 0) return fail(BN_ERR_INVALID_ARG, "row " + std::to_string(i) + ": source " + std::to_string(wl.sources[i]) + " is negative");
        n_sources = std::max(n_sources, (size_t)wl.sources[i] + 1);
        // the list brings its own window numbers: what the tracker would refuse of a row only after the step was enqueued
        if (ci.tracked && wl.windows[i] >= ((uint64_t)1 << 31))
            return fail(BN_ERR_INVALID_ARG, "row " + std::to_string(i) + ": a tracked window number must be below 2^31");
    }
    // what an attached prior and tracker refuse of a live step over that many sources
    if ((st = bn::ctx_step_check(c, n_sources, 0, 0)) != BN_OK) return st;
    if ((st = wait_window_list(wl)) != BN_OK) return st;
    BN_HIP_TRY(bn::use_device(ci.device));
    // stream order keeps the gather behind whatever the context still has in flight; the descriptors are kernel arguments, so
    // nothing here can race a step in flight
    bn::clear_launch_state();
    launch_list_rows(ci.stream, ci.d_input, (uint32_t)ci.sample_count, wl);
    if ((st = bn::check_launch("window list gather")) != BN_OK) return st;
    // row i is window refs[i].window of source refs[i].source (the copies made above, read before the step returns)
    return bn::step_device(c, ci.d_input, bn::StepRows{count, true, wl.sources.data(), wl.windows.data(), 0}, top_k, has_min, min_conf, sync);
}

}  // extern "C"
