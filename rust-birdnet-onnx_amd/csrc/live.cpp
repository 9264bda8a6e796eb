// Live ingest pool behind the C ABI (include/birdnet_hip.h, bn_live_*, bn_step_live): per-source rings in one device slab
// [n_sources][ring_samples] in the storage format, host bookkeeping of what is pushed, ready and scheduled, and the device
// ordering between the pool's scatters and the contexts' gathers.  Kernels in live.hip.
//
// Ring coordinates.  A source's sample x lives at ring index (base + x) % ring_samples.  A reset moves base past everything
// pushed so far, so "ring-absolute" positions (base + x) only grow and a gather of the old stream that is still in flight is
// ordered against the new stream's scatters by the same rule as any other.
//
// Ordering.  Each scatter records `scatter_ev` on the pool's stream; a step makes its context's stream wait for it before the
// gather.  Each gather records an event on its context's stream; per source the pool keeps (first ring-absolute start read,
// gather id) of the gathers not yet known complete, and a scatter that overwrites ring-absolute positions below p makes the
// pool's stream wait for every such gather that started reading below p.  The per-row descriptors travel as kernel
// arguments, so nothing a step writes on the host can race with an earlier step still in flight.
//
// Resampling pools (bn_live_create_rates).  The ring holds f32 at the model's rate; `pushed` counts the FINAL outputs written to
// it, `in_pushed` the source samples received.  A push converts [F(in_pushed), F(in_pushed + n)) in its scatter
// (live_resample_kernel), then a second launch on the pool's stream moves the source's last T - 1 samples into its device
// history; a close converts the tail [F, ceil(in_pushed * L / M)) with zeros past the end.  Everything downstream of `pushed`
// (readiness, rows, ordering, reset) is the plain pool's code.
//
// Layout pools (bn_live_create_layout).  Pushes carry interleaved frames in any format (pcm_layout.h) and count FRAMES.  Mono
// int16 / float pushes are stored as they are, as ever; for any other layout the ring holds f32 and the scatter converts each
// frame to the layout rule's sample as it lands (live.hip), so everything behind the ring is the f32 pool's code and bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "capi_internal.h"
#include "live.h"
#include "switches.h"

namespace {

constexpr int N_STAGE = 3;  // pinned staging blocks in rotation

struct Source {
    uint64_t base = 0;       // ring-absolute position of sample 0 of the current stream
    uint64_t pushed = 0;     // samples pushed since creation / the last reset
    uint64_t n_ready = 0;    // windows [0, n_ready) have become ready
    uint64_t sched = 0;      // windows [0, sched) have been scheduled
    bool closed = false;
    uint64_t in_pushed = 0;  // resampling pools: source samples pushed since creation / the last reset
    int32_t table = -1;      // resampling pools: the source's table in bn_live::tables (-1: at the model's rate)
    uint32_t rate = 0;       // resampling pools: the source's sample rate
    std::deque<std::pair<uint64_t, uint64_t>> reads;  // (first ring-absolute start read, gather id), increasing
};

struct Gather {
    uint64_t id;
    bn::Event ev;
    bool done;
};

struct Stage {
    bn::PinnedBuf<char> h;  // pinned: [tiles][data]
    bn::DeviceBuf<char> d;  // device copy of the block (copy mode only)
    size_t cap = 0;
    bn::Event ev;
    bool used = false;
};

}  // namespace

struct bn_live {
    int device = 0;
    int32_t n_sources = 0;
    int32_t format = BN_PCM_I16;
    size_t esz = 2;
    size_t S = 0, step = 0, R = 0;
    bn::Stream stream;  // before everything its work touches (device_mem.h)
    bn::Event scatter_ev;
    bn::DeviceBuf<void> slab;
    bn::DeviceBuf<float> d_window;  // bn_live_read_window's output [S]
    bool scattered = false;
    bool copy_mode = false;  // BN_LIVE_SCATTER=copy: one async H2D copy of the staging block, then the kernel on device memory
    std::vector<Source> src;
    std::deque<std::pair<int32_t, uint64_t>> queue;  // ready, unscheduled windows (source, k) in sequence order
    std::deque<Gather> gathers;                       // gathers not yet known complete, ids increasing
    uint64_t next_gather = 0;
    std::vector<bn::Event> free_events;
    std::vector<int32_t> touched;  // push_impl: per source, its entry in the call's list of touched sources (-1: none)
    Stage stage[N_STAGE];
    int next_stage = 0;
    // what pushes carry (the ring stores it only when it is mono int16 / float and the pool does not resample; else the ring is f32)
    bn::PcmLayout in_layout;
    size_t in_esz = 2;  // bytes of one pushed frame
    // resampling pools
    bool rates = false;
    uint32_t dst_rate = 0;
    std::vector<bn::LiveRsTable> tables;
    std::vector<uint32_t> table_tile;  // outputs per tile, per table: the span of a tile fits the table's span_cap
    bn::DeviceBuf<bn::LiveRsTable> d_tables;
    bn::DeviceBuf<float> d_coef;
    bn::DeviceBuf<float> d_hist;  // [n_sources][hist_cap]
    size_t hist_cap = 0;
    uint32_t lds_bytes = 0;
    ~bn_live() {
        (void)bn::use_device(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto &g : gathers) (void)hipEventSynchronize(g.ev);
    }
};

namespace {

using bn::set_last_error;

bn_status invalid(const std::string &msg) { return set_last_error(BN_ERR_INVALID_ARG, msg); }

bool source_ok(const bn_live *l, int32_t s) { return l && s >= 0 && s < l->n_sources; }

uint64_t ceil_muldiv(uint64_t a, uint32_t mul, uint32_t div) { return (uint64_t)(((unsigned __int128)a * mul + div - 1) / div); }

// outputs of a resampled stream that are final after `pushed` source samples: output n reads sources up to (n*M)/L + T/2
uint64_t final_outputs(uint32_t L, uint32_t M, uint32_t T, uint64_t pushed, bool closed) {
    if (closed) return ceil_muldiv(pushed, L, M);
    return pushed > T / 2 ? ceil_muldiv(pushed - T / 2, L, M) : 0;
}

uint64_t outputs_of(const bn_live *l, const Source &s, uint64_t in_pushed, bool closed) {
    if (s.table < 0) return in_pushed;
    const bn::LiveRsTable &t = l->tables[(size_t)s.table];
    return final_outputs(t.L, t.M, t.T, in_pushed, closed);
}

size_t room_of(const bn_live *l, const Source &s) {
    const uint64_t needed_from = std::min<uint64_t>(s.pushed, s.sched * l->step);
    if (l->rates && s.table >= 0) {
        // the ring must hold every output up to the tail a close flushes: ceil((in_pushed + n) * L / M) <= R + needed_from
        const bn::LiveRsTable &t = l->tables[(size_t)s.table];
        const uint64_t lim = (uint64_t)(((unsigned __int128)(l->R + needed_from) * t.M) / t.L);
        return lim > s.in_pushed ? (size_t)(lim - s.in_pushed) : 0;
    }
    return l->R - (size_t)(s.pushed - needed_from);
}

// windows that are ready given what was pushed (and whether the stream is closed)
uint64_t ready_limit(const bn_live *l, const Source &s) {
    if (s.closed) return s.pushed ? (s.pushed + l->step - 1) / l->step : 0;
    return s.pushed >= l->S ? (s.pushed - l->S) / l->step + 1 : 0;
}

void make_ready(bn_live *l, int32_t source) {
    Source &s = l->src[source];
    const uint64_t lim = ready_limit(l, s);
    for (uint64_t k = s.n_ready; k < lim; k++) l->queue.emplace_back(source, k);
    s.n_ready = std::max(s.n_ready, lim);
}

bn::LiveRow row_of(const bn_live *l, const Source &s, uint64_t k) {
    const uint64_t start = k * l->step;
    bn::LiveRow r;
    r.base = 0;  // set by the caller (slot offset)
    r.pos = (uint32_t)((s.base + start) % l->R);
    r.valid = (uint32_t)std::min<uint64_t>(l->S, s.pushed - start);
    return r;
}

// retire completed gathers from the front, whichever sources they read, and recycle their events: every push and step calls
// this, so the pool holds an event only for gathers in flight (and a few recycled ones), however its sources come and go
void retire_gathers(bn_live *l) {
    while (!l->gathers.empty()) {
        Gather &g = l->gathers.front();
        if (!g.done && hipEventQuery(g.ev) == hipSuccess) g.done = true;
        if (!g.done) break;
        l->free_events.push_back(std::move(g.ev));
        l->gathers.pop_front();
    }
}

// is gather `id` complete?  (queries its event once)
bool gather_done(bn_live *l, uint64_t id) {
    if (l->gathers.empty() || id < l->gathers.front().id) return true;
    Gather &g = l->gathers[id - l->gathers.front().id];
    if (!g.done && hipEventQuery(g.ev) == hipSuccess) g.done = true;
    const bool d = g.done;
    retire_gathers(l);
    return d;
}

// the pool's stream waits for every gather of source s that read ring-absolute positions below `limit`
bn_status wait_readers(bn_live *l, Source &s, uint64_t limit, std::vector<uint64_t> &waited) {
    while (!s.reads.empty() && gather_done(l, s.reads.front().second)) s.reads.pop_front();
    for (const auto &rd : s.reads) {
        if (rd.first >= limit) break;
        if (std::find(waited.begin(), waited.end(), rd.second) != waited.end() || gather_done(l, rd.second)) continue;
        BN_HIP_TRY(hipStreamWaitEvent(l->stream, l->gathers[rd.second - l->gathers.front().id].ev, 0));
        waited.push_back(rd.second);
    }
    return BN_OK;
}

// the next pinned staging block, free to be written and at least `bytes` large
bn_status acquire_stage(bn_live *l, size_t bytes, Stage **out) {
    Stage &st = l->stage[l->next_stage];
    if (st.used) BN_HIP_TRY(hipEventSynchronize(st.ev));
    if (bytes > st.cap) {
        const size_t cap = std::max(bytes, st.cap * 3 / 2);
        st.h.reset();
        st.d.reset();
        st.cap = 0;
        BN_HIP_TRY(st.h.alloc(cap));
        if (l->copy_mode) BN_HIP_TRY(st.d.alloc(cap));
        st.cap = cap;
    }
    *out = &st;
    return BN_OK;
}

size_t pad256(size_t b) { return (b + 255) / 256 * 256; }

// The scatter of a resampling pool.  want: per touched source the source samples this call adds (0 with closing: the tail).
// Staging block: [jobs][tiles][data], the data grouped by source so that a job's new samples are contiguous.  On success the
// sources' rings hold their outputs up to outputs_of(in_pushed + added, closing); the caller does the bookkeeping.
bn_status scatter_rates(bn_live *l, const std::vector<std::pair<int32_t, uint64_t>> &want, size_t n, const int32_t *sources, const void *const *pcm,
                        const size_t *n_samples, bool closing) {
    std::vector<bn::LiveRsJob> jobs(want.size());
    std::vector<bn::LiveRsTile> tiles;
    std::vector<uint64_t> out_end(want.size());
    uint64_t total = 0;
    for (size_t j = 0; j < want.size(); j++) {
        const int32_t si = want[j].first;
        const Source &s = l->src[si];
        bn::LiveRsJob &jb = jobs[j];
        jb.p0 = s.in_pushed;
        jb.hist = (uint64_t)si * l->hist_cap;
        jb.src = (uint32_t)total;
        jb.n_in = (uint32_t)want[j].second;
        jb.table = s.table < 0 ? bn::LIVE_RS_PASS : (uint32_t)s.table;
        jb.pad = 0;
        total += want[j].second;
        const uint64_t out1 = outputs_of(l, s, s.in_pushed + want[j].second, closing);
        out_end[j] = out1;
        const uint32_t tile = s.table < 0 ? bn::LIVE_TILE : l->table_tile[(size_t)s.table];
        const uint64_t slot = (uint64_t)si * l->R;
        for (uint64_t o = s.pushed; o < out1;) {
            const uint64_t pos = (s.base + o) % l->R;
            const uint32_t len = (uint32_t)std::min<uint64_t>({out1 - o, l->R - pos, tile});
            tiles.push_back(bn::LiveRsTile{slot + pos, o, len, (uint32_t)j});
            o += len;
        }
    }
    BN_HIP_TRY(bn::use_device(l->device));
    retire_gathers(l);
    if (tiles.empty() && total == 0) return BN_OK;
    const size_t jobs_b = pad256(jobs.size() * sizeof(bn::LiveRsJob));
    const size_t tiles_b = pad256(tiles.size() * sizeof(bn::LiveRsTile));
    const size_t bytes = jobs_b + tiles_b + total * l->in_esz + bn::PCM_READ_SLACK;
    Stage *stp = nullptr;
    bn_status bs = acquire_stage(l, bytes, &stp);
    if (bs != BN_OK) return bs;
    Stage &st = *stp;
    memcpy(st.h, jobs.data(), jobs.size() * sizeof(bn::LiveRsJob));
    memcpy(st.h + jobs_b, tiles.data(), tiles.size() * sizeof(bn::LiveRsTile));
    {
        std::vector<size_t> cursor(want.size());
        for (size_t j = 0; j < want.size(); j++) cursor[j] = (size_t)jobs[j].src;
        char *data = st.h + jobs_b + tiles_b;
        for (size_t i = 0; i < n; i++) {
            if (!n_samples[i]) continue;
            size_t &c = cursor[(size_t)l->touched[sources[i]]];
            memcpy(data + c * l->in_esz, pcm[i], n_samples[i] * l->in_esz);
            c += n_samples[i];
        }
    }
    // the scatter waits for the gathers that read the ring space it overwrites: positions below (write end - R)
    std::vector<uint64_t> waited;
    for (size_t j = 0; j < want.size(); j++) {
        Source &s = l->src[want[j].first];
        const uint64_t end = s.base + out_end[j];
        if (out_end[j] > s.pushed && end > l->R) {
            bs = wait_readers(l, s, end - l->R, waited);
            if (bs != BN_OK) return bs;
        }
    }
    bn::clear_launch_state();
    const char *blk = st.h;
    if (l->copy_mode) {
        BN_HIP_TRY(hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, l->stream));
        blk = st.d;
    }
    const bn::LiveRsJob *d_jobs = reinterpret_cast<const bn::LiveRsJob *>(blk);
    const bn::PcmSrc staged{blk + jobs_b + tiles_b, l->in_layout};
    bn::launch_live_resample(l->stream, static_cast<float *>(l->slab.get()), staged, l->d_tables, l->d_coef, l->d_hist, d_jobs,
                             reinterpret_cast<const bn::LiveRsTile *>(blk + jobs_b), (uint32_t)tiles.size(), l->lds_bytes);
    if (!closing) bn::launch_live_history(l->stream, l->d_hist, staged, l->d_tables, d_jobs, (uint32_t)jobs.size());
    if (bn_status lst = bn::check_launch("live resample"); lst != BN_OK) return lst;
    BN_HIP_TRY(hipEventRecord(st.ev, l->stream));
    BN_HIP_TRY(hipEventRecord(l->scatter_ev, l->stream));
    st.used = true;
    l->scattered = true;
    l->next_stage = (l->next_stage + 1) % N_STAGE;
    return BN_OK;
}

bn_status push_impl(bn_live *l, size_t n, const int32_t *sources, const void *const *pcm, const size_t *n_samples) {
    if (!l) return invalid("null pool");
    if (n && (!sources || !pcm || !n_samples)) return invalid("null argument");
    // validate the whole call before anything changes
    std::vector<std::pair<int32_t, uint64_t>> want;  // per source touched: samples asked for (l->touched maps a source to its entry)
    struct Untouch {  // l->touched is all -1 again whenever this call returns
        bn_live *l;
        std::vector<std::pair<int32_t, uint64_t>> &want;
        ~Untouch() {
            for (const auto &w : want) l->touched[w.first] = -1;
        }
    } untouch{l, want};
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        const int32_t s = sources[i];
        if (!source_ok(l, s)) return invalid("source " + std::to_string(s) + " out of range [0, " + std::to_string(l->n_sources) + ")");
        if (n_samples[i] && !pcm[i]) return invalid("null PCM buffer for source " + std::to_string(s));
        if (l->src[s].closed) return invalid("source " + std::to_string(s) + " is closed (reset it to start a new stream)");
        if (l->touched[s] < 0) {
            l->touched[s] = (int32_t)want.size();
            want.emplace_back(s, n_samples[i]);
        } else {
            want[l->touched[s]].second += n_samples[i];
        }
        total += n_samples[i];
    }
    for (const auto &w : want)
        if (w.second > room_of(l, l->src[w.first]))
            return invalid("push of " + std::to_string(w.second) + " samples to source " + std::to_string(w.first) + " exceeds its room of " +
                           std::to_string(room_of(l, l->src[w.first])) + " samples");
    if (total == 0) return BN_OK;
    if (total >= 0xffffffffull) return invalid("a push may stage at most 2^32 - 2 samples");
    if (l->rates) {
        bn_status bs = scatter_rates(l, want, n, sources, pcm, n_samples, false);
        if (bs != BN_OK) return bs;
        // windows become ready in array order
        for (size_t i = 0; i < n; i++) {
            if (!n_samples[i]) continue;
            Source &s = l->src[sources[i]];
            s.in_pushed += n_samples[i];
            s.pushed = outputs_of(l, s, s.in_pushed, false);
            make_ready(l, sources[i]);
        }
        return BN_OK;
    }
    // tiles: every chunk split at ring wraps and every LIVE_TILE samples
    std::vector<bn::LiveTile> tiles;
    {
        std::vector<uint64_t> at(want.size());  // ring-absolute write position per touched source
        for (size_t j = 0; j < want.size(); j++) {
            const Source &s = l->src[want[j].first];
            at[j] = s.base + s.pushed;
        }
        uint32_t off = 0;
        for (size_t i = 0; i < n; i++) {
            const size_t j = (size_t)l->touched[sources[i]];
            const uint64_t slot = (uint64_t)sources[i] * l->R;
            size_t left = n_samples[i];
            while (left) {
                const uint64_t pos = at[j] % l->R;
                const uint32_t len = (uint32_t)std::min<uint64_t>({left, l->R - pos, bn::LIVE_TILE});
                tiles.push_back(bn::LiveTile{slot + pos, off, len});
                at[j] += len;
                off += len;
                left -= len;
            }
        }
    }
    const size_t tiles_b = (tiles.size() * sizeof(bn::LiveTile) + 255) / 256 * 256;
    const size_t bytes = tiles_b + total * l->in_esz + bn::PCM_READ_SLACK;
    BN_HIP_TRY(bn::use_device(l->device));
    retire_gathers(l);
    // a staging block is reused only after the scatter that read it completed
    Stage *stp = nullptr;
    {
        bn_status bs = acquire_stage(l, bytes, &stp);
        if (bs != BN_OK) return bs;
    }
    Stage &st = *stp;
    memcpy(st.h, tiles.data(), tiles.size() * sizeof(bn::LiveTile));
    {
        char *p = st.h + tiles_b;
        for (size_t i = 0; i < n; i++) {
            if (!n_samples[i]) continue;
            memcpy(p, pcm[i], n_samples[i] * l->in_esz);
            p += n_samples[i] * l->in_esz;
        }
    }
    // the scatter waits for the gathers that read the ring space it overwrites: positions below (write end - R)
    std::vector<uint64_t> waited;
    for (const auto &w : want) {
        Source &s = l->src[w.first];
        const uint64_t end = s.base + s.pushed + w.second;
        if (end > l->R) {
            bn_status bs = wait_readers(l, s, end - l->R, waited);
            if (bs != BN_OK) return bs;
        }
    }
    bn::clear_launch_state();
    const char *blk = st.h;
    if (l->copy_mode) {
        BN_HIP_TRY(hipMemcpyAsync(st.d, st.h, bytes, hipMemcpyHostToDevice, l->stream));
        blk = st.d;
    }
    bn::launch_live_scatter(l->stream, l->slab, bn::PcmSrc{blk + tiles_b, l->in_layout}, reinterpret_cast<const bn::LiveTile *>(blk),
                            (uint32_t)tiles.size());
    if (bn_status lst = bn::check_launch("live scatter"); lst != BN_OK) return lst;
    BN_HIP_TRY(hipEventRecord(st.ev, l->stream));
    BN_HIP_TRY(hipEventRecord(l->scatter_ev, l->stream));
    st.used = true;
    l->scattered = true;
    l->next_stage = (l->next_stage + 1) % N_STAGE;
    // windows become ready in array order
    for (size_t i = 0; i < n; i++) {
        if (!n_samples[i]) continue;
        l->src[sources[i]].pushed += n_samples[i];
        make_ready(l, sources[i]);
    }
    return BN_OK;
}

// the tables of a resampling pool, one per distinct source rate, the tile size of each, and the device buffers
bn_status setup_rates(bn_live *l, uint32_t dst_rate, const uint32_t *src_rates, uint32_t zero_crossings) {
    std::vector<float> coef;
    std::vector<uint32_t> table_rate;
    uint32_t lds_floats = 1;
    size_t max_T = 2;
    for (int32_t si = 0; si < l->n_sources; si++) {
        Source &s = l->src[(size_t)si];
        s.rate = src_rates[si];
        if (s.rate == dst_rate) continue;
        const auto known = std::find(table_rate.begin(), table_rate.end(), s.rate);
        if (known != table_rate.end()) {
            s.table = (int32_t)(known - table_rate.begin());
            continue;
        }
        const std::string who = "source " + std::to_string(si) + " (" + std::to_string(s.rate) + " -> " + std::to_string(dst_rate) + " Hz)";
        // refuse before the table is built: L * T may be huge for rates without a large common divisor
        const bn::ResampleTable f = bn::resample_factors(s.rate, dst_rate, zero_crossings);
        if (f.T > bn::LIVE_RS_MAX_T || (uint64_t)f.L * f.T > (1ull << 22) || (uint64_t)bn::LIVE_TILE * f.M + f.L >= (1ull << 32))
            return invalid(who + ": the polyphase table (L = " + std::to_string(f.L) + ", M = " + std::to_string(f.M) + ", T = " + std::to_string(f.T) +
                           ") exceeds what a live pool accepts (T <= " + std::to_string(bn::LIVE_RS_MAX_T) + ", L * T <= 2^22, M < 2^20)");
        const bn::ResampleTable rt = bn::make_resample_table(s.rate, dst_rate, zero_crossings);
        bn::LiveRsTable t;
        t.L = rt.L;
        t.M = rt.M;
        t.T = rt.T;
        t.coef_off = (uint32_t)coef.size();
        // span of a tile of n outputs, whatever its phase: ((n - 1) * M + L - 1) / L + T floats
        auto span_of = [&](uint64_t n_out) { return (uint32_t)(((n_out - 1) * t.M + t.L - 1) / t.L + t.T); };
        const uint32_t table_floats = t.L * t.T;
        t.lds_table = table_floats < bn::LIVE_RS_LDS_FLOATS && span_of(1024) <= bn::LIVE_RS_LDS_FLOATS - table_floats;
        const uint32_t avail = bn::LIVE_RS_LDS_FLOATS - (t.lds_table ? table_floats : 0);
        uint32_t tile = bn::LIVE_TILE;
        while (tile > 1 && span_of(tile) > avail) tile = std::min<uint32_t>(tile - 1, (uint32_t)((uint64_t)(avail - t.T) * t.L / t.M + 1));
        t.span_cap = span_of(tile);
        lds_floats = std::max(lds_floats, t.span_cap + (t.lds_table ? table_floats : 0));
        max_T = std::max<size_t>(max_T, t.T);
        coef.insert(coef.end(), rt.coef.begin(), rt.coef.end());
        s.table = (int32_t)l->tables.size();
        l->tables.push_back(t);
        l->table_tile.push_back(tile);
        table_rate.push_back(s.rate);
    }
    l->rates = true;
    l->dst_rate = dst_rate;
    l->lds_bytes = lds_floats * (uint32_t)sizeof(float);
    l->hist_cap = max_T - 1;
    const size_t hist_b = (size_t)l->n_sources * l->hist_cap * sizeof(float);
    BN_HIP_TRY(l->d_hist.alloc(hist_b));
    BN_HIP_TRY(bn::gated::Memset(l->d_hist, 0, hist_b));
    if (!l->tables.empty()) {
        BN_HIP_TRY(l->d_tables.alloc(l->tables.size() * sizeof(bn::LiveRsTable)));
        BN_HIP_TRY(bn::gated::Memcpy(l->d_tables, l->tables.data(), l->tables.size() * sizeof(bn::LiveRsTable), hipMemcpyHostToDevice));
        BN_HIP_TRY(l->d_coef.alloc(coef.size() * sizeof(float)));
        BN_HIP_TRY(bn::gated::Memcpy(l->d_coef, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return BN_OK;
}

// bn_live_create (src_rates == nullptr), bn_live_create_rates and bn_live_create_layout
bn_status create_pool(int32_t device, int32_t n_sources, bn::PcmLayout layout, size_t segment_samples, size_t step_samples, size_t ring_samples,
                      uint32_t dst_rate, const uint32_t *src_rates, uint32_t zero_crossings, bn_live **out) {
    if (!out) return invalid("null argument");
    *out = nullptr;
    if (const char *why = bn::pcm_layout_problem(layout))
        return invalid(std::string(why) + " (format " + std::to_string(layout.format) + ", channels " + std::to_string(layout.channels) + ", channel " +
                       std::to_string(layout.channel) + ")");
    layout = bn::pcm_normalised(layout);
    if (n_sources < 1) return invalid("n_sources must be at least 1");
    if (segment_samples == 0 || segment_samples % 4 != 0) return invalid("segment_samples must be a positive multiple of 4");
    if (step_samples < 1 || step_samples > segment_samples) return invalid("step_samples must be in 1..segment_samples");
    if (ring_samples < segment_samples + step_samples) return invalid("ring_samples must be at least segment_samples + step_samples");
    if (ring_samples >= (1ull << 31)) return invalid("ring_samples must be below 2^31");
    if (src_rates) {
        if (dst_rate == 0) return invalid("dst_rate must be positive");
        for (int32_t s = 0; s < n_sources; s++)
            if (src_rates[s] == 0) return invalid("source " + std::to_string(s) + ": sample rates must be positive");
    }
    if (bn_status dst = bn::require_device(device); dst != BN_OK) return dst;
    BN_HIP_TRY(bn::use_device(device));
    auto l = std::make_unique<bn_live>();
    l->device = device;
    l->n_sources = n_sources;
    l->in_layout = layout;
    l->in_esz = bn::pcm_frame_bytes(layout);
    // the ring stores mono int16 / float pushes as they are; any other layout lands in it as f32, converted by the scatter
    l->format = bn::pcm_is_plain(layout) ? layout.format : BN_PCM_F32;
    l->esz = l->format == BN_PCM_I16 ? sizeof(int16_t) : sizeof(float);
    l->S = segment_samples;
    l->step = step_samples;
    l->R = ring_samples;
    l->copy_mode = bn::sw_is(bn::sw::BN_LIVE_SCATTER, "copy");
    l->src.resize((size_t)n_sources);
    l->touched.assign((size_t)n_sources, -1);
    if (src_rates) {
        // the ring of a resampling pool holds f32 at the model's rate, whatever the sources deliver
        l->format = BN_PCM_F32;
        l->esz = sizeof(float);
        bn_status st = setup_rates(l.get(), dst_rate, src_rates, zero_crossings);
        if (st != BN_OK) return st;
        // a full ring must still hold a ready window: the outputs not yet final plus one source sample's worth stay below
        // ceil((T/2 + 1) * L / M)
        for (size_t i = 0; i < l->tables.size(); i++) {
            const bn::LiveRsTable &t = l->tables[i];
            const uint64_t tail = ceil_muldiv(t.T / 2 + 1, t.L, t.M);
            if (ring_samples < segment_samples + step_samples + tail)
                return invalid("ring_samples must be at least segment_samples + step_samples + " + std::to_string(tail) + " for a source resampled by " +
                               std::to_string(t.L) + "/" + std::to_string(t.M));
        }
    }
    size_t slab_b = 0;
    if (!bn::pcm_ring_bytes((size_t)n_sources, ring_samples, l->esz, &slab_b)) return invalid("n_sources * ring_samples exceeds the address space");
    BN_HIP_TRY(l->stream.create(hipStreamNonBlocking));
    BN_HIP_TRY(l->scatter_ev.create(hipEventDisableTiming));
    for (auto &st : l->stage) BN_HIP_TRY(st.ev.create(hipEventDisableTiming));
    BN_HIP_TRY(l->slab.alloc(slab_b));
    BN_HIP_TRY(bn::gated::Memset(l->slab, 0, slab_b));
    BN_HIP_TRY(l->d_window.alloc(segment_samples * sizeof(float)));
    *out = l.release();
    return BN_OK;
}

}  // namespace

extern "C" {

bn_status bn_live_create(int32_t device, int32_t n_sources, int32_t format, size_t segment_samples, size_t step_samples, size_t ring_samples,
                         bn_live **out) {
    if (out) *out = nullptr;
    if (format != BN_PCM_I16 && format != BN_PCM_F32) return invalid("unknown PCM format " + std::to_string(format));
    return create_pool(device, n_sources, bn::PcmLayout{format, 1, 0}, segment_samples, step_samples, ring_samples, 0, nullptr, 0, out);
}

bn_status bn_live_create_rates(int32_t device, int32_t n_sources, int32_t format, size_t segment_samples, size_t step_samples, size_t ring_samples,
                               uint32_t dst_rate, const uint32_t *src_rates, uint32_t zero_crossings, bn_live **out) {
    if (!src_rates) {
        if (out) *out = nullptr;
        return invalid("null argument");
    }
    if (out) *out = nullptr;
    if (format != BN_PCM_I16 && format != BN_PCM_F32) return invalid("unknown PCM format " + std::to_string(format));
    return create_pool(device, n_sources, bn::PcmLayout{format, 1, 0}, segment_samples, step_samples, ring_samples, dst_rate, src_rates, zero_crossings, out);
}

bn_status bn_live_create_layout(int32_t device, int32_t n_sources, const bn_pcm_layout *layout, size_t struct_size, size_t segment_samples,
                                size_t step_samples, size_t ring_samples, uint32_t dst_rate, const uint32_t *src_rates, uint32_t zero_crossings,
                                bn_live **out) {
    if (!out) return invalid("null argument");
    *out = nullptr;
    bn::PcmLayout pl;
    if (bn_status st = bn::read_pcm_layout(layout, struct_size, &pl); st != BN_OK) return st;
    return create_pool(device, n_sources, pl, segment_samples, step_samples, ring_samples, dst_rate, src_rates, zero_crossings, out);
}

size_t bn_live_resampled_samples(uint32_t src_rate, uint32_t dst_rate, uint32_t zero_crossings, uint64_t pushed, int32_t closed) {
    if (src_rate == 0 || dst_rate == 0) return 0;
    if (src_rate == dst_rate) return (size_t)pushed;
    const bn::ResampleTable f = bn::resample_factors(src_rate, dst_rate, zero_crossings);
    return (size_t)final_outputs(f.L, f.M, f.T, pushed, closed != 0);
}

uint32_t bn_live_source_rate(const bn_live *l, int32_t source) {
    if (!source_ok(l, source) || !l->rates) return 0;
    return l->src[source].rate;
}

void bn_live_free(bn_live *l) { delete l; }

bn_status bn_live_push(bn_live *l, int32_t source, const void *pcm, size_t n_samples) {
    return push_impl(l, 1, &source, &pcm, &n_samples);
}

bn_status bn_live_push_many(bn_live *l, size_t n, const int32_t *sources, const void *const *pcm, const size_t *n_samples) {
    return push_impl(l, n, sources, pcm, n_samples);
}

bn_status bn_live_close(bn_live *l, int32_t source) {
    if (!l) return invalid("null pool");
    if (!source_ok(l, source)) return invalid("source " + std::to_string(source) + " out of range [0, " + std::to_string(l->n_sources) + ")");
    Source &s = l->src[source];
    if (s.closed) return invalid("source " + std::to_string(source) + " is already closed");
    if (l->rates && s.table >= 0) {
        // the tail: outputs whose taps reach past the end, computed with zeros there (room always keeps space for them)
        std::vector<std::pair<int32_t, uint64_t>> want{{source, 0}};
        bn_status bs = scatter_rates(l, want, 0, nullptr, nullptr, nullptr, true);
        if (bs != BN_OK) return bs;
        s.pushed = outputs_of(l, s, s.in_pushed, true);
    }
    s.closed = true;
    make_ready(l, source);
    return BN_OK;
}

bn_status bn_live_reset(bn_live *l, int32_t source) {
    if (!l) return invalid("null pool");
    if (!source_ok(l, source)) return invalid("source " + std::to_string(source) + " out of range [0, " + std::to_string(l->n_sources) + ")");
    Source &s = l->src[source];
    std::deque<std::pair<int32_t, uint64_t>> keep;
    for (const auto &q : l->queue)
        if (q.first != source) keep.push_back(q);
    l->queue.swap(keep);
    s.base += s.pushed;  // in-flight gathers of the old stream stay ordered against the new stream's scatters (s.reads is kept)
    s.pushed = s.n_ready = s.sched = 0;
    s.in_pushed = 0;  // the new stream sees zeros before its sample 0: the kernel never reads history below stream sample 0
    s.closed = false;
    return BN_OK;
}

size_t bn_live_ready(const bn_live *l, int32_t source) {
    if (!l) return 0;
    if (source < 0) return l->queue.size();
    if (!source_ok(l, source)) return 0;
    const Source &s = l->src[source];
    return (size_t)(s.n_ready - s.sched);
}

size_t bn_live_event_count(const bn_live *l) { return l ? l->gathers.size() + l->free_events.size() : 0; }

size_t bn_live_room(const bn_live *l, int32_t source) {
    if (!source_ok(l, source)) return 0;
    return room_of(l, l->src[source]);
}

bn_status bn_live_read_window(const bn_live *lc, int32_t source, uint64_t window, float *host_out) {
    bn_live *l = const_cast<bn_live *>(lc);
    if (!l || !host_out) return invalid("null argument");
    if (!source_ok(l, source)) return invalid("source " + std::to_string(source) + " out of range [0, " + std::to_string(l->n_sources) + ")");
    const Source &s = l->src[source];
    if (window < s.sched || window >= s.n_ready)
        return invalid("window " + std::to_string(window) + " of source " + std::to_string(source) + " is not ready and unscheduled (ready: [" +
                       std::to_string(s.sched) + ", " + std::to_string(s.n_ready) + "))");
    BN_HIP_TRY(bn::use_device(l->device));
    bn::LiveGatherRows rows;
    rows.r[0] = row_of(l, s, window);
    rows.r[0].base = (uint64_t)source * l->R;
    bn::clear_launch_state();
    bn::launch_live_gather(l->stream, l->d_window, l->slab, l->format == BN_PCM_I16, (uint32_t)l->R, (uint32_t)l->S, rows, 1);
    if (bn_status lst = bn::check_launch("live gather"); lst != BN_OK) return lst;
    BN_HIP_TRY(hipStreamSynchronize(l->stream));
    BN_HIP_TRY(bn::gated::Memcpy(host_out, l->d_window, l->S * sizeof(float), hipMemcpyDeviceToHost));
    return BN_OK;
}

bn_status bn_step_live(bn_ctx *c, bn_live *l, size_t max_windows, size_t top_k, int32_t has_min, float min_conf, int32_t *source_out,
                       uint64_t *window_out, size_t *n_out, int32_t sync) {
    if (!c || !l || !n_out || !source_out || !window_out) return invalid("null argument");
    *n_out = 0;
    bn::CtxStepInput ci;
    bn_status st = bn::ctx_step_input(c, top_k, &ci);
    if (st != BN_OK) return st;
    if (max_windows > ci.max_batch) return invalid("max_windows " + std::to_string(max_windows) + " exceeds context max " + std::to_string(ci.max_batch));
    if (ci.device != l->device) return invalid("pool and context live on different devices");
    if (ci.sample_count != l->S)
        return invalid("the context's model takes " + std::to_string(ci.sample_count) + "-sample segments, the pool cuts " + std::to_string(l->S));
    if ((st = bn::ctx_step_check(c, l->src.size(), 0, 0)) != BN_OK) return st;
    const size_t B = std::min(max_windows, l->queue.size());
    if (B == 0) return BN_OK;
    BN_HIP_TRY(bn::use_device(l->device));
    retire_gathers(l);
    // the gather's event first: once the gather is launched, its order against later scatters must not be lost
    bn::Event ev;
    if (!l->free_events.empty()) {
        ev = std::move(l->free_events.back());
        l->free_events.pop_back();
    } else {
        BN_HIP_TRY(ev.create(hipEventDisableTiming));
    }
    const hipError_t we = l->scattered ? hipStreamWaitEvent(ci.stream, l->scatter_ev, 0) : hipSuccess;
    if (we != hipSuccess) {
        l->free_events.push_back(std::move(ev));
        return set_last_error(BN_ERR_BACKEND, std::string("hipStreamWaitEvent failed: ") + hipGetErrorString(we));
    }
    // gather first, bookkeeping after: a launch failure leaves the pool unchanged
    bn::clear_launch_state();
    for (size_t r0 = 0; r0 < B; r0 += bn::LIVE_GATHER_ROWS) {
        const size_t m = std::min<size_t>(bn::LIVE_GATHER_ROWS, B - r0);
        bn::LiveGatherRows rows;
        for (size_t i = 0; i < m; i++) {
            const auto &q = l->queue[r0 + i];
            rows.r[i] = row_of(l, l->src[q.first], q.second);
            rows.r[i].base = (uint64_t)q.first * l->R;
        }
        bn::launch_live_gather(ci.stream, ci.d_input + r0 * l->S, l->slab, l->format == BN_PCM_I16, (uint32_t)l->R, (uint32_t)l->S, rows,
                               (uint32_t)m);
    }
    if (bn_status lst = bn::check_launch("live gather"); lst != BN_OK) {
        l->free_events.push_back(std::move(ev));
        return lst;
    }
    const hipError_t re = hipEventRecord(ev, ci.stream);
    if (re != hipSuccess) {
        (void)hipStreamSynchronize(ci.stream);  // the gather's order is lost: wait for it instead
        l->free_events.push_back(std::move(ev));
    } else {
        const uint64_t id = l->next_gather++;
        l->gathers.push_back(Gather{id, std::move(ev), false});
        int32_t last = -1;
        for (size_t i = 0; i < B; i++) {
            const auto &q = l->queue[i];
            Source &s = l->src[q.first];
            // one read record per (source, gather): the first window of the source in this step has the lowest start
            if (q.first != last && (s.reads.empty() || s.reads.back().second != id)) s.reads.emplace_back(s.base + q.second * l->step, id);
            last = q.first;
        }
    }
    for (size_t i = 0; i < B; i++) {
        const auto &q = l->queue.front();
        source_out[i] = q.first;
        window_out[i] = q.second;
        l->src[q.first].sched = q.second + 1;
        l->queue.pop_front();
    }
    // the windows are taken from here on: on a failure of the step itself *n_out still names them (their results are lost)
    *n_out = B;
    // the prior's and the tracker's rows are these sources and windows (the caller's arrays, read before the step returns)
    return bn::step_device(c, ci.d_input, bn::StepRows{B, true, source_out, window_out, 0}, top_k, has_min, min_conf, sync);
}

}  // extern "C"
