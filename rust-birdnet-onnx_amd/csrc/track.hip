// Detection events on the device (include/birdnet_hip.h, bn_track_*): per-source species tracking across windows.
//
// State: six planes [field][source][species] of 32-bit words (hits, first, last, peak window, peak confidence, sum), so every
// access of a wave is coalesced.  hits == 0 means no open event; the other planes of such a record are never read.
//
// track_update_kernel: blocks of 256 lanes, grid (species / 256, groups).  A group is one source of the update with its rows in
// increasing window order; the host builds the groups (rows of one source need not be adjacent in a live step) and the kernel
// reads the lists in place from pinned memory.  One lane owns one (source, species) for the whole update:
//   1  the hits plane first; a lane with no open event and no hit touches nothing else (nearly every lane of every step)
//   2  the source's rows in order: logits[row][j] coalesced across j, sigmoid_ref, the prior's rules under BN_TRACK_PRIOR, the
//      state machine of the contract on the record in registers
//   3  a closed event with hits >= min_hits is emitted: wave64 ballot + prefix count, ONE integer atomicAdd per wave on the
//      update's counter reserves the wave's slots; events past the capacity are counted, not written
//   4  the record is written back once, and only the planes that changed: hits when it differs from what was read; last and sum
//      after a hit; first when an event opened; peak and peak window when the peak moved (or an event opened)
// bn_track_flush is the same body with no rows and a "close everything" flag.  track_finish_kernel then hands the counter to the
// host (pinned) and zeroes it for the next update; updates of one tracker are serialised by its event, so one counter serves all.
// No floating-point atomics: a record's sum is added by its own lane in window order.  The events reach pinned memory in the order
// the slots were reserved, which depends on scheduling; the host sorts them by (source, species, first window) when they are read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "hip_gate.h"
#include "kernels.h"
#include "prior_rules.h"
#include "sigmoid_ref.h"

namespace bn {
namespace {

constexpr int TT = 256;               // lanes per block
constexpr uint32_t MAX_GROUPS_Y = 65535;  // groups per launch (grid.y)
enum Plane { P_HITS = 0, P_FIRST, P_LAST, P_PEAKW, P_PEAK, P_SUM, N_PLANES };

struct TrackArgs {
    const float *logits;  // [rows, n]
    uint32_t *state;      // [N_PLANES][n_sources][n]
    // pinned, read in place
    const int32_t *grp_source;  // [groups]
    const uint32_t *grp_off;    // [groups + 1] into the row lists
    const uint32_t *row_idx;    // the row of the logits block
    const uint32_t *row_win;
    const int32_t *row_site;  // under use_prior
    const float *table;       // the prior's [n_sites, tstride]
    bn_event *events;         // [cap], pinned
    uint32_t *counter;        // device: events closed with hits >= min_hits in this update
    int64_t n, plane, tstride;
    uint32_t n_sources, n_sites, g0, cap, min_hits, max_gap;
    int32_t use_prior, rerank, close_all;
    float enter, thr;
};

__global__ __launch_bounds__(TT) void track_update_kernel(TrackArgs a) {
    const uint32_t g = a.g0 + blockIdx.y;
    const uint32_t s = (uint32_t)a.grp_source[g];
    if (s >= a.n_sources) return;  // block-uniform; the host has checked every source: never touch state outside the planes
    const uint32_t r0 = a.grp_off[g], r1 = a.grp_off[g + 1];
    const int64_t j = (int64_t)blockIdx.x * TT + threadIdx.x;
    const bool valid = j < a.n;  // lanes past the row stay in the loop: the ballots below need whole waves
    const int64_t at = (int64_t)s * a.n + j;
    const uint32_t lane = threadIdx.x & 63u;

    uint32_t hits = valid ? a.state[P_HITS * a.plane + at] : 0u;
    const uint32_t hits_in = hits;
    uint32_t first = 0, last = 0, peakw = 0;
    float peak = 0.f, sum = 0.f;
    bool loaded = false;
    bool w_hit = false, w_first = false, w_peak = false;  // planes to write back: last + sum / first / peak + peak window

    for (uint32_t r = r0; r <= r1; r++) {  // the iteration r == r1 closes what a flush closes and emits nothing else
        const bool tail = r == r1;
        if (tail && !a.close_all) break;  // block-uniform
        bool hit = false;
        float conf = 0.f;
        uint32_t k = 0;
        if (!tail) {
            k = a.row_win[r];
            if (valid) {
                conf = sigmoid_ref(a.logits[(int64_t)a.row_idx[r] * a.n + j]);
                bool adm = true;
                if (a.use_prior) {
                    uint32_t site = (uint32_t)a.row_site[r];
                    if (site >= a.n_sites) site = 0;  // the host has checked every id; never read outside the table
                    const float p = a.table[(int64_t)site * a.tstride + j];
                    adm = admitted(p, a.thr);
                    conf = prior_conf(conf, p, a.rerank);
                }
                hit = adm && conf >= a.enter;
            }
        }
        bool emit = false;
        bn_event e{};
        if (hits > 0) {
            if (!loaded) {
                first = a.state[P_FIRST * a.plane + at];
                last = a.state[P_LAST * a.plane + at];
                peakw = a.state[P_PEAKW * a.plane + at];
                peak = __uint_as_float(a.state[P_PEAK * a.plane + at]);
                sum = __uint_as_float(a.state[P_SUM * a.plane + at]);
                loaded = true;
            }
            const bool close = tail || (k - last - 1u) + (hit ? 0u : 1u) > a.max_gap;
            if (close) {
                if (hits >= a.min_hits) {
                    emit = true;
                    e.source = (int32_t)s;
                    e.species = (uint32_t)j;
                    e.first_window = first;
                    e.last_window = last;
                    e.hits = hits;
                    e.peak_window = peakw;
                    e.peak_conf = peak;
                    e.mean_conf = sum / (float)hits;
                }
                hits = 0;
            }
        }
        if (hit) {
            if (hits == 0) {
                first = k;
                sum = 0.f;
                peak = conf;
                peakw = k;
                loaded = true;  // the record is this lane's from here on
                w_first = w_peak = true;
            }
            last = k;
            hits += 1;
            sum += conf;
            if (conf > peak) {
                peak = conf;
                peakw = k;
                w_peak = true;
            }
            w_hit = true;
        }
        // every lane of the wave is here: r and the loop's exits are block-uniform
        const uint64_t mask = __ballot(emit);
        if (mask) {
            const uint32_t cnt = (uint32_t)__popcll(mask);
            const int leader = __ffsll((unsigned long long)mask) - 1;
            uint32_t base = 0;
            if ((int)lane == leader) base = atomicAdd(a.counter, cnt);
            base = __shfl(base, leader);
            if (emit) {
                const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (slot < a.cap) a.events[slot] = e;
            }
        }
    }
    if (!valid) return;
    if (hits != hits_in) a.state[P_HITS * a.plane + at] = hits;
    if (hits == 0) return;  // no open event: the other planes of the record are never read
    if (w_hit) {
        a.state[P_LAST * a.plane + at] = last;
        a.state[P_SUM * a.plane + at] = __float_as_uint(sum);
    }
    if (w_first) a.state[P_FIRST * a.plane + at] = first;
    if (w_peak) {
        a.state[P_PEAKW * a.plane + at] = peakw;
        a.state[P_PEAK * a.plane + at] = __float_as_uint(peak);
    }
}

// the update's count to the host, the counter back to zero for the next update
__global__ void track_finish_kernel(uint32_t *counter, uint32_t *h_total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        *h_total = *counter;
        *counter = 0u;
    }
}

// One update's lists and results in ONE pinned block: [grp_source: groups][grp_off: groups + 1][row_idx, row_win, row_site: rows each]
// [total: 4 words][events: cap]
struct Stage {
    void *base = nullptr;
    size_t rows = 0, groups = 0, cap = 0;
    int32_t *grp_source = nullptr;
    uint32_t *grp_off = nullptr, *row_idx = nullptr, *row_win = nullptr;
    int32_t *row_site = nullptr;
    uint32_t *total = nullptr;
    bn_event *events = nullptr;

    static size_t words(size_t rows, size_t groups) { return (2 * groups + 1 + 3 * rows + 4 + 7) / 8 * 8; }  // events 32-byte aligned
    static size_t bytes(size_t rows, size_t groups, size_t cap) { return words(rows, groups) * sizeof(uint32_t) + cap * sizeof(bn_event); }
    void carve(void *b, size_t rows_, size_t groups_, size_t cap_) {
        base = b, rows = rows_, groups = groups_, cap = cap_;
        uint32_t *w = static_cast<uint32_t *>(b);
        grp_source = reinterpret_cast<int32_t *>(w);
        grp_off = w + groups;
        row_idx = grp_off + groups + 1;
        row_win = row_idx + rows;
        row_site = reinterpret_cast<int32_t *>(row_win + rows);
        total = row_win + 2 * rows;
        events = reinterpret_cast<bn_event *>(w + words(rows, groups));
    }
};

bool event_less(const bn_event &x, const bn_event &y) {
    if (x.source != y.source) return x.source < y.source;
    if (x.species != y.species) return x.species < y.species;
    return x.first_window < y.first_window;
}

}  // namespace
}  // namespace bn

static_assert(sizeof(bn_event) == 32, "bn_event is eight 32-bit words");

struct bn_track {
    std::atomic<int> refs{1};  // the caller's handle + one per context that attached it
    int device = 0;
    size_t n_sources = 0, n_species = 0, max_events = 0;
    float enter_conf = 0.f;
    uint32_t min_hits = 1, max_gap = 0, flags = 0;
    bn::Stream stream;                  // bn_track_update_host / flush / reset / open_events
    bn::Event last_ev;                  // recorded behind every update's kernels, on whatever stream ran them
    bn::DeviceBuf<uint32_t> d_state;    // [N_PLANES][n_sources][n_species]  (after stream and event: they go last, device_mem.h)
    bn::DeviceBuf<uint32_t> d_counter;  // one word, zero between updates
    std::vector<int64_t> last_window;   // per source; -1: none since creation / reset
    bool updated = false;               // last_ev has been recorded
    std::mutex mu;
    ~bn_track() {
        (void)bn::use_device(device);
        if (updated) (void)hipEventSynchronize(last_ev);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

struct bn::TrackAttach {
    bn_track *track = nullptr;
    size_t max_batch = 0;
    int32_t source = 0;
    bn::PinnedRing ring;  // a step's lists and events, read and written by the kernels in place
    bn::Stage stage[bn::PinnedRing::SLOTS];  // the ring's blocks, carved
    // the last tracked step
    int res_slot = -1;   // -1: none since the attach; -2: a step whose rows were all stale (no launch)
    bool res_sorted = false;
    size_t res_stale = 0;
    std::vector<int32_t> order;  // scratch of the grouping
    ~TrackAttach();              // drops the reference
};

namespace {

using bn::set_last_error;
using bn::Stage;

constexpr uint32_t KNOWN_FLAGS = BN_TRACK_PRIOR;
constexpr uint64_t WINDOW_LIMIT = 1ull << 31;

void track_unref(bn_track *t) {
    if (t && t->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete t;
}

bn_status check_source(const bn_track *t, int64_t source, const char *what) {
    if (source < 0 || (uint64_t)source >= t->n_sources)
        return set_last_error(BN_ERR_INVALID_ARG, std::string(what) + " " + std::to_string(source) + " is outside 0.." + std::to_string(t->n_sources));
    return BN_OK;
}

// the prior an update runs under: refusals of BN_TRACK_PRIOR's needs, *use = whether the kernel consults a table
bn_status check_prior(const bn_track *t, const bn_prior *prior, bn::PriorView *pv, bool *use) {
    *use = (t->flags & BN_TRACK_PRIOR) != 0;
    if (!*use) return BN_OK;
    if (!prior) return set_last_error(BN_ERR_INVALID_ARG, "the tracker was created with BN_TRACK_PRIOR: an update needs a prior, passed or attached to the context");
    *pv = bn::prior_view(prior);
    if (pv->device != t->device)
        return set_last_error(BN_ERR_INVALID_ARG, "the tracker lives on device " + std::to_string(t->device) + ", the prior on " + std::to_string(pv->device));
    if (pv->n_species != t->n_species)
        return set_last_error(BN_ERR_INVALID_ARG, "the tracker has " + std::to_string(t->n_species) + " species, the prior " + std::to_string(pv->n_species));
    return BN_OK;
}

// Groups `rows` rows by source into st (stable: a source's rows keep their order) and returns the number of groups.  skip[i] != 0
// leaves row i out.  order: scratch.
size_t build_groups(Stage &st, const int32_t *sources, const uint64_t *windows, const int32_t *sites, const uint8_t *skip, size_t rows,
                    std::vector<int32_t> &order) {
    order.clear();
    for (size_t i = 0; i < rows; i++)
        if (!skip || !skip[i]) order.push_back((int32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return sources[x] < sources[y]; });
    size_t groups = 0;
    for (size_t q = 0; q < order.size(); q++) {
        const int32_t i = order[q];
        if (q == 0 || sources[i] != sources[order[q - 1]]) {
            st.grp_source[groups] = sources[i];
            st.grp_off[groups] = (uint32_t)q;
            groups++;
        }
        st.row_idx[q] = (uint32_t)i;
        st.row_win[q] = (uint32_t)windows[i];
        st.row_site[q] = sites ? sites[i] : 0;
    }
    st.grp_off[groups] = (uint32_t)order.size();
    return groups;
}

// the update kernel over st's first `groups` groups + the finish kernel, on `stream`, in the tracker's update order
bn_status enqueue_update(bn_track *t, hipStream_t stream, const float *d_logits, const Stage &st, size_t groups, const bn::PriorView *pv, bool close_all) {
    void *dp = nullptr;
    BN_HIP_TRY(hipHostGetDevicePointer(&dp, st.base, 0));
    Stage d = st;  // the same layout at the block's device address
    d.carve(dp, st.rows, st.groups, st.cap);
    if (t->updated) BN_HIP_TRY(hipStreamWaitEvent(stream, t->last_ev, 0));
    bn::TrackArgs a{};
    a.logits = d_logits;
    a.state = t->d_state;
    a.grp_source = d.grp_source;
    a.grp_off = d.grp_off;
    a.row_idx = d.row_idx;
    a.row_win = d.row_win;
    a.row_site = d.row_site;
    a.events = d.events;
    a.counter = t->d_counter;
    a.n = (int64_t)t->n_species;
    a.plane = (int64_t)(t->n_sources * t->n_species);
    a.n_sources = (uint32_t)t->n_sources;
    a.cap = (uint32_t)st.cap;
    a.min_hits = t->min_hits;
    a.max_gap = t->max_gap;
    a.close_all = close_all ? 1 : 0;
    a.enter = t->enter_conf;
    if (pv) {
        a.use_prior = 1;
        a.table = pv->d_table;
        a.tstride = (int64_t)pv->tstride;
        a.n_sites = (uint32_t)pv->n_sites;
        a.rerank = pv->rerank;
        a.thr = pv->threshold;
    }
    bn::clear_launch_state();
    const unsigned gx = (unsigned)((t->n_species + bn::TT - 1) / bn::TT);
    for (size_t g0 = 0; g0 < groups; g0 += bn::MAX_GROUPS_Y) {
        a.g0 = (uint32_t)g0;
        const unsigned gy = (unsigned)std::min<size_t>(bn::MAX_GROUPS_Y, groups - g0);
        hipLaunchKernelGGL(bn::track_update_kernel, dim3(gx, gy), dim3(bn::TT), 0, stream, a);
    }
    hipLaunchKernelGGL(bn::track_finish_kernel, dim3(1), dim3(64), 0, stream, t->d_counter, d.total);
    bn_status st_l = bn::check_launch("tracker update");
    // the event even after a failed launch: whatever did reach the stream stays ordered against the next update
    const hipError_t re = hipEventRecord(t->last_ev, stream);
    if (re == hipSuccess) t->updated = true;
    if (st_l != BN_OK) return st_l;
    BN_HIP_TRY(re);
    return BN_OK;
}

// a completed update's events, sorted in place; *n kept, *dropped lost to the capacity
void read_events(const Stage &st, bool *sorted, size_t *n, size_t *dropped) {
    const size_t total = *st.total, kept = std::min(total, st.cap);
    if (!*sorted) {
        std::sort(st.events, st.events + kept, bn::event_less);
        *sorted = true;
    }
    *n = kept;
    *dropped = total - kept;
}

// the synchronous tail of bn_track_update_host / bn_track_flush: wait, sort, hand the first `cap` events to the caller
bn_status collect(bn_track *t, const Stage &st, bn_event *events_out, size_t cap, size_t *n_out, size_t *dropped) {
    BN_HIP_TRY(hipStreamSynchronize(t->stream));
    bool sorted = false;
    size_t n = 0, lost = 0;
    read_events(st, &sorted, &n, &lost);
    const size_t m = std::min(n, cap);
    if (m) memcpy(events_out, st.events, m * sizeof(bn_event));
    if (n_out) *n_out = m;
    if (dropped) *dropped = lost + (n - m);
    return BN_OK;
}

}  // namespace

bn_status bn::track_attach(bn_track *t, int device, size_t num_species, size_t max_batch, TrackAttach **out) {
    if (!t || !out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (num_species != t->n_species)
        return set_last_error(BN_ERR_INVALID_ARG, "the tracker has " + std::to_string(t->n_species) + " species, the model " + std::to_string(num_species));
    if (device != t->device)
        return set_last_error(BN_ERR_INVALID_ARG, "the context lives on device " + std::to_string(device) + ", the tracker on " + std::to_string(t->device));
    BN_HIP_TRY(bn::use_device(device));
    auto a = std::make_unique<TrackAttach>();
    a->max_batch = max_batch;
    const size_t rows = std::max<size_t>(max_batch, 1);
    BN_HIP_TRY(a->ring.create(Stage::bytes(rows, rows, t->max_events)));
    for (int i = 0; i < PinnedRing::SLOTS; i++) a->stage[i].carve(a->ring.h[i], rows, rows, t->max_events);
    t->refs.fetch_add(1, std::memory_order_relaxed);
    a->track = t;
    *out = a.release();
    return BN_OK;
}

bn::TrackAttach::~TrackAttach() { track_unref(track); }
void bn::track_detach(TrackAttach *a) { delete a; }

bn_status bn::track_set_source(TrackAttach *a, int32_t source) {
    bn_status st = check_source(a->track, source, "source");
    if (st != BN_OK) return st;
    a->source = source;
    return BN_OK;
}

bn_status bn::track_step_check(const TrackAttach *a, const PriorAttach *prior, size_t n_sources, uint64_t first_window, size_t count) {
    const bn_track *t = a->track;
    PriorView pv{};
    bool use = false;
    bn_status st = check_prior(t, bn::prior_of(prior), &pv, &use);
    if (st != BN_OK) return st;
    if (n_sources > t->n_sources)
        return set_last_error(BN_ERR_INVALID_ARG, "the pool has " + std::to_string(n_sources) + " sources, the attached tracker " + std::to_string(t->n_sources));
    if (count) {
        if (first_window + count > WINDOW_LIMIT) return set_last_error(BN_ERR_INVALID_ARG, "a tracked window number must be below 2^31");
        const int64_t last = t->last_window[(size_t)a->source];
        if ((int64_t)first_window <= last)
            return set_last_error(BN_ERR_INVALID_ARG, "window " + std::to_string(first_window) + " does not exceed the last tracked window " + std::to_string(last) +
                                                          " of source " + std::to_string(a->source));
    }
    return BN_OK;
}

bn_status bn::track_step(TrackAttach *a, hipStream_t stream, const float *d_logits, const StepRows &rows, const PriorAttach *prior) {
    bn_track *t = a->track;
    const size_t batch = rows.batch;
    const int32_t *sources = rows.sources;
    std::lock_guard<std::mutex> lk(t->mu);
    if (batch > a->max_batch) return set_last_error(BN_ERR_INVALID_ARG, "batch exceeds the context's max_batch");
    PriorView pv{};
    bool use = false;
    bn_status st = check_prior(t, bn::prior_of(prior), &pv, &use);
    if (st != BN_OK) return st;
    // the rows as (source, window, site); a live row at or below its source's last window is stale
    std::vector<int32_t> src(batch), site(batch, 0);
    std::vector<uint64_t> win(batch);
    std::vector<uint8_t> skip(batch, 0);
    // (source, its last window before this row): whatever keeps the update from being enqueued takes the rows back, so that the
    // tracker's last windows never name a window it has not seen
    std::vector<std::pair<int32_t, int64_t>> undo;
    auto take_back = [&] {
        for (auto it = undo.rbegin(); it != undo.rend(); ++it) t->last_window[(size_t)it->first] = it->second;
    };
    size_t stale = 0;
    for (size_t i = 0; i < batch; i++) {
        src[i] = sources ? sources[i] : a->source;
        win[i] = rows.windows ? rows.windows[i] : rows.first_window + i;
        if ((st = check_source(t, src[i], "the source of a row,")) != BN_OK || win[i] >= WINDOW_LIMIT) {
            take_back();
            return st != BN_OK ? st : set_last_error(BN_ERR_INVALID_ARG, "a tracked window number must be below 2^31");
        }
        if (use) site[i] = bn::prior_site_of(prior, sources ? src[i] : -1);
        int64_t &last = t->last_window[(size_t)src[i]];
        if ((int64_t)win[i] <= last) {
            skip[i] = 1;
            stale++;
            continue;
        }
        undo.emplace_back(src[i], last);
        last = (int64_t)win[i];
    }
    a->res_stale = stale;
    if (stale == batch) {
        a->res_slot = -2;
        return BN_OK;
    }
    int slot = 0;
    void *block = nullptr;
    hipError_t we = a->ring.acquire(&slot, &block);
    if (we == hipSuccess) {
        Stage &sg = a->stage[slot];
        const size_t groups = build_groups(sg, src.data(), win.data(), site.data(), skip.data(), batch, a->order);
        *sg.total = 0;
        st = enqueue_update(t, stream, d_logits, sg, groups, use ? &pv : nullptr, false);
        if (st == BN_OK) we = a->ring.commit(slot, stream);
    }
    if (we != hipSuccess || st != BN_OK) {
        take_back();
        a->res_slot = -1;
        if (st != BN_OK) return st;
        return set_last_error(BN_ERR_BACKEND, std::string("tracker step: ") + hipGetErrorString(we));
    }
    a->res_slot = slot;
    a->res_sorted = false;
    return BN_OK;
}

bn_status bn::track_step_results(TrackAttach *a, const bn_event **events, size_t *n, size_t *dropped, size_t *stale_rows) {
    if (!a || a->res_slot == -1) return set_last_error(BN_ERR_INVALID_ARG, "no tracked step has run on this context since a tracker was attached");
    size_t kept = 0, lost = 0;
    const bn_event *ev = nullptr;
    if (a->res_slot >= 0) {
        const Stage &sg = a->stage[a->res_slot];
        read_events(sg, &a->res_sorted, &kept, &lost);
        ev = sg.events;
    }
    if (events) *events = ev;
    if (n) *n = kept;
    if (dropped) *dropped = lost;
    if (stale_rows) *stale_rows = a->res_stale;
    return BN_OK;
}

extern "C" {

bn_status bn_track_create(int32_t device, size_t n_sources, size_t n_species, float enter_conf, uint32_t min_hits, uint32_t max_gap, size_t max_events,
                          uint32_t flags, bn_track **out) {
    if (!out) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    *out = nullptr;
    if (n_sources == 0 || n_species == 0 || max_events == 0)
        return set_last_error(BN_ERR_INVALID_ARG, "a tracker needs at least one source, one species and room for one event");
    if (n_sources > 0x7fffffffu || n_species > 0x7fffffffu || max_events > 0x7fffffffu)
        return set_last_error(BN_ERR_INVALID_ARG, "n_sources, n_species and max_events must be below 2^31");
    if (!std::isfinite(enter_conf)) return set_last_error(BN_ERR_INVALID_ARG, "enter_conf must be finite");
    if (min_hits == 0) return set_last_error(BN_ERR_INVALID_ARG, "min_hits must be at least 1");
    if (max_gap >= WINDOW_LIMIT) return set_last_error(BN_ERR_INVALID_ARG, "max_gap must be below 2^31");
    if (flags & ~KNOWN_FLAGS) return set_last_error(BN_ERR_INVALID_ARG, "unknown flag bits " + std::to_string(flags & ~KNOWN_FLAGS));
    if (bn_status dst = bn::require_device(device); dst != BN_OK) return dst;
    BN_HIP_TRY(bn::use_device(device));
    if (!bn::prepare_device(device)) return set_last_error(BN_ERR_BACKEND, "device " + std::to_string(device) + " could not be prepared for the library's kernels");
    auto t = std::make_unique<bn_track>();
    t->device = device;
    t->n_sources = n_sources;
    t->n_species = n_species;
    t->max_events = max_events;
    t->enter_conf = enter_conf;
    t->min_hits = min_hits;
    t->max_gap = max_gap;
    t->flags = flags;
    t->last_window.assign(n_sources, -1);
    const size_t state_b = (size_t)bn::N_PLANES * n_sources * n_species * sizeof(uint32_t);
    BN_HIP_TRY(t->stream.create(hipStreamNonBlocking));
    BN_HIP_TRY(t->last_ev.create(hipEventDisableTiming));
    BN_HIP_TRY(t->d_state.alloc(state_b));
    BN_HIP_TRY(t->d_counter.alloc(sizeof(uint32_t)));
    BN_HIP_TRY(hipMemsetAsync(t->d_state, 0, state_b, t->stream));
    BN_HIP_TRY(hipMemsetAsync(t->d_counter, 0, sizeof(uint32_t), t->stream));
    BN_HIP_TRY(hipStreamSynchronize(t->stream));
    *out = t.release();
    return BN_OK;
}

void bn_track_free(bn_track *t) { track_unref(t); }

size_t bn_track_sources(const bn_track *t) { return t ? t->n_sources : 0; }
size_t bn_track_species(const bn_track *t) { return t ? t->n_species : 0; }

size_t bn_track_open_events(const bn_track *tc, int32_t source) {
    bn_track *t = const_cast<bn_track *>(tc);
    if (!t || source < -1 || (source >= 0 && (size_t)source >= t->n_sources)) return 0;
    std::lock_guard<std::mutex> lk(t->mu);
    if (bn::use_device(t->device) != hipSuccess) return 0;
    if (t->updated && hipEventSynchronize(t->last_ev) != hipSuccess) return 0;
    const size_t first = source < 0 ? 0 : (size_t)source * t->n_species, count = source < 0 ? t->n_sources * t->n_species : t->n_species;
    std::vector<uint32_t> hits(count);
    if (bn::gated::Memcpy(hits.data(), t->d_state + first, count * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    size_t open = 0;
    for (uint32_t h : hits) open += h ? 1 : 0;
    return open;
}

bn_status bn_track_update_host(bn_track *t, const float *logits, size_t rows, const int32_t *sources, const uint64_t *windows, const bn_prior *prior,
                               const int32_t *sites, bn_event *events_out, size_t cap, size_t *n_out, size_t *dropped) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!t) return set_last_error(BN_ERR_INVALID_ARG, "null tracker");
    if (n_out) *n_out = 0;
    if (dropped) *dropped = 0;
    if (rows == 0) return BN_OK;
    if (!logits || !sources || !windows || !n_out || (cap && !events_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (rows > 0x7fffffffu) return set_last_error(BN_ERR_INVALID_ARG, "an update takes fewer than 2^31 rows");
    bn::PriorView pv{};
    bool use = false;
    bn_status st = check_prior(t, prior, &pv, &use);
    if (st != BN_OK) return st;
    if (use && !sites) return set_last_error(BN_ERR_INVALID_ARG, "null sites under BN_TRACK_PRIOR");
    std::lock_guard<std::mutex> lk(t->mu);
    // every refusal before anything changes: the windows of a source must increase, from its last on
    std::vector<int64_t> last(t->last_window);
    for (size_t r = 0; r < rows; r++) {
        if ((st = check_source(t, sources[r], "the source of a row,")) != BN_OK) return st;
        if (windows[r] >= WINDOW_LIMIT) return set_last_error(BN_ERR_INVALID_ARG, "window numbers must be below 2^31");
        if (use && (sites[r] < 0 || (size_t)sites[r] >= pv.n_sites))
            return set_last_error(BN_ERR_INVALID_ARG, "the site of a row, " + std::to_string(sites[r]) + ", is outside 0.." + std::to_string(pv.n_sites));
        int64_t &l = last[(size_t)sources[r]];
        if ((int64_t)windows[r] <= l)
            return set_last_error(BN_ERR_INVALID_ARG, "row " + std::to_string(r) + ": window " + std::to_string(windows[r]) + " of source " +
                                                          std::to_string(sources[r]) + " does not exceed the source's last window " + std::to_string(l));
        l = (int64_t)windows[r];
    }
    BN_HIP_TRY(bn::use_device(t->device));
    bn::Scratch bufs;
    bufs.stream = t->stream;  // the tracker's own: waited for, not destroyed
    float *d_logits = nullptr;
    BN_HIP_TRY(bufs.alloc(&d_logits, rows * t->n_species * sizeof(float)));
    BN_HIP_TRY(bufs.pinned.alloc(Stage::bytes(rows, rows, t->max_events)));
    Stage sg;
    sg.carve(bufs.pinned, rows, rows, t->max_events);
    BN_HIP_TRY(bn::gated::Memcpy(d_logits, logits, rows * t->n_species * sizeof(float), hipMemcpyHostToDevice));
    std::vector<int32_t> order;
    const size_t groups = build_groups(sg, sources, windows, use ? sites : nullptr, nullptr, rows, order);
    *sg.total = 0;
    t->last_window.swap(last);  // the rows are taken from here on
    if ((st = enqueue_update(t, t->stream, d_logits, sg, groups, use ? &pv : nullptr, false)) != BN_OK) return st;
    return collect(t, sg, events_out, cap, n_out, dropped);
}

bn_status bn_track_flush(bn_track *t, int32_t source, bn_event *events_out, size_t cap, size_t *n_out, size_t *dropped) {
    if (bn_status dst = bn::require_any_device(); dst != BN_OK) return dst;
    if (!t) return set_last_error(BN_ERR_INVALID_ARG, "null tracker");
    if (n_out) *n_out = 0;
    if (dropped) *dropped = 0;
    if (!n_out || (cap && !events_out)) return set_last_error(BN_ERR_INVALID_ARG, "null argument");
    if (source != -1)
        if (bn_status st = check_source(t, source, "source"); st != BN_OK) return st;
    std::lock_guard<std::mutex> lk(t->mu);
    BN_HIP_TRY(bn::use_device(t->device));
    const size_t groups = source < 0 ? t->n_sources : 1;
    bn::Scratch bufs;
    bufs.stream = t->stream;
    BN_HIP_TRY(bufs.pinned.alloc(Stage::bytes(1, groups, t->max_events)));
    Stage sg;
    sg.carve(bufs.pinned, 1, groups, t->max_events);
    for (size_t g = 0; g < groups; g++) {  // no rows: every group closes what it has open
        sg.grp_source[g] = source < 0 ? (int32_t)g : source;
        sg.grp_off[g] = 0;
    }
    sg.grp_off[groups] = 0;
    *sg.total = 0;
    if (bn_status st = enqueue_update(t, t->stream, nullptr, sg, groups, nullptr, true); st != BN_OK) return st;
    return collect(t, sg, events_out, cap, n_out, dropped);
}

bn_status bn_track_reset(bn_track *t, int32_t source) {
    if (!t) return set_last_error(BN_ERR_INVALID_ARG, "null tracker");
    if (bn_status st = check_source(t, source, "source"); st != BN_OK) return st;
    std::lock_guard<std::mutex> lk(t->mu);
    BN_HIP_TRY(bn::use_device(t->device));
    // behind every update enqueued so far, and complete on return: a later update on any stream sees the source empty
    if (t->updated) BN_HIP_TRY(hipStreamWaitEvent(t->stream, t->last_ev, 0));
    BN_HIP_TRY(hipMemsetAsync(t->d_state + (size_t)source * t->n_species, 0, t->n_species * sizeof(uint32_t), t->stream));
    BN_HIP_TRY(hipStreamSynchronize(t->stream));
    t->last_window[(size_t)source] = -1;
    return BN_OK;
}

}  // extern "C"
