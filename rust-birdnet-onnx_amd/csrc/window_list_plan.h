// The host-side arithmetic of a step over an explicit list of windows (recording.cpp: bn_step_window_list, bn_recording_window_list;
// kernel in levels.hip) that needs neither a device nor the runtime: which frames of its recording a row reads (the `start + S`
// arithmetic, which never forms start + S), the reader kind of a layout, the grouping of a list's rows by reader kind, the cuts of a
// group into launches of at most ROWS_PER_LAUNCH rows, and per recording the last frame any of its rows reads (what an asynchronous
// upload is waited for).  Host code only, so that a stand-alone program can run it under a sanitizer (tools/asan_window_list_plan.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "last_error.h"
#include "pcm_layout.h"

namespace bn {
namespace wlist {

constexpr size_t ROWS_PER_LAUNCH = 128;  // the row descriptors travel as kernel arguments (levels.h, WindowListRows)

// The reader pcm_read.h's pcm_visit picks for a (checked, normalised) layout, as a number: the two mono loads the library always had,
// then the interleaved reader of each format
enum Kind : int { MONO_I16 = 0, MONO_F32 = 1, FRAMES_I16 = 2, FRAMES_F32 = 3, FRAMES_I24 = 4, FRAMES_I32 = 5, FRAMES_U8 = 6, KINDS = 7 };
inline int reader_kind(const PcmLayout &l) {
    if (pcm_is_plain(l)) return l.format == BN_PCM_I16 ? MONO_I16 : MONO_F32;
    switch (l.format) {
        case BN_PCM_I16: return FRAMES_I16;
        case BN_PCM_F32: return FRAMES_F32;
        case BN_PCM_I24: return FRAMES_I24;
        case BN_PCM_I32: return FRAMES_I32;
        case BN_PCM_U8: return FRAMES_U8;
        default: return -1;
    }
}

// frames of the window [start, start + S) that the recording of n frames holds; the rest of the window reads as 0.  start < n is
// the caller's refusal (check_start); start + S is never formed, so a start at the edge of uint64 cannot wrap
inline uint64_t valid_frames(uint64_t start, uint64_t n, uint64_t S) { return start < n ? std::min<uint64_t>(S, n - start) : 0; }
// the last frame the window reads (valid_frames(start, n, S) >= 1)
inline uint64_t last_frame(uint64_t start, uint64_t n, uint64_t S) { return start + (valid_frames(start, n, S) - 1); }
// does the window reach past the last frame?
inline bool padded(uint64_t start, uint64_t n, uint64_t S) { return valid_frames(start, n, S) < S; }

inline bn_status check_start(size_t row, uint64_t start, uint64_t n) {
    if (start >= n)
        return set_last_error(BN_ERR_INVALID_ARG, "row " + std::to_string(row) + ": start " + std::to_string(start) + " is not below the " +
                                                      std::to_string(n) + " frames of its recording");
    return BN_OK;
}

// one row of a list, as the plan sees it: which of the call's distinct recordings it reads, and from where
struct Row {
    uint32_t rec;
    uint64_t start;
};
// one distinct recording of a list
struct Rec {
    PcmLayout layout;
    uint64_t n_samples = 0;
};
// rows order[first .. first + count) in one launch of the kernel instantiated for `kind`
struct Launch {
    int kind;
    size_t first, count;
};
struct Plan {
    std::vector<uint32_t> order;     // the list's positions grouped by reader kind, list order kept inside a group
    std::vector<Launch> launches;    // kinds ascending, each group cut every ROWS_PER_LAUNCH rows
    std::vector<uint64_t> last;      // per recording: the last frame any of its rows reads
    std::vector<uint8_t> used;       // per recording: does any row read it?
};

// The plan of a list.  Refuses (nothing of `out` is to be used then) a row that names no recording of `recs`, a recording whose layout
// no reader knows, a start at or past its recording's end, and a list of 2^32 rows or more (a row's position is a 32-bit batch row)
inline bn_status build(const std::vector<Rec> &recs, const Row *rows, size_t count, uint64_t S, Plan *out) {
    out->order.clear();
    out->launches.clear();
    out->last.assign(recs.size(), 0);
    out->used.assign(recs.size(), 0);
    if (count > 0xffffffffull) return set_last_error(BN_ERR_INVALID_ARG, "a window list holds fewer than 2^32 rows");
    if (S == 0) return set_last_error(BN_ERR_INVALID_ARG, "segment_samples must be positive");
    size_t per_kind[KINDS] = {};
    std::vector<int8_t> kind_of(recs.size());
    for (size_t r = 0; r < recs.size(); r++) {
        const int k = reader_kind(recs[r].layout);
        if (k < 0) return set_last_error(BN_ERR_INVALID_ARG, "unknown PCM format");
        kind_of[r] = (int8_t)k;
    }
    for (size_t i = 0; i < count; i++) {
        if (rows[i].rec >= recs.size()) return set_last_error(BN_ERR_INVALID_ARG, "row " + std::to_string(i) + " names no recording");
        const Rec &rc = recs[rows[i].rec];
        if (bn_status st = check_start(i, rows[i].start, rc.n_samples); st != BN_OK) return st;
        const uint64_t lf = last_frame(rows[i].start, rc.n_samples, S);
        uint64_t &last = out->last[rows[i].rec];
        if (!out->used[rows[i].rec] || lf > last) last = lf;
        out->used[rows[i].rec] = 1;
        per_kind[kind_of[rows[i].rec]]++;
    }
    // a counting sort by kind: stable, so a group keeps the list's order
    size_t at[KINDS];
    size_t total = 0;
    for (int k = 0; k < KINDS; k++) {
        at[k] = total;
        for (size_t done = 0; done < per_kind[k]; done += ROWS_PER_LAUNCH)
            out->launches.push_back(Launch{k, total + done, std::min(ROWS_PER_LAUNCH, per_kind[k] - done)});
        total += per_kind[k];
    }
    out->order.resize(count);
    for (size_t i = 0; i < count; i++) out->order[at[kind_of[rows[i].rec]]++] = (uint32_t)i;
    return BN_OK;
}

}  // namespace wlist
}  // namespace bn
