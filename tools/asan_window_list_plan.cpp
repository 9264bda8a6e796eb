// Host-side sanitizer check of the window list's arithmetic (no device, no Python): which frames of its recording a row reads, computed
// without ever forming start + S, the reader kind of a layout, the grouping of a list's rows by reader kind, the cuts of a group into
// launches of at most 128 rows and, per recording, the last frame any of its rows reads
// (rust-birdnet-onnx_amd/csrc/window_list_plan.h), over edge values and mixed lists.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_window_list_plan.cpp -o /tmp/asan_window_list_plan && /tmp/asan_window_list_plan
// Exit 0 and "asan_window_list_plan: ok": every refusal came with its message; every list position appears in exactly one launch, in a
// launch of its recording's reader kind, list order kept inside a kind; no launch holds more than 128 rows and none but the last of a
// kind fewer; the last frame of a recording is the largest its rows read and lies inside it; nothing read memory it does not own and
// no arithmetic overflowed.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "window_list_plan.h"

static std::string g_last;
// the library's definition lives in capi.cpp, which needs the runtime
bn_status bn::set_last_error(bn_status st, const std::string &msg) {
    g_last = msg;
    return st;
}

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) failures++, fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } while (0)

static bool refused(bn_status st, const char *word) { return st == BN_ERR_INVALID_ARG && g_last.find(word) != std::string::npos; }

using namespace bn;
using namespace bn::wlist;

// every property of a plan that build() accepted
static void check_plan(const std::vector<Rec> &recs, const std::vector<Row> &rows, uint64_t S, const Plan &p) {
    const size_t n = rows.size();
    EXPECT(p.order.size() == n && p.last.size() == recs.size() && p.used.size() == recs.size());
    std::vector<int> hits(n, 0);
    size_t covered = 0;
    int prev_kind = -1;
    for (size_t l = 0; l < p.launches.size(); l++) {
        const Launch &ln = p.launches[l];
        EXPECT(ln.count >= 1 && ln.count <= ROWS_PER_LAUNCH && ln.first == covered && ln.first + ln.count <= n);
        EXPECT(ln.kind >= prev_kind && ln.kind >= 0 && ln.kind < KINDS);
        // only the last launch of a kind may be short
        if (l + 1 < p.launches.size() && p.launches[l + 1].kind == ln.kind) EXPECT(ln.count == ROWS_PER_LAUNCH);
        for (size_t j = 0; j < ln.count && ln.first + j < p.order.size(); j++) {
            const uint32_t i = p.order[ln.first + j];
            EXPECT(i < n);
            if (i >= n) continue;
            hits[i]++;
            EXPECT(reader_kind(recs[rows[i].rec].layout) == ln.kind);
            // list order inside a kind
            if (ln.first + j > 0 && (j > 0 || prev_kind == ln.kind)) {
                const uint32_t before = p.order[ln.first + j - 1];
                if (before < n && reader_kind(recs[rows[before].rec].layout) == ln.kind) EXPECT(before < i);
            }
        }
        covered += ln.count;
        prev_kind = ln.kind;
    }
    EXPECT(covered == n);
    for (size_t i = 0; i < n; i++) EXPECT(hits[i] == 1);
    std::vector<uint64_t> want(recs.size(), 0);
    std::vector<uint8_t> used(recs.size(), 0);
    for (size_t i = 0; i < n; i++) {
        const Rec &rc = recs[rows[i].rec];
        const uint64_t v = valid_frames(rows[i].start, rc.n_samples, S);
        EXPECT(v >= 1 && v <= S && v <= rc.n_samples - rows[i].start);
        EXPECT(padded(rows[i].start, rc.n_samples, S) == (v < S));
        const uint64_t lf = last_frame(rows[i].start, rc.n_samples, S);
        EXPECT(lf >= rows[i].start && lf < rc.n_samples && lf - rows[i].start == v - 1);
        want[rows[i].rec] = used[rows[i].rec] ? std::max(want[rows[i].rec], lf) : lf;
        used[rows[i].rec] = 1;
    }
    for (size_t r = 0; r < recs.size(); r++) {
        EXPECT(p.used[r] == used[r]);
        if (used[r]) EXPECT(p.last[r] == want[r]);
    }
}

int main() {
    // ---- the frames a row reads: start + S at the edge of uint64 never wraps
    {
        const uint64_t M = UINT64_MAX;
        EXPECT(valid_frames(0, 10, 4) == 4 && valid_frames(6, 10, 4) == 4 && valid_frames(7, 10, 4) == 3 && valid_frames(9, 10, 4) == 1);
        EXPECT(valid_frames(10, 10, 4) == 0 && valid_frames(M, 10, 4) == 0);
        EXPECT(valid_frames(M - 1, M, 4) == 1 && valid_frames(M - 4, M, 4) == 4 && valid_frames(M - 3, M, 4) == 3);
        EXPECT(valid_frames(M - 1, M, M) == 1 && valid_frames(0, M, M) == M && valid_frames(1, M, M) == M - 1);
        EXPECT(last_frame(M - 1, M, 4) == M - 1 && last_frame(M - 4, M, 4) == M - 1 && last_frame(M - 5, M, 4) == M - 2);
        EXPECT(last_frame(0, M, M) == M - 1 && last_frame(5, M, 0xffffffffull) == 5 + 0xfffffffeull);
        EXPECT(!padded(M - 4, M, 4) && padded(M - 3, M, 4) && padded(M - 1, M, M) && !padded(0, M, M));
        EXPECT(check_start(0, 9, 10) == BN_OK && check_start(0, M - 1, M) == BN_OK);
        EXPECT(refused(check_start(3, 10, 10), "row 3") && refused(check_start(0, M, M), "start") && refused(check_start(0, 0, 0), "start"));
    }
    // ---- reader kinds: pcm_visit's choice
    {
        EXPECT(reader_kind(PcmLayout{BN_PCM_I16, 1, 0}) == MONO_I16 && reader_kind(PcmLayout{BN_PCM_F32, 1, 0}) == MONO_F32);
        EXPECT(reader_kind(PcmLayout{BN_PCM_I16, 2, 0}) == FRAMES_I16 && reader_kind(PcmLayout{BN_PCM_F32, 2, BN_PCM_MIX}) == FRAMES_F32);
        EXPECT(reader_kind(PcmLayout{BN_PCM_I24, 1, 0}) == FRAMES_I24 && reader_kind(PcmLayout{BN_PCM_I32, 16, 15}) == FRAMES_I32);
        EXPECT(reader_kind(PcmLayout{BN_PCM_U8, 1, 0}) == FRAMES_U8 && reader_kind(PcmLayout{99, 1, 0}) < 0);
    }
    const std::vector<Rec> all_kinds{{PcmLayout{BN_PCM_I16, 1, 0}, 1000},        {PcmLayout{BN_PCM_F32, 1, 0}, 7},
                                     {PcmLayout{BN_PCM_I16, 2, BN_PCM_MIX}, 500}, {PcmLayout{BN_PCM_F32, 3, 1}, 12},
                                     {PcmLayout{BN_PCM_I24, 2, BN_PCM_MIX}, 333}, {PcmLayout{BN_PCM_I32, 1, 0}, 64},
                                     {PcmLayout{BN_PCM_U8, 4, 2}, 100},           {PcmLayout{BN_PCM_I24, 1, 0}, UINT64_MAX}};
    size_t plans = 0;
    // ---- 0, 1, 128, 129 and 257 rows (and the sizes around the cuts): every reader kind interleaved, then one recording for all rows
    for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)7, (size_t)127, (size_t)128, (size_t)129, (size_t)256, (size_t)257, (size_t)1031}) {
        for (uint64_t S : {(uint64_t)4, (uint64_t)1028, (uint64_t)144000, (uint64_t)0xfffffffcull}) {
            std::vector<Row> rows(n);
            for (size_t i = 0; i < n; i++) {
                const uint32_t r = (uint32_t)((i * 5 + i / 3) % all_kinds.size());
                rows[i] = Row{r, (uint64_t)((i * 37) % all_kinds[r].n_samples)};
                if (r == 7 && i % 2) rows[i].start = UINT64_MAX - 1 - (i % 5);  // the uint64 edge
            }
            Plan p;
            EXPECT(build(all_kinds, rows.data(), n, S, &p) == BN_OK);
            check_plan(all_kinds, rows, S, p);
            plans++;
            // a list whose rows all name one recording: one kind, ceil(n / 128) launches
            for (uint32_t r : {0u, 4u}) {
                for (size_t i = 0; i < n; i++) rows[i] = Row{r, (uint64_t)((i * 11) % all_kinds[r].n_samples)};
                EXPECT(build(all_kinds, rows.data(), n, S, &p) == BN_OK);
                check_plan(all_kinds, rows, S, p);
                EXPECT(p.launches.size() == (n + ROWS_PER_LAUNCH - 1) / ROWS_PER_LAUNCH);
                for (size_t i = 0; i < p.order.size(); i++) EXPECT(p.order[i] == i);
                for (size_t q = 0; q < all_kinds.size(); q++) EXPECT(p.used[q] == (n && q == r));
                plans++;
            }
        }
    }
    // exactly 128 rows of one kind beside one row of another: two launches, neither cut
    {
        std::vector<Row> rows(129);
        for (size_t i = 0; i < 129; i++) rows[i] = Row{i == 64 ? 1u : 0u, (uint64_t)(i % 7)};
        Plan p;
        EXPECT(build(all_kinds, rows.data(), rows.size(), 4, &p) == BN_OK);
        check_plan(all_kinds, rows, 4, p);
        EXPECT(p.launches.size() == 2 && p.launches[0].kind == MONO_I16 && p.launches[0].count == 128 && p.launches[1].kind == MONO_F32 &&
               p.launches[1].count == 1 && p.order[128] == 64 && p.order[64] == 65);
        plans++;
    }
    // ---- refusals: arrays of exactly the size named, so that a read past them is caught
    {
        Plan p;
        std::vector<Row> rows{{0, 999}, {1, 6}, {7, UINT64_MAX - 1}};
        EXPECT(build(all_kinds, rows.data(), 3, 4, &p) == BN_OK);
        EXPECT(p.last[0] == 999 && p.last[1] == 6 && p.last[7] == UINT64_MAX - 1);
        rows[1].start = 7;
        EXPECT(refused(build(all_kinds, rows.data(), 3, 4, &p), "row 1"));
        rows[1].start = UINT64_MAX;
        EXPECT(refused(build(all_kinds, rows.data(), 3, 4, &p), "row 1"));
        rows[1] = Row{8, 0};
        EXPECT(refused(build(all_kinds, rows.data(), 3, 4, &p), "names no recording"));
        rows[1] = Row{1, 0};
        EXPECT(refused(build(all_kinds, rows.data(), 3, 0, &p), "segment_samples"));
        EXPECT(refused(build(all_kinds, rows.data(), (size_t)1 << 32, 4, &p), "2^32"));  // refused before a row is read
        std::vector<Rec> bad{{PcmLayout{42, 1, 0}, 10}};
        rows[0] = Row{0, 0};
        EXPECT(refused(build(bad, rows.data(), 1, 4, &p), "unknown PCM format"));
        const std::vector<Rec> none;
        EXPECT(build(none, nullptr, 0, 4, &p) == BN_OK && p.launches.empty() && p.order.empty());
        EXPECT(refused(build(none, rows.data(), 1, 4, &p), "names no recording"));
    }
    printf("%zu plans, %d failures\n", plans, failures);
    if (failures) return 1;
    printf("asan_window_list_plan: ok\n");
    return 0;
}
