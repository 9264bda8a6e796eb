// Host-side sanitizer check of the threshold search's arithmetic (no device, no Python): the argument refusals, the id range and the plan
// of a call (rust-birdnet-onnx_amd/csrc/above_plan.h), over edge values and a sweep.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_above_plan.cpp -o /tmp/asan_above_plan && /tmp/asan_above_plan
// Exit 0: every refusal came with its message and before anything was read that need not exist, every plan covers its range with
// non-empty workgroups, keeps within the budget unless it is at the floor of one query per pass, and stays below the documented worst
// case; nothing read memory it does not own and no arithmetic overflowed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "above_plan.h"

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

int main() {
    using namespace bn::above;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- arguments: arrays of exactly the size the contract names, so that a read past them is caught
    {
        std::vector<float> q(2 * 8, 1.f), thr{0.5f, -inf};
        std::vector<uint64_t> ids(2 * 4);
        std::vector<float> sc(2 * 4);
        std::vector<uint32_t> cnt(2);
        EXPECT(check_args(q.data(), 2, thr.data(), 4, 4, ids.data(), sc.data(), cnt.data()) == BN_OK);
        EXPECT(check_args(q.data(), 2, thr.data(), 0, 0, nullptr, nullptr, cnt.data()) == BN_OK);
        EXPECT(check_args(nullptr, 0, nullptr, 4, 4, nullptr, nullptr, nullptr) == BN_OK);
        EXPECT(check_args(q.data(), 2, thr.data(), BN_ABOVE_MAX_HITS, BN_ABOVE_MAX_HITS, ids.data(), sc.data(), cnt.data()) == BN_OK);
        EXPECT(refused(check_args(q.data(), 2, thr.data(), (size_t)BN_ABOVE_MAX_HITS + 1, SIZE_MAX, ids.data(), sc.data(), cnt.data()), "max_hits"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), SIZE_MAX, SIZE_MAX, ids.data(), sc.data(), cnt.data()), "max_hits"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 3, ids.data(), sc.data(), cnt.data()), "h_stride"));
        EXPECT(refused(check_args(nullptr, 2, thr.data(), 4, 4, ids.data(), sc.data(), cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, nullptr, 4, 4, ids.data(), sc.data(), cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, ids.data(), sc.data(), nullptr), "null"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, nullptr, sc.data(), cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, ids.data(), nullptr, cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 0, 0, nullptr, nullptr, nullptr), "null"));
        for (size_t bad = 0; bad < 2; bad++) {
            std::vector<float> t{inf, 0.f};
            t[bad] = nan;
            EXPECT(refused(check_args(q.data(), 2, t.data(), 4, 4, ids.data(), sc.data(), cnt.data()), "NaN"));
            EXPECT(refused(check_args(q.data(), 2, t.data(), 0, 0, nullptr, nullptr, cnt.data()), "NaN"));
        }
    }
    // ---- the id range
    {
        uint32_t lo = 7, hi = 7;
        const size_t big = 0xffffffffull - 65;  // the largest index
        EXPECT(check_range(0, 0, 0, &lo, &hi) == BN_OK && lo == 0 && hi == 0);
        EXPECT(check_range(0, 0, 100, &lo, &hi) == BN_OK && lo == 0 && hi == 100);
        EXPECT(check_range(100, 0, 100, &lo, &hi) == BN_OK && lo == 100 && hi == 100);
        EXPECT(check_range(37, 5, 100, &lo, &hi) == BN_OK && lo == 37 && hi == 42);
        EXPECT(check_range(big - 1, 1, big, &lo, &hi) == BN_OK && lo == big - 1 && hi == big);
        lo = hi = 7;
        EXPECT(refused(check_range(101, 0, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(0, 101, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(99, 2, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(UINT64_MAX, 0, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(1, UINT64_MAX, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(UINT64_MAX, UINT64_MAX, big, &lo, &hi), "past"));
        EXPECT(lo == 7 && hi == 7);
    }
    // ---- plans
    size_t plans = 0;
    const uint32_t sizes[] = {1, 63, 64, 65, 4096, 163877, 1000000, 20000000, 0xffffffffu - 65};
    const size_t hits[] = {0, 1, 63, 64, 65, 100, 1000, 4096, BN_ABOVE_MAX_HITS};
    const size_t wgs[] = {1, 2, 7, 256, 304, 320};
    for (uint32_t size : sizes)
        for (size_t max_hits : hits)
            for (size_t max_wg : wgs)
                for (int part = 0; part < 4; part++) {
                    const uint32_t lo = part == 0 ? 0 : part == 1 ? size / 3 : part == 2 ? size - 1 : size / 2;
                    const uint32_t hi = part == 3 ? (uint32_t)std::min<uint64_t>(size, (uint64_t)lo + 70) : size;
                    if (lo >= hi) continue;
                    const Plan p = plan(lo, hi, max_wg, max_hits);
                    plans++;
                    const uint64_t rows_wg = (uint64_t)p.tiles_per_wg * TILE, covered = (uint64_t)p.n_wg * rows_wg;
                    EXPECT((uint64_t)p.tile_lo * TILE <= lo && (uint64_t)p.tile_hi * TILE >= hi && (uint64_t)p.tile_hi * TILE < (uint64_t)hi + TILE);
                    EXPECT(p.n_wg >= 1 && p.n_wg <= max_wg && p.tiles_per_wg >= 1);
                    EXPECT(covered >= (uint64_t)(p.tile_hi - p.tile_lo) * TILE);                              // every tile has a workgroup
                    EXPECT((uint64_t)(p.n_wg - 1) * p.tiles_per_wg < p.tile_hi - p.tile_lo);                  // and no workgroup is empty
                    EXPECT(p.cap_wg == std::min<uint64_t>(rows_wg, max_hits));
                    bool listed = false;
                    for (int w : WIDTHS) listed = listed || w == p.width;
                    EXPECT(listed);
                    EXPECT(p.stage_entries == (size_t)p.n_wg * p.width * p.cap_wg && p.result_entries == (size_t)p.width * max_hits);
                    EXPECT(p.bytes() <= BUDGET || p.width == 1);
                    if (p.width < 64) {  // the next wider pass would not have fitted
                        int wider = 64;
                        for (int w : WIDTHS)
                            if (w > p.width) wider = w;
                        EXPECT(p.bytes() / p.width * wider > BUDGET);
                    }
                    if (p.width == 1)  // the documented worst case
                        EXPECT(p.bytes() <= ENTRY * std::min<uint64_t>(covered, (uint64_t)p.n_wg * max_hits) + RESULT * max_hits);
                    if (max_hits == 0) EXPECT(p.width == 64 && p.bytes() == 0);
                }
    printf("%zu plans, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
