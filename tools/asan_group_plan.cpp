// Host-side sanitizer check of the grouped threshold search's arithmetic (no device, no Python): the argument refusals, the id range it
// shares with the threshold search and the plan of a call (rust-birdnet-onnx_amd/csrc/group_plan.h), over edge values and a sweep.
//   make tools/asan_group_plan && tools/asan_group_plan
//   (g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc)
// Exit 0: every refusal came with its message, in the documented order and before anything was read that need not exist; every plan
// covers its range with non-empty workgroups, has a listed width, keeps its table within the budget and would not have fitted the next
// wider pass; nothing read memory it does not own and no arithmetic overflowed.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "group_plan.h"

static std::string g_last;
// the library's definition lives in capi.cpp, which needs the runtime
bn_status bn::set_last_error(bn_status st, const std::string &msg) {
    g_last = msg;
    return st;
}

static int failures = 0, refusals = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) failures++, fprintf(stderr, "line %d: %s\n", __LINE__, #cond); \
    } while (0)

static bool refused(bn_status st, const char *word) {
    refusals++;
    return st == BN_ERR_INVALID_ARG && g_last.find(word) != std::string::npos;
}

int main() {
    using namespace bn::group;
    using bn::above::BUDGET;
    using bn::above::check_range;
    using bn::above::TILE;
    using bn::above::WIDTHS;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const size_t limit = BN_INDEX_TAG_LIMIT;
    // ---- arguments: arrays of exactly the size the contract names, so that a read past them is caught
    {
        std::vector<float> q(2 * 8, 1.f), thr{0.5f, -inf};
        std::vector<uint32_t> cnt(2 * 4);
        std::vector<uint64_t> bid(2 * 4);
        std::vector<float> bsc(2 * 4);
        EXPECT(check_args(q.data(), 2, thr.data(), 4, 4, cnt.data(), bid.data(), bsc.data()) == BN_OK);
        EXPECT(check_args(q.data(), 2, thr.data(), 3, 4, cnt.data(), nullptr, nullptr) == BN_OK);
        EXPECT(check_args(q.data(), 2, thr.data(), 1, 1, cnt.data(), nullptr, nullptr) == BN_OK);
        EXPECT(check_args(nullptr, 0, nullptr, 4, 4, nullptr, nullptr, nullptr) == BN_OK);
        EXPECT(check_args(q.data(), 2, thr.data(), limit, limit, cnt.data(), nullptr, nullptr) == BN_OK);  // sizes are not read
        EXPECT(check_args(q.data(), 2, thr.data(), limit, SIZE_MAX, cnt.data(), nullptr, nullptr) == BN_OK);
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 0, 4, cnt.data(), bid.data(), bsc.data()), "n_groups"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), limit + 1, SIZE_MAX, cnt.data(), bid.data(), bsc.data()), "n_groups"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), SIZE_MAX, SIZE_MAX, cnt.data(), bid.data(), bsc.data()), "n_groups"));
        EXPECT(refused(check_args(nullptr, 0, nullptr, 0, 0, nullptr, nullptr, nullptr), "n_groups"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 3, cnt.data(), bid.data(), bsc.data()), "g_stride"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 0, cnt.data(), bid.data(), bsc.data()), "g_stride"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, cnt.data(), bid.data(), nullptr), "pair"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, cnt.data(), nullptr, bsc.data()), "pair"));
        EXPECT(refused(check_args(nullptr, 0, nullptr, 4, 4, nullptr, bid.data(), nullptr), "pair"));
        EXPECT(refused(check_args(nullptr, 2, thr.data(), 4, 4, cnt.data(), bid.data(), bsc.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, nullptr, 4, 4, cnt.data(), bid.data(), bsc.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, nullptr, bid.data(), bsc.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, thr.data(), 4, 4, nullptr, nullptr, nullptr), "null"));
        for (size_t bad = 0; bad < 2; bad++) {
            std::vector<float> t{inf, 0.f};
            t[bad] = nan;
            EXPECT(refused(check_args(q.data(), 2, t.data(), 4, 4, cnt.data(), bid.data(), bsc.data()), "NaN"));
            EXPECT(refused(check_args(q.data(), 2, t.data(), 1, 1, cnt.data(), nullptr, nullptr), "NaN"));
            // the order of the header: the limits and the pair come before the NaN
            EXPECT(refused(check_args(q.data(), 2, t.data(), 0, 0, cnt.data(), nullptr, nullptr), "n_groups"));
            EXPECT(refused(check_args(q.data(), 2, t.data(), 4, 4, cnt.data(), bid.data(), nullptr), "pair"));
        }
    }
    // ---- the id range: above_plan.h's, as group.hip calls it
    {
        uint32_t lo = 7, hi = 7;
        const size_t big = 0xffffffffull - 65;  // the largest index
        EXPECT(check_range(0, 0, 0, &lo, &hi) == BN_OK && lo == 0 && hi == 0);
        EXPECT(check_range(37, 5, 100, &lo, &hi) == BN_OK && lo == 37 && hi == 42);
        EXPECT(check_range(100, 0, 100, &lo, &hi) == BN_OK && lo == 100 && hi == 100);
        EXPECT(check_range(big - 1, 1, big, &lo, &hi) == BN_OK && lo == big - 1 && hi == big);
        lo = hi = 7;
        EXPECT(refused(check_range(101, 0, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(99, 2, 100, &lo, &hi), "past"));
        EXPECT(refused(check_range(UINT64_MAX, UINT64_MAX, big, &lo, &hi), "past"));
        EXPECT(lo == 7 && hi == 7);
    }
    // ---- plans
    size_t plans = 0;
    const uint32_t sizes[] = {1, 63, 64, 65, 4096, 163877, 1000000, 20000000, 0xffffffffu - 65};
    const size_t groups[] = {1, 2, 64, 52428, 52429, 65535, 65536};
    const size_t wgs[] = {1, 2, 7, 256, 304, 320};
    for (uint32_t size : sizes)
        for (size_t n_groups : groups)
            for (size_t max_wg : wgs)
                for (int part = 0; part < 4; part++) {
                    const uint32_t lo = part == 0 ? 0 : part == 1 ? size / 3 : part == 2 ? size - 1 : size / 2;
                    const uint32_t hi = part == 3 ? (uint32_t)std::min<uint64_t>(size, (uint64_t)lo + 70) : size;
                    if (lo >= hi) continue;
                    const Plan p = plan(lo, hi, max_wg, n_groups);
                    plans++;
                    const uint64_t covered = (uint64_t)p.n_wg * p.tiles_per_wg * TILE;
                    EXPECT((uint64_t)p.tile_lo * TILE <= lo && (uint64_t)p.tile_hi * TILE >= hi && (uint64_t)p.tile_hi * TILE < (uint64_t)hi + TILE);
                    EXPECT(p.n_wg >= 1 && p.n_wg <= max_wg && p.tiles_per_wg >= 1);
                    EXPECT(covered >= (uint64_t)(p.tile_hi - p.tile_lo) * TILE);                  // every tile has a workgroup
                    EXPECT((uint64_t)(p.n_wg - 1) * p.tiles_per_wg < p.tile_hi - p.tile_lo);      // and no workgroup is empty
                    const bn::above::Plan a = bn::above::plan(lo, hi, max_wg, 0);                  // the split is the count's
                    EXPECT(a.tile_lo == p.tile_lo && a.tile_hi == p.tile_hi && a.tiles_per_wg == p.tiles_per_wg && a.n_wg == p.n_wg);
                    bool listed = false;
                    for (int w : WIDTHS) listed = listed || w == p.width;
                    EXPECT(listed);
                    EXPECT(p.records == (size_t)p.width * n_groups && p.bytes() == p.records * RECORD);
                    EXPECT(p.bytes() <= BUDGET);  // one query's records always fit: the floor is never reached
                    if (p.width < 64) {           // the next wider pass would not have fitted
                        int wider = 64;
                        for (int w : WIDTHS)
                            if (w > p.width) wider = w;
                        EXPECT(p.bytes() / p.width * wider > BUDGET);
                    }
                    EXPECT(p.width == (n_groups <= 52428 ? 64 : 48));  // the header's figures
                }
    printf("%zu plans, %d refusals, %d failures\n", plans, refusals, failures);
    return failures ? 1 : 0;
}
