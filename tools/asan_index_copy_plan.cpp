// Host-side sanitizer check of the row copy's arithmetic (no device, no Python): the argument refusals, the id range and the plan of a
// call (rust-birdnet-onnx_amd/csrc/index_copy_plan.h), over edge values and a sweep.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_index_copy_plan.cpp -o /tmp/asan_index_copy_plan && /tmp/asan_index_copy_plan
// Exit 0: every refusal came with its message and left its outputs alone; every plan's units are exactly its rows, its grid is never
// empty, never more than the steps there are and never more than 8 workgroups per CU; a walk of the kernel's own numbering over small
// plans visits every unit of the destination exactly once and stays inside both slabs; no arithmetic overflowed.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "index_copy_plan.h"

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

// index_copy_kernel's numbering on the host: for every (workgroup, step, half-wave, unit in flight) the destination unit and the source
// unit it names.  hits[u]: how often destination unit u is written; the source unit must lie in the source slab
static void walk(const bn::copy::Plan &p, uint64_t n, const std::vector<uint32_t> *ids, uint32_t first_id, uint64_t src_rows, std::vector<int> *hits) {
    using namespace bn::copy;
    const uint32_t halves = BLOCK / UNIT_LANES;
    for (uint64_t b = 0; b < p.grid; b++)
        for (uint64_t base = b * STEP_UNITS; base < p.n_units; base += (uint64_t)p.grid * STEP_UNITS) {
            const uint64_t row0 = base / p.units_per_row;
            const uint32_t piece0 = (uint32_t)(base - row0 * p.units_per_row);
            for (uint32_t h = 0; h < halves; h++)
                for (uint32_t k = 0; k < IN_FLIGHT; k++) {
                    const uint32_t o = k * halves + h, pc = piece0 + o;
                    if (base + o >= p.n_units) continue;
                    const uint64_t row = row0 + pc / p.units_per_row;
                    const uint32_t piece = pc % p.units_per_row;
                    EXPECT(row < n && row * p.units_per_row + piece == base + o);
                    const uint64_t from = ids ? (*ids)[row] : first_id + row;
                    EXPECT(from < src_rows);
                    (*hits)[base + o]++;
                }
        }
}

int main() {
    using namespace bn::copy;
    // ---- handles and pairs
    {
        int a = 0, b = 0;
        EXPECT(check_handles(&a, &b, "index") == BN_OK);
        EXPECT(refused(check_handles(nullptr, &b, "index"), "null destination"));
        EXPECT(refused(check_handles(&a, nullptr, "index"), "null source index"));
        EXPECT(refused(check_handles(&a, nullptr, "subset"), "null source subset"));
        EXPECT(refused(check_handles(nullptr, nullptr, "subset"), "null destination"));
        EXPECT(check_pair(&a, &b, false, 130, 130, 0, 0) == BN_OK);
        EXPECT(refused(check_pair(&a, &a, false, 130, 130, 0, 0), "same index"));
        EXPECT(refused(check_pair(&a, &a, true, 130, 130, 0, 0), "borrows"));
        EXPECT(refused(check_pair(&a, &a, false, 130, 131, 0, 1), "same index"));  // the header's order
        EXPECT(refused(check_pair(&a, &b, false, 130, 131, 0, 1), "dim"));
        EXPECT(refused(check_pair(&a, &b, true, 130, 130, 0, 1), "device"));
    }
    // ---- the id range
    {
        uint64_t first = 7, n = 7;
        const size_t big = 0xffffffffull - 65;  // the largest index
        EXPECT(check_range(0, 0, 0, &first, &n) == BN_OK && first == 0 && n == 0);
        EXPECT(check_range(0, 0, 100, &first, &n) == BN_OK && first == 0 && n == 100);
        EXPECT(check_range(100, 0, 100, &first, &n) == BN_OK && first == 100 && n == 0);
        EXPECT(check_range(37, 5, 100, &first, &n) == BN_OK && first == 37 && n == 5);
        EXPECT(check_range(99, 1, 100, &first, &n) == BN_OK && first == 99 && n == 1);
        EXPECT(check_range(big - 1, 1, big, &first, &n) == BN_OK && first == big - 1 && n == 1);
        first = n = 7;
        EXPECT(refused(check_range(101, 0, 100, &first, &n), "range"));
        EXPECT(refused(check_range(0, 101, 100, &first, &n), "range"));
        EXPECT(refused(check_range(99, 2, 100, &first, &n), "range"));
        EXPECT(refused(check_range(100, 1, 100, &first, &n), "range"));
        EXPECT(refused(check_range(UINT64_MAX, 0, 100, &first, &n), "range"));
        EXPECT(refused(check_range(1, UINT64_MAX, 100, &first, &n), "range"));
        EXPECT(refused(check_range(UINT64_MAX, UINT64_MAX, big, &first, &n), "range"));
        EXPECT(first == 7 && n == 7);
    }
    // ---- plans: refusals, then a sweep
    {
        Plan p;
        p.grid = 77;
        EXPECT(refused(plan(0, 128, 256, &p), "nothing"));
        EXPECT(refused(plan(5, 128, 0, &p), "nothing"));
        EXPECT(refused(plan(5, 0, 256, &p), "whole"));
        EXPECT(refused(plan(5, 130, 256, &p), "whole"));
        EXPECT(refused(plan(5, 64, 256, &p), "whole"));
        EXPECT(refused(plan(MAX_ROWS + 1, 128, 256, &p), "more than"));
        EXPECT(refused(plan(UINT64_MAX, 128, 256, &p), "more than"));
        EXPECT(refused(plan(MAX_ROWS, SIZE_MAX / 128 * 128, 256, &p), "whole"));          // more units per row than 32 bits
        EXPECT(refused(plan(MAX_ROWS, (size_t)128 << 31, 256, &p), "overflow"));         // 2^32 rows x 2^38 floats x 4 bytes
        EXPECT(p.grid == 77);
        EXPECT(plan(MAX_ROWS, (size_t)1 << 20, 256, &p) == BN_OK && p.n_units == MAX_ROWS * 8192 && p.slab_bytes == (size_t)MAX_ROWS << 22);
    }
    size_t plans = 0, walks = 0;
    const uint64_t rows[] = {1, 2, 3, 7, 31, 32, 33, 63, 64, 65, 700, 4096, 163877, 1000000, 20000000, MAX_ROWS};
    const size_t dpads[] = {128, 256, 384, 1536, 4096, (size_t)1 << 20};
    const size_t cus[] = {1, 2, 7, 256, 304, SIZE_MAX};
    for (uint64_t n : rows)
        for (size_t dpad : dpads)
            for (size_t max_wg : cus) {
                Plan p;
                EXPECT(plan(n, dpad, max_wg, &p) == BN_OK);
                plans++;
                const uint64_t steps = (p.n_units + STEP_UNITS - 1) / STEP_UNITS;
                EXPECT(p.units_per_row == dpad / UNIT_FLOATS && p.n_units == n * p.units_per_row);
                EXPECT(p.slab_bytes == (size_t)n * dpad * sizeof(float) && p.slab_bytes / sizeof(float) / dpad == n);
                EXPECT(p.grid >= 1 && p.grid <= steps && p.grid <= std::min(max_wg, MAX_CUS) * WG_PER_CU);
                EXPECT(p.grid == steps || p.grid == std::min(max_wg, MAX_CUS) * WG_PER_CU);
                if (p.n_units > 200000 || max_wg > 304) continue;
                // the kernel's numbering: a range, and a list of every other row and the last
                std::vector<int> hits(p.n_units, 0);
                walk(p, n, nullptr, 5, n + 5, &hits);
                EXPECT(std::all_of(hits.begin(), hits.end(), [](int c) { return c == 1; }));
                std::vector<uint32_t> ids;
                for (uint64_t j = 0; j < n; j++) ids.push_back((uint32_t)(2 * j));
                ids.back() = (uint32_t)(2 * n + 3);
                std::fill(hits.begin(), hits.end(), 0);
                walk(p, n, &ids, 0, 2 * n + 4, &hits);
                EXPECT(std::all_of(hits.begin(), hits.end(), [](int c) { return c == 1; }));
                walks += 2;
            }
    printf("%zu plans, %zu walks, %d failures\n", plans, walks, failures);
    return failures ? 1 : 0;
}
