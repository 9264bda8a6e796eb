// Host-side sanitizer check of the sequence search's arithmetic (no device, no Python): the argument refusals, the packing of sequences
// into the 64 query slots of a pass, the passes and rounds of a call, the tiles a workgroup computes beyond its run and the kernel's LDS
// (rust-birdnet-onnx_amd/csrc/seq_plan.h), over edge values and a sweep.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_seq_plan.cpp -o /tmp/asan_seq_plan && /tmp/asan_seq_plan
// Exit 0: every refusal came with its message and before anything was read that need not exist; every pass fits the 64 slots and the
// cap, the cap is the largest that keeps the LDS within 160 KB, the passes cover every sequence, a round fits the staging buffers, the
// computed tiles hold what every judged start reads; nothing read memory it does not own and no arithmetic overflowed.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "seq_plan.h"

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
    using namespace bn::seq;
    // ---- arguments: arrays of exactly the size the contract names, so that a read past them is caught
    {
        std::vector<float> q(2 * 3 * 8, 1.f);
        std::vector<uint64_t> ids(2 * 4);
        std::vector<float> sc(2 * 4);
        std::vector<uint32_t> cnt(2);
        EXPECT(check_args(q.data(), 2, 3, 0, 4, 4, ids.data(), sc.data(), cnt.data()) == BN_OK);
        EXPECT(check_args(q.data(), 2, 3, BN_PEAK_RADIUS_MAX, 4, 4, ids.data(), sc.data(), cnt.data()) == BN_OK);
        EXPECT(check_args(q.data(), 2, 1, 0, 1, 4, ids.data(), sc.data(), cnt.data()) == BN_OK);
        EXPECT(check_args(q.data(), 2, BN_SEQ_LEN_MAX, 0, 256, 256, ids.data(), sc.data(), cnt.data()) == BN_OK);  // nothing is read here
        EXPECT(check_args(nullptr, 0, 3, 0, 4, 4, nullptr, nullptr, nullptr) == BN_OK);
        EXPECT(refused(check_args(q.data(), 2, 3, 0, 0, 4, ids.data(), sc.data(), cnt.data()), "top_m"));
        EXPECT(refused(check_args(q.data(), 2, 3, 0, 257, 300, ids.data(), sc.data(), cnt.data()), "top_m"));
        EXPECT(refused(check_args(q.data(), 2, 3, 0, SIZE_MAX, SIZE_MAX, ids.data(), sc.data(), cnt.data()), "top_m"));
        EXPECT(refused(check_args(q.data(), 2, 3, 0, 4, 3, ids.data(), sc.data(), cnt.data()), "m_stride"));
        EXPECT(refused(check_args(q.data(), 2, 0, 0, 4, 4, ids.data(), sc.data(), cnt.data()), "seq_len"));
        EXPECT(refused(check_args(q.data(), 2, (size_t)BN_SEQ_LEN_MAX + 1, 0, 4, 4, ids.data(), sc.data(), cnt.data()), "seq_len"));
        EXPECT(refused(check_args(q.data(), 2, SIZE_MAX, 0, 4, 4, ids.data(), sc.data(), cnt.data()), "seq_len"));
        EXPECT(refused(check_args(q.data(), 2, 3, (size_t)BN_PEAK_RADIUS_MAX + 1, 4, 4, ids.data(), sc.data(), cnt.data()), "peak_radius"));
        EXPECT(refused(check_args(q.data(), 2, 3, SIZE_MAX, 4, 4, ids.data(), sc.data(), cnt.data()), "peak_radius"));
        EXPECT(refused(check_args(nullptr, 2, 3, 0, 4, 4, ids.data(), sc.data(), cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, 3, 0, 4, 4, nullptr, sc.data(), cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, 3, 0, 4, 4, ids.data(), nullptr, cnt.data()), "null"));
        EXPECT(refused(check_args(q.data(), 2, 3, 0, 4, 4, ids.data(), sc.data(), nullptr), "null"));
        // the order of the header's list: top_m, m_stride, seq_len, peak_radius, the NULLs
        EXPECT(refused(check_args(nullptr, 2, 0, 65, 0, 0, nullptr, nullptr, nullptr), "top_m"));
        EXPECT(refused(check_args(nullptr, 2, 0, 65, 4, 3, nullptr, nullptr, nullptr), "m_stride"));
        EXPECT(refused(check_args(nullptr, 2, 0, 65, 4, 4, nullptr, nullptr, nullptr), "seq_len"));
        EXPECT(refused(check_args(nullptr, 2, 3, 65, 4, 4, nullptr, nullptr, nullptr), "peak_radius"));
    }
    // ---- the _ids form: [first_id, first_id + seq_len) within the index
    {
        const size_t big = 0xffffffffull - 65;  // the largest index
        const std::vector<uint64_t> f{0, 95, 96};
        EXPECT(check_first_ids(f.data(), 2, 5, 100) == BN_OK && check_first_ids(nullptr, 0, 5, 0) == BN_OK);
        EXPECT(check_first_ids(f.data(), 3, 4, 100) == BN_OK);
        EXPECT(refused(check_first_ids(f.data(), 3, 5, 100), "96"));
        EXPECT(refused(check_first_ids(f.data(), 1, 1, 0), "past"));
        const std::vector<uint64_t> g{big - 64, big - 63, UINT64_MAX, big};
        EXPECT(check_first_ids(g.data(), 1, 64, big) == BN_OK);
        EXPECT(refused(check_first_ids(g.data(), 2, 64, big), "past"));
        EXPECT(refused(check_first_ids(g.data() + 2, 1, 1, big), "past"));  // no wrap-around of first_id + seq_len
        EXPECT(refused(check_first_ids(g.data() + 3, 1, 1, big), "past"));
    }
    // ---- packing, cap, LDS
    EXPECT(CAP >= 1 && CAP < SLOTS && Lds::BYTES <= LDS_LIMIT && Lds::BYTES + PER_SEQ > LDS_LIMIT);
    EXPECT(Lds::Z == SCAN_LDS && Lds::FIRST == Lds::Z + (size_t)ZRING * CAP * TILE * 4 && Lds::OK == Lds::FIRST + CAP * 4 && Lds::BYTES == Lds::OK + CAP * 4);
    size_t plans = 0;
    for (size_t L = 1; L <= BN_SEQ_LEN_MAX; L++) {
        const int P = per_pass(L);
        EXPECT(P >= 1 && P <= CAP && (size_t)P * L <= SLOTS);
        EXPECT(P == CAP || (size_t)(P + 1) * L > SLOTS);  // the largest the slots and the cap allow
        EXPECT(L != 1 || P == CAP);
        EXPECT(L <= 32 || P == 1);
        EXPECT(L != 8 || P == 8);
        for (size_t n : {(size_t)0, (size_t)1, (size_t)P, (size_t)P + 1, (size_t)1000, (size_t)1 << 40}) {
            const size_t np = passes(n, L);
            EXPECT(np * P >= n && (np == 0 || (np - 1) * P < n));
            plans++;
        }
    }
    // ---- the tiles a workgroup computes: what a judged start reads lies in them
    const uint32_t tiles[] = {1, 2, 3, 4, 5, 7, 100, 2561, 0x03ffffffu};
    const uint32_t per[] = {1, 2, 3, 8, 61};
    for (uint32_t n_tiles : tiles)
        for (uint32_t tpw : per)
            for (size_t R : {(size_t)0, (size_t)1, (size_t)BN_PEAK_RADIUS_MAX}) {
                const uint32_t n_wg = (n_tiles + tpw - 1) / tpw;
                for (uint32_t g : {0u, 1u, n_wg / 2, n_wg - 2, n_wg - 1, n_wg}) {
                    if (g > n_wg) continue;  // n_wg - 2 wrapped
                    const uint32_t t0 = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)g * tpw), t1 = (uint32_t)std::min<uint64_t>(n_tiles, (uint64_t)t0 + tpw);
                    const Computed c = computed_tiles(t0, t1, n_tiles, R);
                    plans++;
                    EXPECT(c.c0 <= c.c1 && c.c1 <= n_tiles);
                    if (t0 >= t1) {
                        EXPECT(c.c0 == c.c1);
                        continue;
                    }
                    EXPECT(c.c0 <= t0 && c.c1 >= t1 && c.c1 - c.c0 <= t1 - t0 + 3);
                    // the starts judged are those of tiles [t0, t1); with R their neighbours' tiles [t0 - 1, t1 + 1) need sequence scores
                    // too; the sequence scores of tile t need the window scores of tiles t and t + 1, as far as the index has them
                    const uint32_t z0 = R && t0 ? t0 - 1 : t0, z1 = R ? std::min(n_tiles, t1 + 1) : t1;
                    EXPECT(c.c0 == z0 && c.c1 == std::min(n_tiles, z1 + 1));
                }
            }
    printf("%zu plans, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
