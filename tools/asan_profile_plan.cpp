// Host-side sanitizer check of the spectral profile's arithmetic (no device, no Python): the refusals of a spec, the frames of a
// window, the run of frames each wave owns and the boundary frame it transforms besides, the LDS figure and the swizzle of a row, the
// floats of out_bins and the windows of a launch (rust-birdnet-onnx_amd/csrc/profile_plan.h), over edge values.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_profile_plan.cpp -o /tmp/asan_profile_plan && /tmp/asan_profile_plan
// Exit 0 and "asan_profile_plan: ok": every refusal came with its message; the four runs partition [0, F) in order and every
// difference t | t + 1 belongs to exactly one wave; the swizzle is a bijection of a row that spreads each half wave's store over 32
// banks; no size wrapped; nothing read memory it does not own and no arithmetic overflowed.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "profile_plan.h"

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
using namespace bn::profile;

// the runs of a window of F frames: a partition of [0, F) in wave order, and each difference t | t + 1 in exactly one wave
static void check_runs(uint32_t F, uint32_t q) {
    uint32_t next = 0;
    uint64_t diffs = 0;
    for (uint32_t w = 0; w < WAVES; w++) {
        uint32_t f0 = 99, f1 = 99;
        bool extra = true;
        wave_frames(F, q, w, &f0, &f1, &extra);
        EXPECT(f0 == next && f1 >= f0 && f1 <= F && f1 - f0 <= q);
        EXPECT(extra == (f0 < f1 && f1 < F));  // the frame it transforms besides exists and is the next wave's first
        if (f0 < f1) diffs += (uint64_t)(f1 - f0 - 1) + (extra ? 1 : 0);
        next = f1;
    }
    EXPECT(next == F && diffs == (uint64_t)F - 1);
}

int main() {
    size_t plans = 0;
    // ---- accepted specs
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        for (uint32_t hop : {1u, 100u, N / 2, N}) {
            for (uint64_t S : {(uint64_t)N, (uint64_t)N + hop, (uint64_t)8192, (uint64_t)144000, (uint64_t)0xfffffffcull}) {
                if (S < N) continue;
                // the spec on the heap, exactly its size and at an odd address: a read past it or an aligned read is caught
                std::vector<char> raw(sizeof(bn_profile_spec) + 1);
                const bn_profile_spec s{N, hop, (uint32_t)(S % 3), N / 2 + 1 - (uint32_t)(S % 2)};
                memcpy(raw.data() + 1, &s, sizeof(s));
                Plan p;
                EXPECT(check_spec(reinterpret_cast<const bn_profile_spec *>(raw.data() + 1), sizeof(bn_profile_spec), S, &p) == BN_OK);
                EXPECT(p.N == N && p.hop == hop && p.lo == s.bin_lo && p.hi == s.bin_hi && p.n_bins == s.bin_hi - s.bin_lo);
                EXPECT((uint64_t)p.n_frames == (S - N) / hop + 1 && (uint64_t)p.span == (uint64_t)(p.n_frames - 1) * hop + N && p.span <= S);
                EXPECT((uint64_t)p.unread == S - p.span && p.unread < hop);
                EXPECT((uint64_t)p.run * WAVES >= p.n_frames && (uint64_t)(p.run - 1) * WAVES < p.n_frames);
                check_runs(p.n_frames, p.run);
                plans++;
            }
        }
    }
    {
        Plan p;
        const bn_profile_spec a{1024, 512, 43, 214};
        EXPECT(check_spec(&a, sizeof(a), 144000, &p) == BN_OK && p.n_frames == 280 && p.run == 70 && p.unread == 128 && p.n_bins == 171);
        EXPECT(check_spec(&a, sizeof(a) + 8, 144000, &p) == BN_OK);  // a longer struct of a later header
    }
    // ---- runs: waves with no frame, one frame and no successor, uneven runs
    for (uint32_t F = 1; F <= 41; F++) check_runs(F, F / WAVES + (F % WAVES != 0));
    check_runs(0xffffff01u, 0x3fffffc1u);
    {
        uint32_t f0, f1;
        bool extra;
        wave_frames(5, 2, 2, &f0, &f1, &extra);
        EXPECT(f0 == 4 && f1 == 5 && !extra);
        wave_frames(5, 2, 1, &f0, &f1, &extra);
        EXPECT(f0 == 2 && f1 == 4 && extra);
        wave_frames(5, 2, 3, &f0, &f1, &extra);
        EXPECT(f0 == 5 && f1 == 5 && !extra);
        wave_frames(1, 1, 0, &f0, &f1, &extra);
        EXPECT(f0 == 0 && f1 == 1 && !extra);
    }
    // ---- refusals
    {
        Plan p;
        bn_profile_spec s{1024, 512, 0, 513};
        EXPECT(refused(check_spec(nullptr, sizeof(s), 4096, &p), "null profile spec"));
        EXPECT(refused(check_spec(&s, sizeof(s) - 1, 4096, &p), "spec_size") && refused(check_spec(&s, 0, 4096, &p), "spec_size"));
        for (uint32_t f : {0u, 255u, 1000u, 4096u, 0xffffffffu}) {
            s = {f, 512, 0, 10};
            EXPECT(refused(check_spec(&s, sizeof(s), 144000, &p), "frame"));
        }
        s = {1024, 512, 0, 513};
        EXPECT(refused(check_spec(&s, sizeof(s), 1023, &p), "below the frame") && refused(check_spec(&s, sizeof(s), (uint64_t)1 << 32, &p), "2^32"));
        for (uint32_t hop : {0u, 1025u, 0xffffffffu}) {
            s = {1024, hop, 0, 513};
            EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "hop"));
        }
        for (auto [lo, hi] : {std::pair<uint32_t, uint32_t>{10, 10}, {11, 10}, {0, 514}, {0xffffffffu, 0}, {513, 514}}) {
            s = {1024, 512, lo, hi};
            EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "bins ["));
        }
        s = {1024, 512, 512, 513};
        EXPECT(check_spec(&s, sizeof(s), 4096, &p) == BN_OK && p.n_bins == 1);
    }
    // ---- LDS: the figure, and the swizzle of a row
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        const uint32_t M = N / 2, RR = M / 64;
        EXPECT(lds_bytes(N) == 4 * (3 * (M + 1) + 3) * 4 && lds_bytes(N) <= 65536);
        std::vector<int> seen(M + 1, 0);
        for (uint32_t k = 0; k <= M; k++) {
            const uint32_t at = lds_index(N, k);
            EXPECT(at <= M && seen[at]++ == 0);
        }
        EXPECT(lds_index(N, M) == M);
        // the store of register slot q by half wave h: lanes whose 6-bit reversal is L = 2 L' + h write bin L RR + q
        for (uint32_t q = 0; q < RR; q++) {
            for (uint32_t h = 0; h < 2; h++) {
                uint32_t banks = 0;
                for (uint32_t l = 0; l < 32; l++) banks |= 1u << (lds_index(N, (2 * l + h) * RR + q) % 32);
                EXPECT(banks == 0xffffffffu);
            }
        }
        plans++;
    }
    EXPECT(lds_bytes(2048) == 49248);
    // ---- the floats of out_bins and the windows of a launch
    {
        size_t n = 7;
        EXPECT(bins_floats(5, 129, &n) && n == 5 * 3 * 129);
        EXPECT(bins_floats(0, 1, &n) && n == 0);
        EXPECT(!bins_floats(1, 0, &n));
        EXPECT(!bins_floats(SIZE_MAX, 1, &n) && !bins_floats(SIZE_MAX / 4 / 3 + 1, 1, &n) && !bins_floats(SIZE_MAX / 4 / 3075 + 1, 1025, &n));
        EXPECT(bins_floats(SIZE_MAX / 4 / 3075, 1025, &n) && n / 3075 == SIZE_MAX / 4 / 3075);
        for (uint32_t nb : {1u, 14u, 129u, 1025u}) {
            const size_t piece = piece_windows(nb);
            EXPECT(piece >= 1 && piece <= ((size_t)1 << 20) && piece * 3 * nb <= ((size_t)1 << 26));
        }
        EXPECT(piece_windows(1) == (size_t)1 << 20 && piece_windows(0) == (size_t)1 << 20);
    }
    printf("%zu plans, %d failures\n", plans, failures);
    if (failures) return 1;
    printf("asan_profile_plan: ok\n");
    return 0;
}
