// Host-side sanitizer check of the delay estimate's arithmetic (no device, no Python): the refusals of a spec, Z of both weightings,
// the LDS figure and every position of it the kernel touches, where a lag lies in the row of correlations, the peak key against the
// tie rule spelt out, the floats of out_curve and the windows of a launch, and bn_delay_refine
// (rust-birdnet-onnx_amd/csrc/delay_plan.h), over edge values.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_delay_plan.cpp -o /tmp/asan_delay_plan && /tmp/asan_delay_plan
// Exit 0 and "asan_delay_plan: ok": every refusal came with its message; every lag and both neighbours of every peak lie inside the
// row; the key orders any two (value, lag) pairs as the rule does and gives the lag back; no size wrapped; nothing read memory it
// does not own and no arithmetic overflowed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "delay_plan.h"

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
using namespace bn::delay;

static uint32_t bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
}

// the rule, spelt out: is (v1, t1) a better peak than (v2, t2)?
static bool better(float v1, int32_t t1, float v2, int32_t t2) {
    if (v1 != v2) return v1 > v2;
    if (std::abs(t1) != std::abs(t2)) return std::abs(t1) < std::abs(t2);
    return t1 < t2;
}

int main() {
    size_t plans = 0;
    // ---- accepted specs
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        const double e = window_energy(N);
        EXPECT(std::fabs(e - 0.375 * N) < 1e-9 * N);  // sum of hann^2 over a period
        for (uint32_t hop : {1u, N / 2, N}) {
            for (uint64_t S : {(uint64_t)N, (uint64_t)N + 3 * hop, (uint64_t)144000, (uint64_t)0xfffffffcull}) {
                for (uint32_t weighting : {(uint32_t)BN_DELAY_PLAIN, (uint32_t)BN_DELAY_PHAT}) {
                    // the spec on the heap, exactly its size and at an odd address: a read past it or an aligned read is caught
                    std::vector<char> raw(sizeof(bn_delay_spec) + 1);
                    const bn_delay_spec s{N, hop, (uint32_t)(S % 3), N / 2 + 1 - (uint32_t)(S % 2), (uint32_t)(S % 2 ? 0 : N / 2 - 1), weighting};
                    memcpy(raw.data() + 1, &s, sizeof(s));
                    Plan p;
                    EXPECT(check_spec(reinterpret_cast<const bn_delay_spec *>(raw.data() + 1), sizeof(s), S, &p) == BN_OK);
                    EXPECT(p.N == N && p.n_lags == 2 * s.max_lag + 1 && p.n_lags < N && p.n_frames == (S - N) / hop + 1 && p.span <= S);
                    EXPECT(p.run == (p.n_frames + (uint64_t)WAVES - 1) / WAVES);
                    const double Z = normaliser(weighting, N, p.n_frames, p.lo, p.hi);
                    EXPECT(Z >= 1.0 && p.out_scale > 0.0f && std::fabs((double)p.out_scale * (weighting == BN_DELAY_PHAT ? 1.0 : 4.0) * Z - 1.0) < 1e-7);
                    // every lag, and both neighbours of every possible peak, inside the row
                    for (int32_t tau = -(int32_t)s.max_lag - 1; tau <= (int32_t)s.max_lag + 1; tau++) {
                        const uint32_t at = lag_index(N, tau);
                        EXPECT(at < N && at == (uint32_t)((tau % (int32_t)N + (int32_t)N) % (int32_t)N));
                    }
                    plans++;
                }
            }
        }
        // the band's weight against the sum it stands for
        for (uint32_t lo : {0u, 1u, N / 4}) {
            for (uint32_t hi : {lo + 1, N / 2, N / 2 + 1}) {
                uint32_t sum = 0;
                for (uint32_t k = lo; k < hi; k++) sum += (k == 0 || k == N / 2) ? 1 : 2;
                EXPECT(band_weight(N, lo, hi) == sum);
            }
        }
        // LDS: the figure, and every position the kernel's three stages touch, stays inside its array
        const uint32_t M = N / 2, rows_bytes = WAVES * 2 * (M + 1) * 4;
        EXPECT(lds_bytes(N) == rows_bytes + N * 4 + WAVES * 12 && lds_bytes(N) <= 65536);
        std::vector<char> seen(M + 1, 0);
        for (uint32_t k = 0; k <= M; k++) {
            const uint32_t at = lds_index(N, k);
            EXPECT(at <= M && !seen[at]);
            seen[at] = 1;
            if (k < M) EXPECT(lds_index(N, M - k) <= M);  // the partner bin the inverse's wave fetches
        }
        for (uint32_t r = 0; r < N / 128; r++)
            for (uint32_t lane = 0; lane < 64; lane++) EXPECT(2 * (r * 64 + lane) + 1 < N);  // the float2 store of r
    }
    // ---- refused specs
    {
        Plan p;
        const bn_delay_spec ok{1024, 512, 0, 513, 128, BN_DELAY_PHAT};
        EXPECT(refused(check_spec(nullptr, sizeof(ok), 4096, &p), "null delay spec"));
        EXPECT(refused(check_spec(&ok, sizeof(ok) - 1, 4096, &p), "spec_size"));
        bn_delay_spec s = ok;
        s.frame = 1000;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "frame"));
        s = ok, s.hop = 0;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "hop"));
        s = ok, s.hop = 1025;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "hop"));
        s = ok, s.bin_lo = 513;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "bins"));
        s = ok, s.bin_hi = 514;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "bins"));
        s = ok, s.max_lag = 512;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "max_lag"));
        s = ok, s.max_lag = 0xffffffffu;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "max_lag"));
        s = ok, s.weighting = 2;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "weighting"));
        EXPECT(refused(check_spec(&ok, sizeof(ok), 1020, &p), "segment_samples"));
        EXPECT(refused(check_spec(&ok, sizeof(ok), (uint64_t)1 << 32, &p), "segment_samples"));
        s = ok, s.max_lag = 511;
        EXPECT(check_spec(&s, sizeof(s), 4096, &p) == BN_OK && p.n_lags == 1023);
    }
    // ---- the peak key: any two (value, lag) pairs in the rule's order, and the lag back out of the key
    {
        const float values[] = {-INFINITY, -3.5f, -1e-40f, 0.0f, 1e-40f, 0.25f, 1.0f, 1.0000001f, INFINITY};
        const int32_t lags[] = {-1023, -7, -1, 0, 1, 7, 1023};
        for (float v1 : values)
            for (int32_t t1 : lags) {
                const uint64_t k1 = peak_key(bits_of(v1), t1);
                EXPECT(key_lag(k1) == t1 && k1 > 0);
                for (float v2 : values)
                    for (int32_t t2 : lags) {
                        if (v1 == v2 && t1 == t2) continue;
                        EXPECT((k1 > peak_key(bits_of(v2), t2)) == better(v1, t1, v2, t2));
                    }
            }
    }
    // ---- the curve's sizes and the windows of a launch
    {
        size_t n = 0;
        EXPECT(curve_floats(10, 257, &n) && n == 2570);
        EXPECT(!curve_floats(SIZE_MAX / 4, 3, &n) && !curve_floats(SIZE_MAX, 1, &n) && !curve_floats(1, 0, &n));
        EXPECT(curve_floats(SIZE_MAX / 4 / 1023, 1023, &n));
        for (uint32_t lags : {1u, 3u, 257u, 2047u}) {
            const size_t piece = piece_windows(lags);
            EXPECT(piece >= 1 && piece <= ((size_t)1 << 20) && piece * lags <= ((size_t)1 << 26));
        }
    }
    // ---- bn_delay_refine
    {
        double lag = 99.0;
        bn_window_delay w{5, 1.0f, 0.5f, 0.5f, 0, 4};
        EXPECT(refine(&w, sizeof(w), &lag) == BN_OK && lag == 5.0);  // a symmetric peak
        w = bn_window_delay{-3, 1.0f, 0.0f, 0.5f, 0, 4};             // the parabola through (-1, 0), (0, 1), (1, 0.5): vertex at +1/6
        EXPECT(refine(&w, sizeof(w), &lag) == BN_OK && std::fabs(lag - (-3.0 + 0.5 * (0.0 - 0.5) / (0.0 - 2.0 + 0.5))) < 1e-15);
        w = bn_window_delay{2, 1.0f, 1.0f, 1.0f, 0, 4};  // a line: no vertex
        EXPECT(refine(&w, sizeof(w), &lag) == BN_OK && lag == 2.0);
        w = bn_window_delay{2, 1.0f, 0.0f, 1.5f, 0, 4};  // not a peak at all: clamped
        EXPECT(refine(&w, sizeof(w), &lag) == BN_OK && lag == 2.5);
        w = bn_window_delay{2, 1.0f, 1.5f, 0.0f, 0, 4};
        EXPECT(refine(&w, sizeof(w), &lag) == BN_OK && lag == 1.5);
        w = bn_window_delay{0, NAN, NAN, NAN, BN_LEVEL_NONFINITE, 4};
        EXPECT(refine(&w, sizeof(w), &lag) == BN_OK && lag == 0.0);
        // a record at an odd address, exactly its size
        std::vector<char> raw(sizeof(w) + 1);
        w = bn_window_delay{7, 2.0f, 1.0f, 1.0f, 0, 1};
        memcpy(raw.data() + 1, &w, sizeof(w));
        EXPECT(refine(reinterpret_cast<const bn_window_delay *>(raw.data() + 1), sizeof(w), &lag) == BN_OK && lag == 7.0);
        EXPECT(refused(refine(nullptr, sizeof(w), &lag), "null") && refused(refine(&w, sizeof(w), nullptr), "null"));
        EXPECT(refused(refine(&w, sizeof(w) - 1, &lag), "struct_size"));
    }
    if (failures) {
        fprintf(stderr, "asan_delay_plan: %d failures\n", failures);
        return 1;
    }
    printf("asan_delay_plan: ok (%zu plans)\n", plans);
    return 0;
}
