// Host-side sanitizer check of PCEN's arithmetic (no device, no Python): the spec's refusals field by field, NaN included, the
// bytes of the output at extreme n_frames, the launch pieces at a small piece length -- every chunk of a call lies whole in one
// piece, starts where the call's own chunking puts it, and the last one is partial -- apow against a running product, and the
// threshold table (rust-birdnet-onnx_amd/csrc/pcen_plan.h).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/asan_pcen_plan.cpp -o /tmp/asan_pcen_plan && /tmp/asan_pcen_plan
// Exit 0 and "asan_pcen_plan: ok": every refusal came with its message; no size wrapped; the pieces tile the call in whole chunks;
// nothing read memory it does not own and no arithmetic overflowed.
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "pcen_plan.h"

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
using namespace bn::pcen;

static void refusals() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const bn_pcen_spec good{BN_PCEN_U8, 0.025f, 1e6f, 0.98f, 2.0f, 0.5f, 1e-6f, 8.0f};
    Plan p;
    EXPECT(check_spec(&good, sizeof good, &p) == BN_OK && p.elem == 1 && p.s == 0.025f && p.a == 1.0f - 0.025f && p.max_value == 8.0f);
    EXPECT(refused(check_spec(nullptr, sizeof good, &p), "null PCEN spec") && refused(check_spec(&good, sizeof good - 1, &p), "pcen_size"));
    struct Case {
        size_t field;  // in floats from the struct's start
        float value;
        const char *word;
    };
    const Case cases[] = {{1, 0.0f, "smooth"}, {1, 1.5f, "smooth"}, {1, nan, "smooth"}, {2, 0.0f, "gain"},   {2, inf, "gain"},   {2, nan, "gain"},
                          {3, -0.1f, "alpha"}, {3, 1.1f, "alpha"},  {3, nan, "alpha"},  {4, -1.0f, "delta"}, {4, inf, "delta"},  {4, nan, "delta"},
                          {5, 0.0f, "r must"}, {5, 1.1f, "r must"}, {5, nan, "r must"}, {6, 0.0f, "eps"},    {6, inf, "eps"},    {6, nan, "eps"},
                          {7, 0.0f, "max_value"}, {7, inf, "max_value"}, {7, nan, "max_value"}};
    for (const Case &c : cases) {
        bn_pcen_spec s = good;
        memcpy(reinterpret_cast<char *>(&s) + 4 * c.field, &c.value, 4);
        EXPECT(refused(check_spec(&s, sizeof s, &p), c.word));
    }
    bn_pcen_spec s = good;
    s.format = 2;
    EXPECT(refused(check_spec(&s, sizeof s, &p), "unknown PCEN format 2"));
    // F32 does not look at max_value; the edges of the closed ends pass
    s = good, s.format = BN_PCEN_F32, s.max_value = nan, s.smooth = 1.0f, s.alpha = 0.0f, s.delta = 0.0f, s.r = 1.0f;
    EXPECT(check_spec(&s, sizeof s, &p) == BN_OK && p.elem == 4 && p.a == 0.0f);
    // the spec is read through memcpy: an unaligned one is fine
    std::vector<char> raw(sizeof good + 1);
    memcpy(raw.data() + 1, &good, sizeof good);
    EXPECT(check_spec(reinterpret_cast<const bn_pcen_spec *>(raw.data() + 1), sizeof good, &p) == BN_OK);
}

static void sizes() {
    size_t v = 0;
    EXPECT(out_bytes(SIZE_MAX / 4100, 1025, 4, &v) && v == SIZE_MAX / 4100 * 4100 && !out_bytes(SIZE_MAX / 4100 + 1, 1025, 4, &v));
    EXPECT(out_bytes(SIZE_MAX, 1, 1, &v) && v == SIZE_MAX && !out_bytes(SIZE_MAX, 1, 4, &v) && out_bytes(0, 7, 4, &v) && v == 0);
    // pieces: whole chunks within the limit, one chunk where the limit is below one
    EXPECT(piece_frames(CHUNK) == CHUNK && piece_frames(3 * CHUNK + 17) == 3 * CHUNK && piece_frames(5) == CHUNK);
    for (uint32_t rows : {1u, 64u, 65u, 128u, 1025u}) {
        const size_t lim = spectro::piece_frames(rows), p = piece_frames(lim);
        EXPECT(p % CHUNK == 0 && p <= lim && p + CHUNK > lim && p * rows <= (size_t)1 << 26);
    }
    // a call walked in pieces of 2 chunks: the chunks of the pieces are the chunks of the call, in order, the last one partial
    for (size_t n : {(size_t)1, (size_t)CHUNK - 1, (size_t)CHUNK, (size_t)CHUNK + 1, (size_t)3 * CHUNK + 5, (size_t)4 * CHUNK, (size_t)7 * CHUNK + 127}) {
        const size_t piece = piece_frames(2 * CHUNK + 60);
        size_t c_call = 0, frames = 0;
        for (size_t done = 0; done < n; done += piece) {
            const size_t m = n - done < piece ? n - done : piece;
            EXPECT(done % CHUNK == 0);
            for (size_t c = 0; c < chunks(m); c++, c_call++) {
                EXPECT(done + c * CHUNK == c_call * CHUNK && chunk_len(m, c) == chunk_len(n, c_call) && chunk_len(m, c) >= 1);
                frames += chunk_len(m, c);
            }
        }
        EXPECT(c_call == chunks(n) && frames == n && chunk_len(n, chunks(n) - 1) == (n % CHUNK ? n % CHUNK : CHUNK));
    }
    EXPECT(chunks(0) == 0 && chunks(SIZE_MAX) == SIZE_MAX / CHUNK + 1);
    EXPECT(row_blocks(1) == 1 && row_blocks(64) == 1 && row_blocks(65) == 2 && row_blocks(1025) == 17);
}

static void tables() {
    float p[CHUNK + 1], thr[N_THR + 1];
    for (float s : {0.001f, 0.025f, 0.3f, 1.0f}) {
        apow(s, p);
        const double a = 1.0 - (double)s;
        double run = 1.0;
        EXPECT(p[0] == 1.0f);
        for (uint32_t n = 1; n <= CHUNK; n++) {
            run *= a;
            EXPECT(p[n] <= p[n - 1] && std::fabs((double)p[n] - run) <= run * 6e-8 + 1e-45);
        }
        EXPECT(s < 1.0f || p[1] == 0.0f);
    }
    thr[N_THR] = -7.0f;
    EXPECT(refused(thresholds(8.0f, nullptr), "null") && refused(thresholds(0.0f, thr), "max_value") && refused(thresholds(std::numeric_limits<float>::quiet_NaN(), thr), "max_value") &&
           refused(thresholds(std::numeric_limits<float>::infinity(), thr), "max_value"));
    for (float mx : {8.0f, 1e-40f, 3.0e38f}) {
        EXPECT(thresholds(mx, thr) == BN_OK && thr[N_THR] == -7.0f);
        for (uint32_t j = 1; j <= N_THR; j++)
            EXPECT(thr[j - 1] == (float)(((double)j - 0.5) * (double)mx / 255.0) && (j == 1 || thr[j - 1] >= thr[j - 2]) && std::isfinite(thr[j - 1]));
    }
}

int main() {
    refusals();
    sizes();
    tables();
    if (failures) return fprintf(stderr, "asan_pcen_plan: %d failures\n", failures), 1;
    printf("asan_pcen_plan: ok\n");
    return 0;
}
