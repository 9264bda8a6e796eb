// Host-side sanitizer check of the noise reduction's arithmetic (no device, no Python): the refusals of a spec and a noise estimate,
// the blocks each wave owns, where every (frame, register, lane) position the kernel reads or stores lies, the register shift, the
// window table and bn_noise_floor's selection (rust-birdnet-onnx_amd/csrc/denoise_plan.h), at every frame length over ragged lengths.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_denoise_plan.cpp -o /tmp/asan_denoise_plan && /tmp/asan_denoise_plan
// Exit 0 and "asan_denoise_plan: ok": every refusal came with its message; the waves' runs partition the blocks in order; walking the
// kernel's loops, every sample of [0, n) is read into the two frames the rule names at the positions the rule names and nothing
// outside [0, n) is, every output sample is stored exactly once, from the block that holds it; the register shift holds for every
// register and lane; the window's squares add to 1 at hop N / 2; nothing read memory it does not own and no arithmetic overflowed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "denoise_plan.h"

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
using namespace bn::denoise;

// the kernel's loops over a recording of n samples, on the host: which source sample lands at which (frame, position), which output
// sample each store writes
static void walk(uint32_t N, uint64_t n) {
    const uint32_t H = N / 2, RR = N / 128, HR = RR / 2;
    const uint64_t B = n_blocks(n, N), groups = n_groups(n, N);
    EXPECT(B * H >= n && (B == 0 || (B - 1) * H < n) && groups * WAVES * RUN >= B && (groups == 0 || (groups - 1) * WAVES * RUN < B));
    std::vector<uint8_t> reads(n * 2, 0);  // sample i: bit per frame parity it was read into, counted per (i, frame i / H + {0, 1})
    std::vector<uint8_t> stores(n, 0);
    uint64_t next = 0;
    for (uint64_t g = 0; g < groups; g++)
        for (uint32_t w = 0; w < WAVES; w++) {
            uint64_t b0 = ~0ull, b1 = ~0ull;
            wave_blocks(B, g, w, &b0, &b1);
            EXPECT(b0 == next && b1 >= b0 && b1 <= B && b1 - b0 <= RUN);
            next = b1;
            if (b0 >= b1) continue;
            for (uint64_t f = b0; f <= b1; f++)
                for (uint32_t r = 0; r < RR; r++)
                    for (uint32_t lane = 0; lane < 64; lane++)
                        for (uint32_t c = 0; c < 2; c++) {
                            const uint32_t p = frame_pos(r, lane) + c;
                            EXPECT(p < N);
                            // the kernel reads the first half only for its first frame and the second half for every frame; the
                            // moved-down registers hold what the shift identity says
                            uint64_t at = 0;
                            const bool in = source_of(f, H, p, &at);
                            if (r < HR) {
                                if (f == b0) EXPECT(in == (b0 > 0) && (!in || at == (b0 - 1) * H + p));
                            } else {
                                EXPECT(in && at == f * H + frame_pos(r - HR, lane) + c && shift_holds(N, r, lane));
                            }
                            if (in && at < n) {
                                // frame f covers [(f - 1) H, (f + 1) H): at / H is f - 1 or f
                                EXPECT(at / H + 1 == f || at / H == f);
                                reads[2 * at + (at / H == f ? 0 : 1)] |= 1;
                            }
                            // stores: the head of frame f completes block f - 1
                            if (r < HR && f > b0) {
                                uint64_t first = 0;
                                const uint32_t cnt = store_count(n, f - 1, H, r, lane, &first);
                                EXPECT(first / H == f - 1 && first % H == frame_pos(r, lane) && cnt <= 2 && (cnt == 0 || first + cnt <= n));
                                if (c < cnt) stores[first + c]++;
                            }
                        }
        }
    EXPECT(next == B);
    for (uint64_t i = 0; i < n; i++) EXPECT(reads[2 * i] == 1 && reads[2 * i + 1] == 1 && stores[i] == 1);
}

int main() {
    // ---- spec and noise
    std::vector<float> noise(1025, 1.0f), a;
    Plan plan;
    bn_denoise_spec s{512, 2.0f, 0.1f};
    EXPECT(check_spec(&s, sizeof(s), noise.data(), &plan, &a) == BN_OK && plan.N == 512 && plan.H == 256 && a.size() == 257 && a[256] == 2.0f);
    EXPECT(refused(check_spec(nullptr, sizeof(s), noise.data(), &plan, &a), "null denoise spec"));
    EXPECT(refused(check_spec(&s, sizeof(s) - 1, noise.data(), &plan, &a), "spec_size"));
    EXPECT(refused(check_spec(&s, sizeof(s), nullptr, &plan, &a), "null noise"));
    for (uint32_t frame : {0u, 128u, 300u, 4096u}) {
        bn_denoise_spec b = s;
        b.frame = frame;
        EXPECT(refused(check_spec(&b, sizeof(b), noise.data(), &plan, &a), "frame"));
    }
    for (float v : {-1.0f, INFINITY, NAN}) {
        bn_denoise_spec b = s;
        b.alpha = v;
        EXPECT(refused(check_spec(&b, sizeof(b), noise.data(), &plan, &a), "alpha"));
        b = s, b.floor_gain = v;
        EXPECT(refused(check_spec(&b, sizeof(b), noise.data(), &plan, &a), "floor_gain"));
        std::vector<float> bad(257, 1.0f);
        bad[256] = v;
        EXPECT(refused(check_spec(&s, sizeof(s), bad.data(), &plan, &a), "noise[256]"));
    }
    {  // an unaligned spec and noise; a product that overflows f32 gates the bin
        std::vector<char> raw(sizeof(s) + 1 + 257 * sizeof(float) + 1);
        memcpy(raw.data() + 1, &s, sizeof(s));
        std::vector<float> big(257, 3e38f);
        memcpy(raw.data() + 1 + sizeof(s) + 1, big.data(), 257 * sizeof(float));  // offset sizeof(s) + 2: not a multiple of 4
        EXPECT(check_spec(reinterpret_cast<const bn_denoise_spec *>(raw.data() + 1), sizeof(s), reinterpret_cast<const float *>(raw.data() + sizeof(s) + 2), &plan, &a) == BN_OK &&
               std::isinf(a[0]));
    }
    // ---- geometry
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        const uint64_t H = N / 2, W = (uint64_t)WAVES * RUN * H;
        for (uint32_t r = 0; r < N / 128; r++)
            for (uint32_t lane = 0; lane < 64; lane++) EXPECT(shift_holds(N, r, lane) == (r >= N / 256));
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)2, H - 1, H, H + 1, 2 * H, RUN * H - 1, RUN * H, RUN * H + 1, W - 1, W, W + 1, W + RUN * H + 2, 2 * W + H + 3}) walk(N, n);
        // the far end: no wrap up to N_MAX
        EXPECT(n_blocks(N_MAX, N) == N_MAX / H && n_groups(N_MAX, N) > GRID_MAX);
        uint64_t b0, b1;
        wave_blocks(n_blocks(N_MAX, N), n_groups(N_MAX, N) - 1, WAVES - 1, &b0, &b1);
        EXPECT(b1 == n_blocks(N_MAX, N) && b1 - b0 == RUN);
        // ---- the window: exact ends, squares adding to 1 at hop N / 2, the scale 2 / N^2
        std::vector<float> tab(table_floats(N));
        const float scale = fill_tables(N, tab.data());
        EXPECT(tab[0] == 0.0f && tab[N / 2] == 1.0f && scale == 2.0f / ((float)N * (float)N));
        for (uint32_t j = 0; j < N / 2; j++) EXPECT(std::fabs((double)tab[j] * tab[j] + (double)tab[j + N / 2] * tab[j + N / 2] - 1.0) < 3e-7 && tab[j] <= tab[j + 1]);
    }
    // ---- bn_noise_floor
    {
        const size_t count = 5, bins = 3;
        std::vector<float> pl(count * BN_PROFILE_PLANES * bins, -7.0f), out(bins, 9.0f);
        const float col[5] = {4.0f, INFINITY, 1.0f, 3.0f, 2.0f};
        for (size_t i = 0; i < count; i++)
            for (size_t k = 0; k < bins; k++) pl[i * BN_PROFILE_PLANES * bins + k] = col[i] + (float)k;
        const double qs[] = {0.0, 0.24, 0.25, 0.5, 0.76, 1.0};
        const float want[] = {1.0f, 1.0f, 2.0f, 3.0f, 4.0f, INFINITY};
        for (int i = 0; i < 6; i++) {
            EXPECT(noise_floor(pl.data(), count, bins, qs[i], out.data()) == BN_OK);
            for (size_t k = 0; k < bins; k++) EXPECT(out[k] == want[i] + (float)k);
        }
        out.assign(bins, 9.0f);
        EXPECT(refused(noise_floor(pl.data(), 0, bins, 0.5, out.data()), "count"));
        EXPECT(refused(noise_floor(pl.data(), count, 0, 0.5, out.data()), "n_bins"));
        EXPECT(refused(noise_floor(pl.data(), count, bins, -0.1, out.data()), "quantile"));
        EXPECT(refused(noise_floor(pl.data(), count, bins, NAN, out.data()), "quantile"));
        EXPECT(refused(noise_floor(nullptr, count, bins, 0.5, out.data()), "null"));
        EXPECT(refused(noise_floor(pl.data(), count, bins, 0.5, nullptr), "null"));
        EXPECT(refused(noise_floor(pl.data(), SIZE_MAX / 8, bins, 0.5, out.data()), "do not fit"));
        pl[BN_PROFILE_PLANES * bins + 1] = NAN;
        EXPECT(refused(noise_floor(pl.data(), count, bins, 0.5, out.data()), "NaN"));
        EXPECT(out[0] == 9.0f && out[1] == 9.0f && out[2] == 9.0f);  // a refusal writes nothing
    }
    if (failures) {
        fprintf(stderr, "asan_denoise_plan: %d failures\n", failures);
        return 1;
    }
    printf("asan_denoise_plan: ok\n");
    return 0;
}
