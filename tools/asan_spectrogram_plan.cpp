// Host-side sanitizer check of the spectrogram's arithmetic (no device, no Python): the refusals of a spec, of a bank and of the two
// designers, the bytes of the output, where a frame starts and the last sample a range reads at extreme n_frames and hop, the frames
// of a launch piece, the LDS figures and the stride the bank-conflict argument needs, the packed bank with each row tile's step
// range, the mel designer and the threshold table (rust-birdnet-onnx_amd/csrc/spectrogram_plan.h), over edge values.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Iinclude -Irust-birdnet-onnx_amd/csrc tools/asan_spectrogram_plan.cpp -o /tmp/asan_spectrogram_plan && /tmp/asan_spectrogram_plan
// Exit 0 and "asan_spectrogram_plan: ok": every refusal came with its message; no size or start wrapped; every packed bank re-sums
// to its weights exactly, with zeros outside each tile's step range; the sixteen lanes of every b128 group fall on sixteen slots;
// nothing read memory it does not own and no arithmetic overflowed.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "spectrogram_plan.h"

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
using namespace bn::spectro;

static float bf16(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// the packed bank against its weights: every tile's steps cover its non-zero columns, the three planes of a packed element re-sum
// to the weight exactly, and everything outside the step range is zero in W
static void check_pack(uint32_t N, size_t rows, const std::vector<float> &w) {
    EXPECT(check_bank(N, rows, w.data()) == BN_OK);
    const PackedBank b = pack_bank(N, rows, w.data());
    const size_t K = N / 2 + 1;
    EXPECT(b.n_tiles == (rows + 15) / 16 && b.n_tiles <= MAX_ROW_TILES);
    uint32_t at = 0;
    for (uint32_t j = 0; j < b.n_tiles; j++) {
        EXPECT(b.tiles.count[j] >= 1 && b.tiles.first[j] + b.tiles.count[j] <= steps(N) && b.tiles.offset[j] == at);
        at += b.tiles.count[j];
        for (size_t m = 16 * (size_t)j; m < 16 * (size_t)(j + 1); m++)
            for (size_t k = 0; k < depth(N); k++) {
                const float want = m < rows && k < K ? w[m * K + k] : 0.0f;
                const size_t s = k / 32;
                if (s < b.tiles.first[j] || s >= b.tiles.first[j] + b.tiles.count[j]) {
                    EXPECT(want == 0.0f);
                    continue;
                }
                const size_t lane = (m % 16) + 16 * ((k % 32) / 8), e = k % 8, base = ((b.tiles.offset[j] + (s - b.tiles.first[j])) * 3 * 64 + lane) * 8 + e;
                EXPECT(bf16(b.image[base]) + bf16(b.image[base + 512]) + bf16(b.image[base + 1024]) == want);
            }
    }
    EXPECT(b.image.size() == (size_t)at * STEP_ELEMS);
}

int main() {
    size_t plans = 0;
    // ---- specs: accepted, from an odd address and exactly their size
    for (uint32_t N : {256u, 512u, 1024u, 2048u})
        for (uint32_t hop : {1u, 100u, N / 2, N})
            for (uint32_t fmt : {0u, 1u}) {
                std::vector<char> raw(sizeof(bn_spectrogram_spec) + 1);
                const bn_spectrogram_spec s{N, hop, 3, N / 2 + 1, fmt, 1.0f, 80.0f}, sb{N, hop, 0, 0, fmt, 0.5f, 60.0f};
                Plan p;
                memcpy(raw.data() + 1, &s, sizeof(s));
                EXPECT(check_spec(reinterpret_cast<const bn_spectrogram_spec *>(raw.data() + 1), sizeof(s), 0, 0, &p) == BN_OK);
                EXPECT(p.N == N && p.hop == hop && p.lo == 3 && p.hi == N / 2 + 1 && p.n_rows == N / 2 - 2 && !p.bank && p.elem == (fmt ? 1u : 4u));
                memcpy(raw.data() + 1, &sb, sizeof(sb));
                EXPECT(check_spec(reinterpret_cast<const bn_spectrogram_spec *>(raw.data() + 1), sizeof(sb) + 8, 256, N, &p) == BN_OK && p.bank && p.n_rows == 256);
                plans++;
            }
    // ---- refusals
    {
        Plan p;
        bn_spectrogram_spec s{1024, 512, 0, 513, 0, 0.0f, 0.0f};
        EXPECT(refused(check_spec(nullptr, sizeof(s), 0, 0, &p), "null spectrogram spec") && refused(check_spec(&s, sizeof(s) - 1, 0, 0, &p), "spec_size"));
        for (uint32_t f : {0u, 255u, 1000u, 4096u, 0xffffffffu}) {
            s.frame = f;
            EXPECT(refused(check_spec(&s, sizeof(s), 0, 0, &p), "frame"));
        }
        s.frame = 1024;
        for (uint32_t hop : {0u, 1025u, 0xffffffffu}) {
            s.hop = hop;
            EXPECT(refused(check_spec(&s, sizeof(s), 0, 0, &p), "hop"));
        }
        s.hop = 512, s.format = 2;
        EXPECT(refused(check_spec(&s, sizeof(s), 0, 0, &p), "format"));
        s.format = 0;
        for (auto [lo, hi] : {std::pair<uint32_t, uint32_t>{10, 10}, {11, 10}, {0, 514}, {0xffffffffu, 0}, {0, 0}}) {
            s.bin_lo = lo, s.bin_hi = hi;
            EXPECT(refused(check_spec(&s, sizeof(s), 0, 0, &p), "bins ["));
        }
        s.bin_lo = 0, s.bin_hi = 513;
        EXPECT(refused(check_spec(&s, sizeof(s), 16, 1024, &p), "must both be 0"));
        s.bin_hi = 0;
        EXPECT(refused(check_spec(&s, sizeof(s), 16, 512, &p), "of frame 512") && check_spec(&s, sizeof(s), 16, 1024, &p) == BN_OK);
        s.format = 1;
        const float inf = __builtin_inff(), nan = __builtin_nanf("");
        for (float v : {0.0f, -1.0f, inf, nan}) {
            s.ref_power = v, s.range_db = 80.0f;
            EXPECT(refused(check_spec(&s, sizeof(s), 16, 1024, &p), "ref_power"));
            s.ref_power = 1.0f, s.range_db = v;
            EXPECT(refused(check_spec(&s, sizeof(s), 16, 1024, &p), "range_db"));
            float thr[N_THR];
            EXPECT(refused(thresholds(v, 80.0f, thr), "ref_power") && refused(thresholds(1.0f, v, thr), "range_db"));
        }
        EXPECT(refused(thresholds(1.0f, 80.0f, nullptr), "null"));
    }
    // ---- sizes, starts and the last sample read: extreme n_frames and hop
    {
        size_t n = 7;
        EXPECT(out_bytes(5, 129, 4, &n) && n == 5 * 129 * 4 && out_bytes(0, 1, 1, &n) && n == 0 && !out_bytes(1, 0, 4, &n));
        EXPECT(out_bytes(SIZE_MAX, 1, 1, &n) && n == SIZE_MAX && !out_bytes(SIZE_MAX, 1, 4, &n) && !out_bytes(SIZE_MAX / 4100 + 1, 1025, 4, &n));
        EXPECT(out_bytes(SIZE_MAX / 4100, 1025, 4, &n) && n / 4100 == SIZE_MAX / 4100);
        const uint64_t big = ~(uint64_t)0;
        EXPECT(frame_start(1000, 0, 0, 2048) == 0 && frame_start(1000, 10, 9, 100) == 910 && frame_start(1000, 10, 10, 100) == 1000);
        EXPECT(frame_start(1000, 1000, 0, 1) == 1000 && frame_start(1000, 1000, big, 2048) == 1000 && frame_start(1000, 0, big, 2048) == 1000);
        EXPECT(frame_start(big, 0, big / 2048, 2048) == big / 2048 * 2048 && frame_start(big, 2048, big / 2048, 2048) == big);
        uint64_t last = 0;
        EXPECT(!last_sample_read(1000, 0, 0, 256, 100, &last) && !last_sample_read(1000, 1000, 5, 256, 100, &last) && !last_sample_read(0, 0, 5, 256, 1, &last));
        EXPECT(last_sample_read(1000, 0, 1, 256, 100, &last) && last == 255 && last_sample_read(1000, 0, 8, 256, 100, &last) && last == 955);
        EXPECT(last_sample_read(1000, 0, 9, 256, 100, &last) && last == 999 && last_sample_read(1000, 0, big, 2048, 2048, &last) && last == 999);
        EXPECT(last_sample_read(big, big - 1, big, 2048, 1, &last) && last == big - 1 && last_sample_read(1000, 999, 1, 256, 256, &last) && last == 999);
        for (uint32_t rows : {1u, 11u, 129u, 256u, 1025u}) {
            const size_t piece = piece_frames(rows);
            EXPECT(piece >= 16 && piece % 16 == 0 && piece <= ((size_t)1 << 24) && piece * rows <= ((size_t)1 << 26));
        }
        EXPECT(piece_frames(0) == (size_t)1 << 24);
    }
    // ---- LDS: the figures, the swizzle of a bins row, the slots of a b128 group
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        const uint32_t M = N / 2;
        EXPECT(depth(N) == M + 32 && steps(N) * 32 == depth(N) && bank_stride(N) >= depth(N) && bank_stride(N) % 8 == 0);
        EXPECT(bins_lds_bytes(N) == HEAD_BYTES + 16 * (M + 1) * 4 && bank_lds_bytes(N) == HEAD_BYTES + 3 * 16 * bank_stride(N) * 2 && bank_lds_bytes(N) <= 160 * 1024);
        std::vector<int> seen(M + 1, 0);
        for (uint32_t k = 0; k <= M; k++) EXPECT(lds_index(N, k) <= M && seen[lds_index(N, k)]++ == 0);
        // lane (i, g) reads byte i * R + 16 g + 64 s; a group is 16 lanes of the wave's lower or upper half
        const uint32_t R = 2 * bank_stride(N);
        const uint32_t groups[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
        for (uint32_t half = 0; half < 2; half++)
            for (const auto &grp : groups)
                for (uint32_t s = 0; s < steps(N); s++) {
                    uint32_t slots = 0;
                    for (uint32_t lane : grp) slots |= 1u << ((((lane & 15) * R + 16 * ((lane >> 4) + 2 * half) + 64 * s) / 16) % 16);
                    EXPECT(slots == 0xffffu);
                }
        plans++;
    }
    // ---- banks: refusals, then packs that re-sum
    {
        std::vector<float> w(2 * 129, 1.0f);
        EXPECT(refused(check_bank(256, 2, nullptr), "null") && refused(check_bank(256, 0, w.data()), "n_rows") && refused(check_bank(256, 257, w.data()), "n_rows"));
        EXPECT(refused(check_bank(300, 2, w.data()), "frame"));
        for (float v : {-1.0f, -0.0f - 1e-30f, __builtin_inff(), __builtin_nanf("")}) {
            w[257] = v;
            EXPECT(refused(check_bank(256, 2, w.data()), "negative or not finite"));
        }
        for (size_t k = 0; k < 129; k++) w[129 + k] = 0.0f;
        EXPECT(refused(check_bank(256, 2, w.data()), "row 1 of the filter bank is all zeros"));
    }
    for (uint32_t N : {256u, 2048u}) {
        const size_t K = N / 2 + 1;
        // a bank whose only weight is on bin N/2: the last step alone
        std::vector<float> top(K, 0.0f);
        top[K - 1] = 0.3f;
        check_pack(N, 1, top);
        EXPECT(pack_bank(N, 1, top.data()).tiles.first[0] == steps(N) - 1 && pack_bank(N, 1, top.data()).tiles.count[0] == 1);
        // 256 rows, each a few bins wide, walking up the spectrum; and a dense one of 17 rows
        std::vector<float> walk(256 * K, 0.0f), dense(17 * K);
        for (size_t m = 0; m < 256; m++)
            for (size_t k = m * (K - 5) / 256; k < m * (K - 5) / 256 + 5; k++) walk[m * K + k] = 1.0f / 3.0f + (float)k * 1e-3f;
        for (size_t i = 0; i < dense.size(); i++) dense[i] = (float)((i * 2654435761u) % 1000) * 1.234e-3f;
        dense[5] = 1.0f;
        check_pack(N, 256, walk);
        check_pack(N, 17, dense);
        EXPECT(pack_bank(N, 17, dense.data()).tiles.count[0] == steps(N) && pack_bank(N, 256, walk.data()).image.size() < (size_t)16 * steps(N) * STEP_ELEMS);
        plans += 3;
    }
    // ---- the mel designer
    {
        std::vector<float> w(256 * 1025, -7.0f);
        EXPECT(refused(mel_bank(0, 1024, 8, 0, 8000, w.data()), "sample_rate") && refused(mel_bank(48000, 1000, 8, 0, 8000, w.data()), "frame"));
        EXPECT(refused(mel_bank(48000, 1024, 0, 0, 8000, w.data()), "n_mels") && refused(mel_bank(48000, 1024, 257, 0, 8000, w.data()), "n_mels"));
        EXPECT(refused(mel_bank(48000, 1024, 8, -1, 8000, w.data()), "fmin_hz") && refused(mel_bank(48000, 1024, 8, 8000, 8000, w.data()), "below fmax_hz"));
        EXPECT(refused(mel_bank(48000, 1024, 8, 0, 24001, w.data()), "half the sample rate") && refused(mel_bank(48000, 1024, 8, __builtin_nan(""), 8000, w.data()), "fmin_hz"));
        EXPECT(refused(mel_bank(48000, 1024, 8, 0, __builtin_nan(""), w.data()), "fmax_hz") && refused(mel_bank(48000, 1024, 8, 0, 8000, nullptr), "null"));
        EXPECT(refused(mel_bank(48000, 256, 128, 0, 24000, w.data()), "triangle 0 holds no bin centre"));
        bool untouched = true;
        for (float v : w) untouched &= v == -7.0f;
        EXPECT(untouched);
        EXPECT(mel_bank(48000, 2048, 128, 0, 24000, w.data()) == BN_OK);
        w.resize(128 * 1025);
        check_pack(2048, 128, w);
        const PackedBank b = pack_bank(2048, 128, w.data());
        uint32_t total = 0;
        for (uint32_t j = 0; j < b.n_tiles; j++) total += b.tiles.count[j];
        EXPECT(b.n_tiles == 8 && total < 2 * steps(2048));  // a few steps per tile, not all 33
        printf("128 mel rows at frame 2048: %u of %u steps packed\n", total, 8 * steps(2048));
        float thr[N_THR];
        EXPECT(thresholds(1.0f, 80.0f, thr) == BN_OK && thr[254] < 1.0f && thr[0] > 1e-8f && thr[0] < 1.1e-8f);
        for (uint32_t j = 1; j < N_THR; j++) EXPECT(thr[j] >= thr[j - 1]);
        EXPECT(thresholds(1e-44f, 1e-3f, thr) == BN_OK);  // denormal powers, a range that rounds many thresholds together
        for (uint32_t j = 1; j < N_THR; j++) EXPECT(thr[j] >= thr[j - 1]);
        plans++;
    }
    printf("%zu plans, %d failures\n", plans, failures);
    if (failures) return 1;
    printf("asan_spectrogram_plan: ok\n");
    return 0;
}
