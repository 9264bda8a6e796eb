// Host-side sanitizer check of template matching's arithmetic (no device, no Python): the refusals of a set and its caps, the output
// and image sizes at extreme n_offsets and where a piece starts at extreme first_sample, the launch pieces and their overlap, the
// packed A operand against a direct index formula with every template's K, T1 and dT, the B operand's walk through LDS against the
// division it replaces (and inside the image's rows), and bn_template_peaks (rust-birdnet-onnx_amd/csrc/template_plan.h).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/asan_template_plan.cpp -o /tmp/asan_template_plan && /tmp/asan_template_plan
// Exit 0 and "asan_template_plan: ok": every refusal came with its message; no size wrapped; the emulated product of the packed
// operand with the walked image equals the rule's sum; nothing read memory it does not own and no arithmetic overflowed.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "template_plan.h"

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
using namespace bn::tmatch;

static uint32_t rnd(uint32_t &s) { return (s = s * 1664525u + 1013904223u) >> 8; }

static void refusals() {
    std::vector<uint8_t> codes((size_t)BN_TEMPLATE_MAX_ELEMS * 2, 0);
    for (size_t i = 0; i < BN_TEMPLATE_MAX_ELEMS; i++) codes[i] = (uint8_t)(i * 7);
    std::vector<uint32_t> one(BN_TEMPLATE_MAX_COUNT + 1, 1);
    Packed p;
    uint32_t f2[2] = {2, 2}, f0[1] = {0}, f129[1] = {129}, fmax[2] = {128, 128};
    EXPECT(refused(pack(1, 4, nullptr, codes.data(), &p), "null") && refused(pack(1, 4, f2, nullptr, &p), "null") && refused(pack(1, 4, f2, codes.data(), nullptr), "null"));
    EXPECT(refused(pack(0, 4, f2, codes.data(), &p), "n_templates 0") && refused(pack(65, 4, one.data(), codes.data(), &p), "n_templates 65"));
    EXPECT(refused(pack(1, 0, f2, codes.data(), &p), "n_rows 0") && refused(pack(1, 513, f2, codes.data(), &p), "n_rows 513"));
    EXPECT(refused(pack(1, 4, f0, codes.data(), &p), "template 0 has 0 frames") && refused(pack(1, 4, f129, codes.data(), &p), "129 frames"));
    EXPECT(refused(pack(2, 512, fmax, codes.data(), &p), "template 1 is flat"));  // the full cap is read, the second one is zeros
    EXPECT(refused(pack(1, 1, one.data(), codes.data() + 1, &p), "template 0 is flat"));  // one element: dT == 0 by the rule
    EXPECT(pack(1, 512, fmax, codes.data(), &p) == BN_OK && p.meta[0].K == BN_TEMPLATE_MAX_ELEMS && p.tiles.count[0] == 1024 && p.image.size() == (size_t)1 << 20);
}

static void sizes() {
    size_t v = 0;
    EXPECT(out_floats(64, SIZE_MAX / 64, &v) && v == SIZE_MAX / 64 * 64 && !out_floats(64, SIZE_MAX / 64 + 1, &v) && !out_floats(2, (size_t)1 << 63, &v));
    EXPECT(out_floats(1, SIZE_MAX, &v) && v == SIZE_MAX && out_floats(3, 0, &v) && v == 0 && !out_floats(0, 5, &v));
    EXPECT(image_frames(SIZE_MAX - 127, 128, &v) && v == SIZE_MAX && !image_frames(SIZE_MAX - 126, 128, &v) && image_frames(0, 1, &v) && v == 0);
    // pieces: whole tiles, the image of a piece is one launch of the spectrogram, consecutive pieces share wmax - 1 frames
    for (uint32_t R : {1u, 15u, 16u, 80u, 128u, 512u})
        for (uint32_t W : {1u, 2u, 64u, 128u})
            for (uint32_t n : {1u, 16u, 17u, 64u}) {
                const size_t p = piece_offsets(R, W, n);
                EXPECT(p >= TILE_OFFSETS && p % TILE_OFFSETS == 0 && p + piece_overlap(W) <= spectro::piece_frames(R) && p * n <= (size_t)1 << 26);
                EXPECT((p + piece_overlap(W)) * R <= (size_t)1 << 26 && (p + TILE_OFFSETS - 1) / TILE_OFFSETS <= (size_t)1 << 20);
            }
    // where a piece starts: first_sample + done * hop, saturated, never wrapped
    EXPECT(spectro::frame_start(UINT64_MAX, UINT64_MAX - 5, 3, 2) == UINT64_MAX && spectro::frame_start(1000, 10, 4, 100) == 410);
    EXPECT(spectro::frame_start(UINT64_MAX, 0, UINT64_MAX, 2048) == UINT64_MAX && spectro::frame_start(1000, 1000, 0, 1) == 1000);
}

// pack random sets, compare every byte with the index formula, then run the kernel's product on the host: A fragments times the
// bytes the walk reads from an LDS-shaped image
static void packed_and_walked(uint32_t R, const std::vector<uint32_t> &frames, uint32_t seed) {
    size_t total = 0;
    for (uint32_t W : frames) total += (size_t)W * R;
    std::vector<uint8_t> codes(total);
    for (auto &c : codes) c = (uint8_t)rnd(seed);
    Packed p;
    EXPECT(pack(frames.size(), R, frames.data(), codes.data(), &p) == BN_OK);
    const uint32_t U = units(R), st = stride(R), rows = lds_rows(p.max_frames);
    EXPECT(st % 64 == 32 && st >= U * UNIT && p.n_tiles == (frames.size() + 15) / 16 && p.meta.size() == 16 * p.n_tiles);
    std::vector<int8_t> lds((size_t)rows * st, 0);  // exactly the kernel's rows: a read outside them is the sanitizer's to report
    for (uint32_t r = 0; r < sum_rows(p.max_frames); r++)
        for (uint32_t j = 0; j < R; j++) lds[(size_t)r * st + j] = (int8_t)(rnd(seed) ^ 0x80);
    size_t at = 0;
    for (size_t q = 0; q < frames.size(); at += (size_t)frames[q] * R, q++) {
        const uint32_t j = (uint32_t)q / 16, i = (uint32_t)q % 16, W = frames[q];
        int64_t T1 = 0, T2 = 0;
        for (size_t e = 0; e < (size_t)W * R; e++) T1 += (int)codes[at + e] - 128, T2 += ((int)codes[at + e] - 128) * ((int)codes[at + e] - 128);
        EXPECT(p.meta[q].frames == W && p.meta[q].K == W * R && p.meta[q].T1 == T1 && p.meta[q].dT == (int64_t)W * R * T2 - T1 * T1);
        EXPECT(p.tiles.count[j] >= steps(W, R) && p.tiles.count[j] <= steps(p.max_frames, R));
        for (uint32_t off : {0u, 17u, TILE_OFFSETS - 1}) {
            int64_t got = 0, want = 0;
            for (uint32_t g = 0; g < 4; g++) {
                UnitWalk walk(off, g, U, st);
                for (uint32_t s = 0; s < p.tiles.count[j]; s++, walk.next()) {
                    const uint32_t u = 4 * s + g;
                    EXPECT(walk.addr == (off + u / U) * st + (u % U) * UNIT && walk.addr + UNIT <= lds.size());
                    const uint8_t *a = &p.image[((size_t)(p.tiles.offset[j] + s) * 64 + 16 * g + i) * UNIT];
                    for (uint32_t e = 0; e < UNIT; e++) {
                        const uint32_t w = u / U, row = (u % U) * UNIT + e;
                        EXPECT(a[e] == (w < W && row < R ? (uint8_t)(codes[at + (size_t)w * R + row] ^ 0x80) : 0));
                        got += (int64_t)(int8_t)a[e] * lds[walk.addr + e];
                    }
                }
            }
            for (uint32_t w = 0; w < W; w++)
                for (uint32_t r = 0; r < R; r++) want += ((int64_t)codes[at + (size_t)w * R + r] - 128) * lds[(size_t)(off + w) * st + r];
            EXPECT(got == want);
        }
    }
    for (size_t q = frames.size(); q < p.meta.size(); q++) EXPECT(p.meta[q].K == 0 && p.meta[q].frames == 0);
}

static void peak_rule() {
    const float nan = __builtin_nanf("");
    const float s[2][8] = {{0.9f, 0.9f, 0.1f, nan, 0.5f, 0.4f, 0.95f, 0.95f}, {nan, nan, nan, nan, nan, nan, nan, 0.3f}};
    Hit out[16];
    size_t n = 0;
    EXPECT(peaks(&s[0][0], 2, 8, 0.3f, 1, out, 16, sizeof(Hit), &n) == BN_OK && n == 4);
    EXPECT(out[0].offset == 0 && out[1].offset == 4 && out[2].offset == 6 && out[3].offset == 7 && out[3].template_index == 1 && out[3].score == 0.3f);
    EXPECT(peaks(&s[0][0], 2, 8, 0.3f, 0, out, 16, sizeof(Hit), &n) == BN_OK && n == 7);  // radius 0: everything at or above min_score
    EXPECT(peaks(&s[0][0], 2, 8, 0.3f, SIZE_MAX, out, 16, sizeof(Hit), &n) == BN_OK && n == 2 && out[0].offset == 6);  // a radius past any row
    char wide[2 * 24];
    memset(wide, 0x5A, sizeof(wide));
    EXPECT(peaks(&s[0][0], 2, 8, 0.3f, 1, wide, 2, 24, &n) == BN_OK && n == 4 && wide[16] == 0x5A && wide[47] == 0x5A);  // cap below the total, a longer struct
    EXPECT(peaks(&s[0][0], 2, 0, 0.3f, 1, out, 16, sizeof(Hit), &n) == BN_OK && n == 0 && peaks(nullptr, 0, 8, 0.3f, 1, nullptr, 0, sizeof(Hit), &n) == BN_OK);
    EXPECT(refused(peaks(nullptr, 2, 8, 0.3f, 1, out, 16, sizeof(Hit), &n), "null") && refused(peaks(&s[0][0], 2, 8, 0.3f, 1, nullptr, 16, sizeof(Hit), &n), "null"));
    EXPECT(refused(peaks(&s[0][0], 2, 8, 0.3f, 1, out, 16, sizeof(Hit), nullptr), "null") && refused(peaks(&s[0][0], 2, 8, 0.3f, 1, out, 16, sizeof(Hit) - 1, &n), "struct_size"));
    EXPECT(refused(peaks(&s[0][0], 2, 8, nan, 1, out, 16, sizeof(Hit), &n), "NaN"));
    static_assert(sizeof(Hit) == sizeof(bn_template_hit) && sizeof(Hit) == 16, "the header's struct");
}

int main() {
    refusals();
    sizes();
    packed_and_walked(1, {2, 5, 128}, 1);
    packed_and_walked(15, {1, 40, 7}, 2);
    packed_and_walked(17, {3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 9, 1}, 3);  // a second tile that is longer than the first
    packed_and_walked(48, {1, 2, 3, 128}, 4);
    packed_and_walked(80, {33, 1}, 5);
    packed_and_walked(512, {128, 1, 127}, 6);
    peak_rule();
    if (failures) return fprintf(stderr, "asan_template_plan: %d failures\n", failures), 1;
    printf("asan_template_plan: ok\n");
    return 0;
}
