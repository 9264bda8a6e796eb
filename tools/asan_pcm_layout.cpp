// Host-only check of csrc/pcm_layout.h -- the arithmetic on frames and bytes behind the PCM layouts (recording upload, live pool,
// the kernels' sample read) -- under -fsanitize=address,undefined (Makefile: tools/asan_pcm_layout; tests/test_pcm_layout_cpu.py).
// No device.  For every format x channels 1..16: frame and sample byte offsets against a byte-by-byte walk of a real buffer, the
// asynchronous upload's chunks (each a whole number of frames, together covering the recording exactly once, the "has frame i
// arrived" count agreeing with the bytes a chunk walk has copied) for chunk sizes that no frame divides, ring sizes, and the
// overflow refusals.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pcm_layout.h"

using namespace bn;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

static const int32_t FORMATS[] = {BN_PCM_I16, BN_PCM_F32, BN_PCM_I24, BN_PCM_I32, BN_PCM_U8};
static const uint32_t WIDTH[] = {2, 4, 3, 4, 1};

static void check_layouts() {
    for (int f = 0; f < 5; f++) CHECK(pcm_sample_bytes(FORMATS[f]) == WIDTH[f]);
    CHECK(pcm_sample_bytes(5) == 0 && pcm_sample_bytes(-1) == 0);
    CHECK(pcm_layout_problem(PcmLayout{5, 1, 0}) && pcm_layout_problem(PcmLayout{-1, 1, 0}));
    for (int f = 0; f < 5; f++) {
        CHECK(pcm_layout_problem(PcmLayout{FORMATS[f], 0, 0}));
        CHECK(pcm_layout_problem(PcmLayout{FORMATS[f], 17, 0}));
        CHECK(pcm_layout_problem(PcmLayout{FORMATS[f], 0xffffffffu, BN_PCM_MIX}));
        for (uint32_t ch = 1; ch <= PCM_MAX_CHANNELS; ch++) {
            for (int32_t c = -1; c < (int32_t)ch; c++) CHECK(!pcm_layout_problem(PcmLayout{FORMATS[f], ch, c}));
            CHECK(pcm_layout_problem(PcmLayout{FORMATS[f], ch, (int32_t)ch}));
            CHECK(pcm_layout_problem(PcmLayout{FORMATS[f], ch, -2}));
            CHECK(pcm_layout_problem(PcmLayout{FORMATS[f], ch, INT32_MIN}) && pcm_layout_problem(PcmLayout{FORMATS[f], ch, INT32_MAX}));
        }
    }
    CHECK(pcm_normalised(PcmLayout{BN_PCM_I24, 1, BN_PCM_MIX}).channel == 0);
    CHECK(pcm_normalised(PcmLayout{BN_PCM_I24, 2, BN_PCM_MIX}).channel == BN_PCM_MIX);
    CHECK(pcm_is_plain(PcmLayout{BN_PCM_I16, 1, 0}) && pcm_is_plain(PcmLayout{BN_PCM_F32, 1, 0}));
    CHECK(!pcm_is_plain(PcmLayout{BN_PCM_I16, 2, 0}) && !pcm_is_plain(PcmLayout{BN_PCM_I32, 1, 0}) && !pcm_is_plain(PcmLayout{BN_PCM_U8, 1, 0}));
}

// offsets against a walk over a buffer of exactly pcm_bytes() bytes: the sanitizer sees every byte the offsets name
static void check_offsets() {
    const size_t n_frames = 37;
    for (int f = 0; f < 5; f++)
        for (uint32_t ch = 1; ch <= PCM_MAX_CHANNELS; ch++) {
            const PcmLayout l{FORMATS[f], ch, 0};
            size_t bytes = 0;
            CHECK(pcm_bytes(l, n_frames, &bytes) && bytes == n_frames * ch * WIDTH[f]);
            CHECK(pcm_frame_bytes(l) == (size_t)ch * WIDTH[f]);
            std::vector<unsigned char> buf(bytes, 0);
            size_t walk = 0;
            for (size_t i = 0; i < n_frames; i++) {
                CHECK(pcm_frame_offset(l, i) == walk);
                for (uint32_t c = 0; c < ch; c++) {
                    const size_t o = pcm_sample_offset(l, i, c);
                    CHECK(o == walk);
                    for (uint32_t b = 0; b < WIDTH[f]; b++) buf.data()[o + b]++;
                    walk += WIDTH[f];
                }
            }
            CHECK(walk == bytes);
            for (size_t k = 0; k < bytes; k++) CHECK(buf[k] == 1);  // every byte belongs to exactly one sample
        }
}

// the chunked upload: copy a recording chunk by chunk, as the uploader does, and ask after every chunk which frames have arrived
static void check_chunks() {
    const size_t chunk_bytes_cases[] = {1, 5, 7, 64, 100, 1000, 4096, (size_t)1 << 20};
    for (int f = 0; f < 5; f++)
        for (uint32_t ch = 1; ch <= PCM_MAX_CHANNELS; ch++)
            for (size_t cb : chunk_bytes_cases) {
                const PcmLayout l{FORMATS[f], ch, BN_PCM_MIX};
                const size_t fb = pcm_frame_bytes(l);
                const size_t cf = pcm_chunk_frames(l, cb);
                CHECK(cf >= 1);
                CHECK(cf * fb <= cb || cf == 1);           // within the chunk size, unless one frame alone exceeds it
                CHECK((cf + 1) * fb > cb);                 // and the largest such number of frames
                for (size_t n_frames : {(size_t)0, (size_t)1, cf - 1, cf, cf + 1, 3 * cf - 1, 3 * cf, 3 * cf + 1, (size_t)1003}) {
                    if (n_frames > 200000) continue;
                    const size_t n_chunks = pcm_chunk_count(n_frames, cf);
                    CHECK(n_chunks == (n_frames + cf - 1) / cf);
                    size_t bytes = 0;
                    CHECK(pcm_bytes(l, n_frames, &bytes));
                    std::vector<unsigned char> src(bytes), dst(bytes, 0);
                    for (size_t k = 0; k < bytes; k++) src[k] = (unsigned char)(k * 131 + 7);
                    size_t copied_frames = 0;
                    for (size_t k = 0; k < n_chunks; k++) {
                        const size_t a = k * cf, n = (cf < n_frames - a ? cf : n_frames - a);
                        CHECK(n >= 1 && a == copied_frames);
                        CHECK(pcm_frame_offset(l, a) % fb == 0);  // a chunk starts on a frame boundary
                        memcpy(dst.data() + pcm_frame_offset(l, a), src.data() + pcm_frame_offset(l, a), n * fb);
                        copied_frames += n;
                        // frame i has arrived exactly when the chunks it needs are done
                        const size_t probe[] = {0, a, a + n - 1, a + n, n_frames - 1};
                        for (size_t i : probe) {
                            if (i >= n_frames) continue;
                            const size_t need = pcm_chunks_for_frame(i, cf, n_chunks);
                            CHECK(need >= 1 && need <= n_chunks);
                            CHECK((need <= k + 1) == (i < copied_frames));
                        }
                    }
                    CHECK(copied_frames == n_frames);
                    CHECK(bytes == 0 || memcmp(src.data(), dst.data(), bytes) == 0);
                }
            }
    // a 6-byte frame does not divide 32 MiB: the cut is at a frame boundary all the same
    const PcmLayout st24{BN_PCM_I24, 2, BN_PCM_MIX};
    const size_t cf = pcm_chunk_frames(st24, (size_t)32 << 20);
    CHECK(cf == ((size_t)32 << 20) / 6 && (cf * 6) % 6 == 0 && ((size_t)32 << 20) - cf * 6 == 2);
}

static void check_overflow() {
    size_t out = 12345;
    for (int f = 0; f < 5; f++)
        for (uint32_t ch = 1; ch <= PCM_MAX_CHANNELS; ch++) {
            const PcmLayout l{FORMATS[f], ch, 0};
            const size_t fb = pcm_frame_bytes(l);
            const size_t most = SIZE_MAX / fb;
            CHECK(pcm_bytes(l, most, &out) && out == most * fb);
            out = 12345;
            CHECK(fb == 1 || (!pcm_bytes(l, most + 1, &out) && out == 12345));  // refused, nothing written (1-byte frames: every count fits)
            CHECK(fb == 1 || !pcm_bytes(l, SIZE_MAX, &out));
        }
    CHECK(!pcm_bytes(PcmLayout{7, 1, 0}, 1, &out));  // an unknown format has no frame size
    CHECK(pcm_ring_bytes(3, 1000, 4, &out) && out == 12000);
    out = 12345;
    CHECK(!pcm_ring_bytes(3, SIZE_MAX / 4 + 1, 4, &out) && out == 12345);
    CHECK(!pcm_ring_bytes(SIZE_MAX / 2, 1000, 4, &out) && out == 12345);
    CHECK(!pcm_ring_bytes(0, 1000, 4, &out) && !pcm_ring_bytes(3, 1000, 0, &out));
    CHECK(pcm_ring_bytes(1, SIZE_MAX / 4, 4, &out) && out == SIZE_MAX / 4 * 4);
}

int main() {
    check_layouts();
    check_offsets();
    check_chunks();
    check_overflow();
    printf("asan_pcm_layout: ok\n");
    return 0;
}
