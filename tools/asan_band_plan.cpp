// Host-side sanitizer check of the band levels' arithmetic (no device, no Python): the refusals of a spec, the frames of a window and
// the unread tail, the last sample a window range reads computed without a sum or product that wraps, the bins of a band given in
// hertz, the LDS figure and the tables (rust-birdnet-onnx_amd/csrc/band_plan.h), over edge values.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       tools/asan_band_plan.cpp -o /tmp/asan_band_plan && /tmp/asan_band_plan
// Exit 0 and "asan_band_plan: ok": every refusal came with its message; every accepted plan covers [0, span) with span <= S and fewer
// than hop positions unread; the last sample read lies inside the recording and inside the last window's frames; a band's bins are
// exactly those whose centres lie in it; the tables hold the window and the twiddles of the rule; nothing read memory it does not
// own and no arithmetic overflowed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "band_plan.h"

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
using namespace bn::band;

static bn_band_spec spec_of(uint32_t frame, uint32_t hop, uint32_t n_bands) {
    bn_band_spec s{};
    s.frame = frame, s.hop = hop, s.n_bands = n_bands;
    for (uint32_t b = 0; b < BN_BAND_MAX; b++) s.bin_lo[b] = b, s.bin_hi[b] = frame / 2 + 1 - b;
    return s;
}

int main() {
    size_t plans = 0;
    // ---- accepted specs: frames, span and the unread tail
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        for (uint32_t hop : {1u, 7u, 100u, N / 2, N - 1, N}) {
            for (uint64_t S : {(uint64_t)N, (uint64_t)N + 1, (uint64_t)N + hop, (uint64_t)4096, (uint64_t)144000, (uint64_t)0xfffffffcull}) {
                if (S < N) continue;
                // the spec on the heap, exactly its size and at an odd address: a read past it or an aligned read is caught
                std::vector<char> raw(sizeof(bn_band_spec) + 1);
                const bn_band_spec s = spec_of(N, hop, 1 + (uint32_t)(S % BN_BAND_MAX));
                memcpy(raw.data() + 1, &s, sizeof(s));
                Plan p;
                EXPECT(check_spec(reinterpret_cast<const bn_band_spec *>(raw.data() + 1), sizeof(bn_band_spec), S, &p) == BN_OK);
                EXPECT(p.N == N && p.hop == hop && p.n_bands == s.n_bands && p.n_frames >= 1);
                EXPECT((uint64_t)p.n_frames == (S - N) / hop + 1);
                EXPECT((uint64_t)p.span == (uint64_t)(p.n_frames - 1) * hop + N && p.span <= S && (uint64_t)p.unread == S - p.span && p.unread < hop);
                for (uint32_t b = 0; b < BN_BAND_MAX; b++) EXPECT(b < p.n_bands ? (p.lo[b] == s.bin_lo[b] && p.hi[b] == s.bin_hi[b]) : (p.lo[b] == 0 && p.hi[b] == 0));
                plans++;
            }
        }
    }
    {
        Plan p;
        const bn_band_spec a = spec_of(1024, 512, 2), b = spec_of(256, 100, 1), c = spec_of(256, 256, 1);
        EXPECT(check_spec(&a, sizeof(a), 144000, &p) == BN_OK && p.n_frames == 280 && p.unread == 128);
        EXPECT(check_spec(&b, sizeof(b), 4096, &p) == BN_OK && p.n_frames == 39 && p.unread == 40);
        EXPECT(check_spec(&c, sizeof(c), 256, &p) == BN_OK && p.n_frames == 1 && p.unread == 0);
        EXPECT(check_spec(&a, sizeof(a) + 8, 144000, &p) == BN_OK);  // a longer struct of a later header
    }
    // ---- refusals
    {
        Plan p;
        bn_band_spec s = spec_of(1024, 512, 2);
        EXPECT(refused(check_spec(nullptr, sizeof(s), 4096, &p), "null band spec"));
        EXPECT(refused(check_spec(&s, sizeof(s) - 1, 4096, &p), "spec_size"));
        EXPECT(refused(check_spec(&s, 0, 4096, &p), "spec_size"));
        for (uint32_t f : {0u, 1u, 128u, 255u, 257u, 1000u, 4096u, 0xffffffffu}) {
            s = spec_of(1024, 512, 2), s.frame = f;
            EXPECT(refused(check_spec(&s, sizeof(s), 144000, &p), "frame"));
        }
        s = spec_of(1024, 512, 2);
        EXPECT(refused(check_spec(&s, sizeof(s), 1023, &p), "below the frame") && refused(check_spec(&s, sizeof(s), 0, &p), "below the frame"));
        EXPECT(refused(check_spec(&s, sizeof(s), (uint64_t)1 << 32, &p), "2^32") && refused(check_spec(&s, sizeof(s), UINT64_MAX, &p), "2^32"));
        s.hop = 0;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "hop"));
        s.hop = 1025;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "hop"));
        s.hop = 0xffffffffu;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "hop"));
        s = spec_of(1024, 512, 0);
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "n_bands"));
        s.n_bands = BN_BAND_MAX + 1;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "n_bands"));
        s.n_bands = 0xffffffffu;  // no band past the array is read
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "n_bands"));
        s = spec_of(1024, 512, 3);
        s.bin_lo[2] = 10, s.bin_hi[2] = 10;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "band 2"));
        s.bin_lo[2] = 11;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "band 2"));
        s.bin_lo[2] = 0, s.bin_hi[2] = 514;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "band 2"));
        s.bin_hi[2] = 513;
        EXPECT(check_spec(&s, sizeof(s), 4096, &p) == BN_OK && p.hi[2] == 513);
        s.bin_lo[1] = 0xffffffffu, s.bin_hi[1] = 0;
        EXPECT(refused(check_spec(&s, sizeof(s), 4096, &p), "band 1"));
    }
    // ---- the last sample a range reads
    {
        const uint64_t MAX = UINT64_MAX;
        uint64_t last = 0;
        // a recording of 10, windows at step 4 (0, 4, 8), span 6
        EXPECT(last_sample_read(10, 0, 4, 6, &last) && last == 5);
        EXPECT(last_sample_read(10, 1, 4, 6, &last) && last == 9);
        EXPECT(last_sample_read(10, 2, 4, 6, &last) && last == 9);
        EXPECT(!last_sample_read(10, 3, 4, 6, &last));
        EXPECT(!last_sample_read(0, 0, 4, 6, &last) && !last_sample_read(10, 0, 0, 6, &last) && !last_sample_read(10, 0, 4, 0, &last));
        // the edges of uint64: neither the product nor start + span may wrap
        EXPECT(last_sample_read(MAX, MAX - 1, 1, 0xffffffffull, &last) && last == MAX - 1);
        EXPECT(last_sample_read(MAX, 0, MAX, 0xffffffffull, &last) && last == 0xfffffffeull);
        EXPECT(!last_sample_read(MAX, 2, MAX - 1, 4, &last) && !last_sample_read(MAX, MAX, MAX, 4, &last) && !last_sample_read(MAX, MAX, 2, 4, &last));
        EXPECT(last_sample_read(MAX, 1, MAX - 1, 4, &last) && last == MAX - 1);
        EXPECT(last_sample_read(MAX, (MAX - 1) / 3, 3, 1024, &last) && last < MAX && last >= (MAX - 1) / 3 * 3);
        for (uint64_t n : {(uint64_t)1, (uint64_t)255, (uint64_t)256, (uint64_t)100000}) {
            for (uint64_t step : {(uint64_t)1, (uint64_t)100, (uint64_t)4096}) {
                for (uint64_t span : {(uint64_t)256, (uint64_t)4000}) {
                    const uint64_t total = (n + step - 1) / step;
                    for (uint64_t k : {(uint64_t)0, total / 2, total - 1}) {
                        EXPECT(last_sample_read(n, k, step, span, &last));
                        EXPECT(last < n && last >= k * step && last - k * step < span);
                        EXPECT(last == n - 1 || last - k * step == span - 1);
                    }
                    EXPECT(!last_sample_read(n, total, step, span, &last));
                }
            }
        }
    }
    // ---- the bins of a band in hertz
    {
        uint32_t lo = 99, hi = 99;
        EXPECT(bins(48000, 1024, 2000.0, 10000.0, &lo, &hi) == BN_OK && lo == 43 && hi == 214);
        EXPECT(bins(48000, 1024, 0.0, 24000.0, &lo, &hi) == BN_OK && lo == 0 && hi == 512);     // the centre of bin 512 is 24000: outside
        EXPECT(bins(48000, 1024, -5.0, 1e300, &lo, &hi) == BN_OK && lo == 0 && hi == 513);
        EXPECT(bins(48000, 1024, 46.875, 93.75, &lo, &hi) == BN_OK && lo == 1 && hi == 2);     // a centre at lo belongs, one at hi does not
        EXPECT(bins(48000, 1024, 46.874, 93.751, &lo, &hi) == BN_OK && lo == 1 && hi == 3);
        EXPECT(bins(0xffffffffu, 256, 0.0, 1.0, &lo, &hi) == BN_OK && lo == 0 && hi == 1);
        EXPECT(bins(1, 2048, 0.4, 0.5, &lo, &hi) == BN_OK && lo == 820 && hi == 1024);
        for (uint32_t rate : {8000u, 22050u, 44100u, 48000u, 192000u}) {
            for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
                for (double a : {0.0, 60.0, 1999.9, 2000.0, 11025.0}) {
                    for (double w : {1.0, 50.0, 3000.0, 1e9}) {
                        const bn_status st = bins(rate, N, a, a + w, &lo, &hi);
                        uint32_t first = 0, n_in = 0;
                        for (uint32_t k = 0; k <= N / 2; k++) {
                            const double c = (double)k * rate / N;
                            if (c >= a && c < a + w && n_in++ == 0) first = k;
                        }
                        if (n_in == 0) EXPECT(refused(st, "no bin centre"));
                        else EXPECT(st == BN_OK && lo == first && hi == first + n_in);
                        plans++;
                    }
                }
            }
        }
        lo = hi = 77;
        EXPECT(refused(bins(0, 1024, 1.0, 2.0, &lo, &hi), "sample_rate") && refused(bins(48000, 1000, 1.0, 2.0, &lo, &hi), "frame"));
        EXPECT(refused(bins(48000, 1024, 2.0, 2.0, &lo, &hi), "lo_hz") && refused(bins(48000, 1024, 3.0, 2.0, &lo, &hi), "lo_hz"));
        EXPECT(refused(bins(48000, 1024, std::nan(""), 2.0, &lo, &hi), "lo_hz") && refused(bins(48000, 1024, 1.0, std::nan(""), &lo, &hi), "lo_hz"));
        EXPECT(refused(bins(48000, 1024, 10.0, 20.0, &lo, &hi), "no bin centre") && refused(bins(48000, 1024, 24000.5, 30000.0, &lo, &hi), "no bin centre"));
        EXPECT(refused(bins(48000, 1024, -20.0, -10.0, &lo, &hi), "no bin centre"));
        EXPECT(refused(bins(48000, 1024, 1.0, 2000.0, nullptr, &hi), "null") && refused(bins(48000, 1024, 1.0, 2000.0, &lo, nullptr), "null"));
        EXPECT(lo == 77 && hi == 77);  // a refusal writes nothing
    }
    // ---- LDS and the tables: exactly table_floats(N) floats are written
    for (uint32_t N : {256u, 512u, 1024u, 2048u}) {
        EXPECT(lds_bytes(N) == 4 * (2 * 9 * 4 + 4) && lds_bytes(N) <= 65536);
        std::vector<float> tab(table_floats(N));
        const float scale = fill_tables(N, tab.data());
        EXPECT(tab[0] == 0.0f && tab[N / 2] == 1.0f && tab[N / 4] == 0.5f);
        double s2 = 0;
        for (uint32_t n = 0; n < N; n++) {
            EXPECT(tab[n] >= 0.0f && tab[n] <= 1.0f && (n == 0 || tab[n] == tab[N - n]));
            s2 += (double)tab[n] * tab[n];
        }
        EXPECT(std::fabs(s2 - 0.375 * N) < 1e-4 * N && std::fabs((double)scale * N * 0.375 * N - 1.0) < 1e-6);
        EXPECT(tab[N] == 1.0f && tab[N + 1] == 0.0f && tab[N + 2 * (N / 4)] == 0.0f && tab[N + 2 * (N / 4) + 1] == -1.0f);
        for (uint32_t k = 0; k < N / 2; k++) {
            const double c = tab[N + 2 * k], s = tab[N + 2 * k + 1];
            EXPECT(std::fabs(c * c + s * s - 1.0) < 3e-7 && s <= 0.0);
        }
        plans++;
    }
    printf("%zu plans, %d failures\n", plans, failures);
    if (failures) return 1;
    printf("asan_band_plan: ok\n");
    return 0;
}
