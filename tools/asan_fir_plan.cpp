// Host-side sanitizer check of the FIR filter's arithmetic (no device, no Python): the refusals of a tap list and of a design, the
// designer at its extreme arguments, the chunk geometry, and the packed Toeplitz operand (rust-birdnet-onnx_amd/csrc/fir_plan.h).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Irust-birdnet-onnx_amd/csrc \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/asan_fir_plan.cpp -o /tmp/asan_fir_plan && /tmp/asan_fir_plan
// Exit 0 and "asan_fir_plan: ok": every refusal came with its message and wrote nothing; every design is finite, symmetric and of unit
// gain at its band's centre; every B fragment the kernel reads lies inside a plane and every plane position a tap meets inside the
// part that holds samples; the operand, read back through the fragment order and re-summed, is the Toeplitz matrix of the taps
// exactly; nothing read or wrote memory it does not own and no arithmetic overflowed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fir_plan.h"

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
using namespace bn::fir;

static float bf16_value(uint16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main() {
    size_t plans = 0;
    // ---- the tap list: exactly n_taps floats on the heap, so a read past them is caught
    {
        EXPECT(refused(check_taps(nullptr, 3), "null taps"));
        for (size_t n : {(size_t)0, (size_t)2, (size_t)2048, (size_t)2049, (size_t)SIZE_MAX, (size_t)SIZE_MAX - 1}) {
            std::vector<float> one(1, 1.0f);
            EXPECT(refused(check_taps(one.data(), n), "n_taps"));
        }
        for (size_t n : {(size_t)1, (size_t)3, (size_t)2047}) {
            std::vector<float> t(n, 0.5f);
            EXPECT(check_taps(t.data(), n) == BN_OK);
            t[n - 1] = std::nanf("");
            EXPECT(refused(check_taps(t.data(), n), "is not finite"));
            t[n - 1] = -INFINITY;
            EXPECT(refused(check_taps(t.data(), n), "is not finite"));
        }
    }
    // ---- geometry and the operand
    for (uint32_t n : {1u, 3u, 15u, 17u, 19u, 47u, 49u, 51u, 511u, 2045u, 2047u}) {
        const uint32_t K = depth(n), c = halo(n), P = plane_elems(n);
        EXPECT(K % 32 == 0 && K >= n + 15 && K < n + 15 + 32 && steps(n) * 32 == K && 2 * c + 1 == n);
        EXPECT(P % 16 == 0 && lds_bytes(n) == 6 * P && lds_bytes(n) <= 40 * 1024 && live_elems(n) <= P);
        // the last lane of the last tile at the last step reads the plane's last eight elements, no more
        EXPECT((CHUNK - TILE) + 16 * 15 + 8 * 3 + 32 * (steps(n) - 1) + 8 == P);
        // the last output of a chunk reads the sample at plane position CHUNK - 1 + 2 c: the last one that holds a sample
        EXPECT(CHUNK - 1 + 2 * c == live_elems(n) - 1);
        std::vector<float> taps(n);
        for (uint32_t t = 0; t < n; t++) taps[t] = std::ldexp((float)((t * 2654435761u) >> 8) - 8388608.0f, -23 - (int)(t % 40));
        const std::vector<uint16_t> img = pack_taps(taps.data(), n);
        EXPECT(img.size() == image_elems(n) && img.size() * 2 % 16 == 0);
        for (uint32_t j = 0; j < 16; j++)
            for (uint32_t k = 0; k < K; k++) {
                const uint32_t s = k / 32, lane = j + 16 * ((k % 32) / 8), e = k % 8;
                float sum = 0.0f;  // lo + mid + hi is exact in this order
                for (int p = 2; p >= 0; p--) sum += bf16_value(img[(((size_t)s * 3 + p) * 64 + lane) * 8 + e]);
                const int64_t t = (int64_t)j + n - 1 - k;
                EXPECT(sum == (t >= 0 && t < (int64_t)n ? taps[t] : 0.0f));
            }
        plans++;
    }
    // ---- the designer
    {
        std::vector<float> h(3, 7.0f);
        EXPECT(refused(bandpass(48000, 100.0, 1000.0, 3, nullptr), "null"));
        EXPECT(refused(bandpass(48000, 100.0, 1000.0, 0, h.data()), "n_taps") && refused(bandpass(48000, 100.0, 1000.0, 4, h.data()), "n_taps"));
        EXPECT(refused(bandpass(48000, 100.0, 1000.0, SIZE_MAX, h.data()), "n_taps") && refused(bandpass(48000, 100.0, 1000.0, 2049, h.data()), "n_taps"));
        EXPECT(refused(bandpass(0, 100.0, 1000.0, 3, h.data()), "sample_rate"));
        EXPECT(refused(bandpass(48000, 1000.0, 1000.0, 3, h.data()), "lo_hz must be below hi_hz") && refused(bandpass(48000, std::nan(""), 1000.0, 3, h.data()), "lo_hz"));
        EXPECT(refused(bandpass(48000, 100.0, std::nan(""), 3, h.data()), "lo_hz") && refused(bandpass(48000, 24000.0, 1e9, 3, h.data()), "half the sample rate"));
        EXPECT(refused(bandpass(48000, -10.0, 0.0, 3, h.data()), "hi_hz must be positive") && refused(bandpass(48000, -INFINITY, -1.0, 3, h.data()), "hi_hz"));
        EXPECT(h[0] == 7.0f && h[1] == 7.0f && h[2] == 7.0f);  // a refusal writes nothing
    }
    for (uint32_t rate : {1u, 8000u, 48000u, 0xffffffffu})
        for (size_t n : {(size_t)1, (size_t)3, (size_t)63, (size_t)2047})
            for (int kind = 0; kind < 4; kind++) {
                const double nyq = 0.5 * rate;
                const double lo = kind == 0 ? -INFINITY : kind == 3 ? 0.999 * nyq : 0.1 * nyq, hi = kind == 1 ? INFINITY : kind == 3 ? nyq : 0.6 * nyq;
                std::vector<float> h(n);
                EXPECT(bandpass(rate, lo, hi, n, h.data()) == BN_OK);
                double gain = 0.0;
                const double fc = 0.5 * ((lo > 0 ? lo : 0.0) + (hi < nyq ? hi : nyq)) / rate;
                for (size_t t = 0; t < n; t++) {
                    EXPECT(std::isfinite(h[t]) && h[t] == h[n - 1 - t]);
                    gain += (double)h[t] * std::cos(6.283185307179586476925286766559 * fc * ((double)t - 0.5 * (double)(n - 1)));
                }
                EXPECT(std::fabs(gain - 1.0) < 1e-4);
                if (n == 1) EXPECT(h[0] == 1.0f);
                plans++;
            }
    printf("%zu plans, %d failures\n", plans, failures);
    if (failures) return 1;
    printf("asan_fir_plan: ok\n");
    return 0;
}
