// denoise_kernel -- the spectral gate of bn_recording_create_denoised (launched by recording.cpp; declarations in denoise.h, the rule in
// include/birdnet_hip.h, "Noise reduction", the geometry in denoise_plan.h).  Templated on the frame length N and on the reader
// (pcm_read.h) like the band kernels, around a transform that goes there and back in one wave's registers (denoise_fft.h).  The data
// flow is the point: a sample is read once, transformed twice and stored once, and the overlap never leaves a lane's registers.
//
// WAVE OWNERSHIP.  H = N/2; frame t covers source positions [(t - 1) H, (t + 1) H); output block b, samples [b H, (b + 1) H), is
// the second half of frame b plus the first half of frame b + 1.  A wave owns denoise::RUN consecutive blocks [b0, b1) and transforms
// frames b0 .. b1, one more frame than blocks (the first frame's head belongs to the wave before, which transforms that frame too:
// the redundancy 1 / RUN).  A workgroup is four such waves that share nothing: no LDS, no barrier, no atomics.
//
// THE REGISTER SHIFT.  Register r of lane l holds frame positions p = 2 (64 r + l) and p + 1.  H = 64 * (RR/2) * 2, so position p >= H
// of frame t is position p - H of frame t + 1 in the SAME lane, RR/2 registers lower (denoise::shift_holds).  Hence:
//   * input is read once: per frame only the new half, H samples in registers RR/2 .. RR-1 (a lane's two samples are neighbours, a
//     wave's loads of one register one contiguous span); the other half is the previous frame's raw upper registers moved down, and
//     windowed afresh.  Only the wave's first frame reads both halves.
//   * the overlap-add is a register add: the tail of y_t waits in RR/2 float2 registers and is added to the head of y_{t+1} in the
//     same lane; the block leaves as 8-byte stores contiguous over the lanes, 512 bytes per wave and register, masked to n.
// The bits of y_t depend on frame t's samples alone, and tail + head is one commutative addition, so an output does not know which
// wave made it or how long the recording is.
//
// Loaded once per wave and kept: the window values of its positions, the twiddles, the thresholds a_k of the lane's bins and of their
// partners, floor_gain and the scales.  Plain f32; no fused multiply-add and no packed f32 (see the Makefile); the one division is the
// gain's.
#include "denoise.h"

#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "denoise_fft.h"
#include "device_mem.h"
#include "kernels.h"
#include "pcm_read.h"

namespace bn {
namespace {

// K of the header's bound, in units of eps = BN_BAND_EPS_ULPS u: the forward error reaches the output once directly and at most twice
// more through the gain (|dg| |X| <= 2 (1 - floor_gain) |dX|), and the inverse direction adds its own eps
static_assert(1 + 2 + 1 == BN_DENOISE_K, "BN_DENOISE_K: forward, forward through the gain (2), inverse");
// the inverse direction is the forward's mirror image: as many stages, the repack for the unpack, the synthesis window for the analysis
// window -- so band levels' eps holds for it
static_assert(7 * band::ilog2(band::FRAME_MAX / 2) + 2 + 7 + 1 == BN_BAND_EPS_ULPS, "one eps per transform direction");
// the term in u: a_k rounded (1), the division (1), the subtraction (1), P's squares, sum and scale (4, through a / P <= 1), the
// product with the gain (1), the overlap-add (1), 3 spare
static_assert(1 + 1 + 1 + 4 + 1 + 1 + 3 == BN_DENOISE_GAIN_ULPS, "BN_DENOISE_GAIN_ULPS is the gain's and the add's share");
static_assert(denoise::WAVES * 64 == denoise::LANES, "four waves");

template <uint32_t N, class R>
__global__ __launch_bounds__(256) void denoise_kernel(float *__restrict__ dst, const R src, uint64_t n, uint64_t B, const float *__restrict__ band_tab,
                                                     const float *__restrict__ win_tab, const float *__restrict__ a, float floor_gain, float scale) {
    constexpr uint32_t H = N / 2, RR = N / 128, HR = RR / 2;
    static_assert(denoise::shift_holds(N, HR, 0) && denoise::shift_holds(N, RR - 1, 63), "the second half of a frame is the first of the next, RR/2 registers lower");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t b0, b1;
    denoise::wave_blocks(B, blockIdx.x, wave, &b0, &b1);
    if (b0 >= b1) return;  // wave-uniform, and the kernel has no barrier
    denoise::DenoiseFft<N> fx;
    fx.load(band_tab, a, lane, floor_gain, scale);
    float2 hw[RR];  // w at the two positions of register r
#pragma unroll
    for (uint32_t r = 0; r < RR; r++) hw[r] = *reinterpret_cast<const float2 *>(win_tab + denoise::frame_pos(r, lane));

    // raw samples of the frame in hand; the first half of frame b0 is [(b0 - 1) H, b0 H), zeros for b0 == 0
    float2 xs[RR], tail[HR];
#pragma unroll
    for (uint32_t r = 0; r < HR; r++) {
        xs[r] = make_float2(0.0f, 0.0f);
        if (b0 > 0) {
            const uint64_t at = (b0 - 1) * H + denoise::frame_pos(r, lane);  // at + 1 < b0 H <= n - 1
            if (at < n) xs[r].x = src(at);
            if (at + 1 < n) xs[r].y = src(at + 1);
        }
        tail[r] = make_float2(0.0f, 0.0f);
    }
    for (uint64_t f = b0; f <= b1; f++) {
        // ---- the new half: frame positions H + p are source samples f H + p (f <= B: f H < n + H)
#pragma unroll
        for (uint32_t r = 0; r < HR; r++) {
            const uint64_t at = f * H + denoise::frame_pos(r, lane);
            float x0 = 0.0f, x1 = 0.0f;
            if (at < n) x0 = src(at);
            if (at + 1 < n) x1 = src(at + 1);
            xs[HR + r] = make_float2(x0, x1);
        }
        float zr[RR], zi[RR];
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) zr[r] = xs[r].x * hw[r].x, zi[r] = xs[r].y * hw[r].y;
        fx.gate(zr, zi, lane);
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) zr[r] = zr[r] * hw[r].x, zi[r] = zi[r] * hw[r].y;
        // ---- block f - 1 = the tail in hand + this frame's head
        if (f > b0) {
#pragma unroll
            for (uint32_t r = 0; r < HR; r++) {
                uint64_t at;
                const uint32_t inside = denoise::store_count(n, f - 1, H, r, lane, &at);  // of the two samples, those below n
                const float2 y = make_float2(tail[r].x + zr[r], tail[r].y + zi[r]);
                if (inside == 2) *reinterpret_cast<float2 *>(dst + at) = y;
                else if (inside == 1) dst[at] = y.x;
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < HR; r++) {
            tail[r] = make_float2(zr[HR + r], zi[HR + r]);
            xs[r] = xs[HR + r];
        }
    }
}

struct Tables {
    DeviceBuf<float> d;
    float scale = 0.0f;
};

}  // namespace

hipError_t denoise_tables(int device, uint32_t N, const float **tab, float *scale) {
    // never destroyed: the tables live as long as the process, and at exit the runtime may be gone before static destructors run
    static std::mutex mu;
    static auto *cache = new std::map<std::pair<int, uint32_t>, Tables>();
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache->find({device, N});
    if (it == cache->end()) {
        std::vector<float> host(denoise::table_floats(N));
        Tables tb;
        tb.scale = denoise::fill_tables(N, host.data());
        hipError_t e = tb.d.alloc(host.size() * sizeof(float));
        if (e == hipSuccess) e = gated::Memcpy(tb.d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
        it = cache->emplace(std::make_pair(device, N), std::move(tb)).first;
    }
    *tab = it->second.d.get();
    *scale = it->second.scale;
    return hipSuccess;
}

void launch_denoise(hipStream_t s, float *dst, const PcmSrc &src, uint64_t n, const denoise::Plan &plan, const float *band_tab, const float *win_tab,
                    const float *a, float scale) {
    if (n == 0) return;
    const uint64_t groups = band::frame_ok(plan.N) && n <= denoise::N_MAX ? denoise::n_groups(n, plan.N) : 0;
    if (groups == 0 || groups > denoise::GRID_MAX || plan.H != plan.N / 2 || !dst || (reinterpret_cast<uintptr_t>(dst) & 7u) || !band_tab || !win_tab || !a) {
        launch_error("denoise: a plan the kernel cannot take");
        return;
    }
    const uint64_t B = denoise::n_blocks(n, plan.N);
    const float floor_gain = plan.floor_gain;
    const bool known = pcm_visit(src, [&](auto rd) {
        using R = decltype(rd);
        const dim3 grid((uint32_t)groups), block(denoise::LANES);
        switch (plan.N) {
            case 256: hipLaunchKernelGGL((denoise_kernel<256, R>), grid, block, 0, s, dst, rd, n, B, band_tab, win_tab, a, floor_gain, scale); break;
            case 512: hipLaunchKernelGGL((denoise_kernel<512, R>), grid, block, 0, s, dst, rd, n, B, band_tab, win_tab, a, floor_gain, scale); break;
            case 1024: hipLaunchKernelGGL((denoise_kernel<1024, R>), grid, block, 0, s, dst, rd, n, B, band_tab, win_tab, a, floor_gain, scale); break;
            default: hipLaunchKernelGGL((denoise_kernel<2048, R>), grid, block, 0, s, dst, rd, n, B, band_tab, win_tab, a, floor_gain, scale); break;
        }
    });
    if (!known) launch_error("denoise: a layout no reader knows");
}

}  // namespace bn
