// fir_kernel -- the filter of bn_recording_create_filtered (launched by recording.cpp; declaration in fir.h, geometry and the packed
// taps in fir_plan.h, the rule in include/birdnet_hip.h, "FIR filtering").  An FIR over a recording is a banded Toeplitz product;
// here it runs on v_mfma_f32_16x16x32_bf16 with bf16x3.h's f32-complete arithmetic: both operands are exact sums of three bf16
// terms and six of the nine partial products are kept (mm6).
//
//   Y[j][i] = y[t0 + 16 i + j] = sum_k A[j][k] B[k][i],   A[j][k] = taps[j + n_taps - 1 - k] (0 outside),   B[k][i] = x[t0 - c + 16 i + k]
//
// with c = (n_taps - 1) / 2 and K = n_taps + 15 rounded up to 32: one 16 x 16 tile is 256 consecutive outputs.
//
// CHUNK.  A workgroup of four waves owns fir::CHUNK = 4096 consecutive outputs, sixteen tiles, four per wave.
//   * Samples.  The chunk and its halo -- x[c0 - c + p], p < CHUNK - 16 + K -- are read ONCE through the shared sample read
//     (pcm_read.h: every layout, the bits every other consumer sees, 0 outside the recording), split ONCE (split3_pair) and kept as
//     three bf16 planes in LDS: 36 960 bytes at 2047 taps.  Positions at or past CHUNK + n_taps - 1 meet only A's zero padding and
//     are stored as 0, so a non-finite sample cannot reach an output that none of its taps touches.
//   * B fragments are plain LDS reads.  Lane (i = lane & 15, g = lane >> 4) of tile t0 needs at step s the eight consecutive bf16
//     at plane offset t0 + 16 i + 8 g + 32 s: a multiple of 8 elements, so one ds_read_b128 per plane.  The shift by c is folded
//     into where the plane starts, not into the offset, so no padding is needed for alignment.  Banks: the lane's bytes start at
//     32 i + 16 g (+ a wave-uniform multiple of 16).  ds_read_b128 is served in four non-contiguous 16-lane groups (gemm_b3.hip):
//     {0-3, 12-15, 20-27} puts i = 0..3 on bytes 0, 32, 64, 96, i = 12..15 on 128 .. 224 (mod 256) and g = 1, i = 4..11 on the
//     odd 16-byte slots 144 .. 240, 16 .. 112: sixteen distinct slots of the 256-byte bank row.  {4-11, 16-19, 28-31} and the two
//     groups of g = 2, 3 (the same pattern 32 bytes on) likewise, and lanes (i, g + 2), (i + 1, g) read the SAME address.  The
//     natural layout is conflict-free; no swizzle.
//   * A fragments depend on the taps alone and are the same for every tile of every workgroup: K / 32 steps x 3 planes x 4 VGPRs
//     (780 at 2047 taps) do not fit registers, and 3 KiB per step do not fit LDS beside the planes at every tap count.  The host
//     packs them in fragment order (fir::pack_taps) and a wave loads step s + 1 -- three coalesced 1-KiB loads that every wave of
//     the grid shares in L2 -- while it multiplies step s.  One A fragment feeds the wave's four tiles: per step 3 global loads,
//     12 LDS reads and 24 matrix instructions.  No split instruction is issued for the taps on the device.
//   * Arithmetic.  An output is one chain: k ascending over the whole padded K, inside a step mm6's fixed order.  Its bits depend
//     on (taps, n mod 16, the samples), not on the chunk, the recording's length or the grid.
//   * Store.  Lane (i, g) holds y[t0 + 16 i + 4 g .. + 3]: one 16-byte store, a wave's stores cover 1 KiB; the tail is masked to n.
// No atomics, no inline assembly, vector stores only.
#include "fir.h"

#include "bf16x3.h"
#include "device_common.h"
#include "kernels.h"
#include "pcm_read.h"
#include "plan_rules.h"

namespace bn {
namespace {

template <class R>
__global__ __launch_bounds__(fir::LANES) void fir_kernel(float *__restrict__ out, R rd, uint64_t n, const u32x4 *__restrict__ image, uint32_t n_taps) {
    extern __shared__ __align__(16) uint32_t fir_lds[];
    const uint32_t P = fir::plane_elems(n_taps), live = fir::live_elems(n_taps), c = fir::halo(n_taps), S = fir::steps(n_taps);
    const uint64_t c0 = (uint64_t)blockIdx.x * fir::CHUNK;
    uint32_t *hi = fir_lds, *mid = hi + P / 2, *lo = mid + P / 2;

    // the chunk and its halo, two samples per lane and pass: plane position p holds x[c0 + p - c]
    for (uint32_t w = threadIdx.x; w < P / 2; w += fir::LANES) {
        const uint32_t p = 2 * w;
        const uint64_t at = c0 + p;  // the sample's index + c
        float x0 = 0.0f, x1 = 0.0f;
        if (p < live && at >= c && at - c < n) x0 = rd(at - c);
        if (p + 1 < live && at + 1 >= c && at + 1 - c < n) x1 = rd(at + 1 - c);
        uint32_t h, m, l;
        split3_pair(x0, x1, h, m, l);
        hi[w] = h, mid[w] = m, lo[w] = l;
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t t0 = wave * fir::TILES_PER_WAVE * fir::TILE;
    if (c0 + t0 >= n) return;  // (after the only barrier) none of this wave's outputs exists
    const uint32_t li = lane & 15, lg = lane >> 4;
    // 16-byte units: a plane is P / 8 of them; the lane's window of tile u at step s starts at frag + 32 u + 4 s
    const u32x4 *bh = reinterpret_cast<const u32x4 *>(hi) + t0 / 8 + 2 * li + lg, *bm = bh + P / 8, *bl = bm + P / 8;
    const u32x4 *img = image + lane;

    floatx4 acc[fir::TILES_PER_WAVE];
#pragma unroll
    for (uint32_t u = 0; u < fir::TILES_PER_WAVE; u++) acc[u] = floatx4{0.0f, 0.0f, 0.0f, 0.0f};
    u32x4 ah = img[0], am = img[64], al = img[128];
    for (uint32_t s = 0; s < S; s++) {
        const uint32_t sn = s + 1 < S ? s + 1 : s;  // the last step loads itself again: no read past the image
        const u32x4 nh = img[sn * 192], nm = img[sn * 192 + 64], nl = img[sn * 192 + 128];
#pragma unroll
        for (uint32_t u = 0; u < fir::TILES_PER_WAVE; u++) acc[u] = mm6(ah, am, al, bh[32 * u + 4 * s], bm[32 * u + 4 * s], bl[32 * u + 4 * s], acc[u]);
        ah = nh, am = nm, al = nl;
    }

#pragma unroll
    for (uint32_t u = 0; u < fir::TILES_PER_WAVE; u++) {
        const uint64_t at = c0 + t0 + fir::TILE * u + 16 * li + 4 * lg;
        if (at + 3 < n) {
            *reinterpret_cast<floatx4 *>(out + at) = acc[u];
        } else {
#pragma unroll
            for (uint32_t r = 0; r < 4; r++)
                if (at + r < n) out[at + r] = acc[u][r];
        }
    }
}

}  // namespace

void launch_fir(hipStream_t s, float *dst, const PcmSrc &src, uint64_t n, const void *image, uint32_t n_taps) {
    if (n == 0) return;
    const uint64_t blocks = (n - 1) / fir::CHUNK + 1;
    if (!fir::count_ok(n_taps) || !dst || !image || !ptr_aligned16(dst) || !ptr_aligned16(image) || blocks > 0x7fffffffull) {
        launch_error("fir: a plan the kernel cannot take");
        return;
    }
    const bool known = pcm_visit(src, [&](auto rd) {
        using R = decltype(rd);
        hipLaunchKernelGGL((fir_kernel<R>), dim3((uint32_t)blocks), dim3(fir::LANES), fir::lds_bytes(n_taps), s, dst, rd, n,
                           static_cast<const u32x4 *>(image), n_taps);
    });
    if (!known) launch_error("fir: a layout no reader knows");
}

}  // namespace bn
