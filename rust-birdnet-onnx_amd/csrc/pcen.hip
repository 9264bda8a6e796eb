// bn_recording_pcen, stage 2 (include/birdnet_hip.h, "PCEN"): per-channel energy normalisation of the f32 spectrogram image that
// stage 1 (launch_spectrogram) left on the device.  Per row j, with x = gain * E, a = 1 - s:
//   M[t] = a M[t-1] + s x[t] where x[t] is finite, M[t-1] otherwise;   V[t] = (x[t] / (eps + M[t])^alpha + delta)^r - delta^r,
// +Inf (code 255) where x[t] is not finite.  The recurrence along time is the one data flow of the recording layer that ties
// frames together.  It is linear, so a chunk of pcen::CHUNK frames acts on M as M_end = a^n M_start + S, with S the recurrence run
// from 0 over the chunk and n its finite frames.  Three launches, none waiting on another workgroup:
//   pcen_chunk_kernel   a wave owns one chunk and 64 consecutive rows, a lane a row.  It walks the chunk from S = 0 with
//                       S = fma(a, S, s * x) over finite elements and counts them; lane l of frame t reads float t * R + row0 + l, so
//                       a wave's load is one 256-byte run, and the loads of AHEAD = 8 frames are issued before the eight dependent
//                       fmas.  It writes S[chunk][row] and n[chunk][row].
//   pcen_carry_kernel   a lane owns a row and walks the chunks in order: it stores the carry M into chunk c, then
//                       M = fma(apow[n], M, S).  apow[n] = a^n comes from the host, double rounded once (pcen::apow), so a carry is two
//                       roundings per chunk however long the chunk.  The loads of eight chunks are issued ahead of the chain.  M
//                       starts from the device state or from the first frame's rule and ends in the device state.
//   pcen_apply_kernel   the chunk kernel's split.  A lane starts from its chunk's carry, reruns the recurrence and forms V per
//                       element; powers are x^p = exp2(p * log2 x) on the hardware's exp2 / log2 (with the compiler's scaling of
//                       denormals), one rule for every alpha and r, delta^r included: where x is 0 the two powers are the same bits
//                       and V is exactly 0.  A frame leaves as 64 consecutive floats or 64 consecutive codes per wave; the 255
//                       thresholds sit in LDS and a code is the spectrogram's eight-read branch-free search (restated here:
//                       spectrogram.hip keeps it in an unnamed namespace).
// Rows that do not fill a wave idle the spare lanes.  No atomics, no private segment, no inline assembly, vector stores only; the
// only LDS is the table (1 024 bytes, apply kernel).  Registers: chunk 16 VGPRs, carry 70, apply 54 ("PCEN").
#include "pcen.h"

#include "kernels.h"

namespace bn {
namespace {

// M's relative depth per frame: the product gain * E and the product s * x on the new term, the rounding of a on the old one (2 at
// most on their sum), the fma (1); per chunk the rounding of apow[n] and the carry's fma (2), charged to every frame; 1 spare for
// the second-order terms
static_assert(2 + 1 + 2 + 1 == BN_PCEN_SMOOTH_DEPTH, "BN_PCEN_SMOOTH_DEPTH is the smoother's fixed depth");
// measured, not derived: four times 22.4, the worst ratio of the GPU suite's cases on an MI355X, rounded up ("PCEN")
static_assert(BN_PCEN_VALUE_DEPTH == 90, "BN_PCEN_VALUE_DEPTH is four times the measured worst ratio");

using pcen::AHEAD;
using pcen::CHUNK;

// what the kernels need of a plan, as kernel arguments (scalar registers)
struct PcenArgs {
    uint32_t n_rows, n_frames, n_chunks, row_blocks, u8;
    float a, s, gain, alpha, delta, r, eps;
};

__device__ __forceinline__ bool finite(float x) { return __builtin_fabsf(x) < __builtin_inff(); }  // false for a NaN
__device__ __forceinline__ float power(float x, float p) { return __builtin_exp2f(p * __builtin_log2f(x)); }

// the number of thresholds thr[0 .. 254] (non-decreasing) that are not above v; a NaN is above all of them
__device__ __forceinline__ uint32_t code_of(const float *thr, float v) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t step = 128; step > 0; step >>= 1) {
        const uint32_t to = c + step;  // thr[to - 1] is the to-th threshold
        if (to <= pcen::N_THR && !(v < thr[to - 1])) c = to;
    }
    return c;
}

// The wave's chunk and rows.  false: a wave past the launch's last unit (wave-uniform)
struct Unit {
    uint32_t chunk, row, len;
    bool live;  // the lane's row exists
    size_t first;  // the element of the chunk's first frame in the lane's row (row 0 for an idle lane)
};
__device__ __forceinline__ bool unit_of(const PcenArgs &a, Unit *u) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t unit = blockIdx.x * pcen::WAVES + wave;
    u->chunk = unit / a.row_blocks;
    if (u->chunk >= a.n_chunks) return false;
    u->row = (unit - u->chunk * a.row_blocks) * pcen::WAVE_ROWS + lane;
    u->live = u->row < a.n_rows;
    const uint32_t t0 = u->chunk * CHUNK;
    u->len = a.n_frames - t0 < CHUNK ? a.n_frames - t0 : CHUNK;
    u->first = (size_t)t0 * a.n_rows + (u->live ? u->row : 0u);
    return true;
}

// frames k0 .. k0 + AHEAD - 1 of the unit's chunk, +Inf (a skipped element) past the chunk's end and in an idle lane
__device__ __forceinline__ void load_ahead(float (&v)[AHEAD], const float *__restrict__ image, const PcenArgs &a, const Unit &u, uint32_t k0) {
#pragma unroll
    for (uint32_t i = 0; i < AHEAD; i++) v[i] = u.live && k0 + i < u.len ? image[u.first + (size_t)(k0 + i) * a.n_rows] : __builtin_inff();
}

__global__ __launch_bounds__(256) void pcen_chunk_kernel(float *__restrict__ sums, uint32_t *__restrict__ counts, const float *__restrict__ image, const PcenArgs a) {
    Unit u;
    if (!unit_of(a, &u)) return;
    float S = 0.0f;
    uint32_t n = 0;
    for (uint32_t k0 = 0; k0 < u.len; k0 += AHEAD) {
        float v[AHEAD];
        load_ahead(v, image, a, u, k0);
#pragma unroll
        for (uint32_t i = 0; i < AHEAD; i++) {
            const float x = a.gain * v[i];
            const bool fin = finite(x);
            const float next = __builtin_fmaf(a.a, S, a.s * x);
            S = fin ? next : S, n += fin ? 1u : 0u;
        }
    }
    if (u.live) sums[(size_t)u.chunk * a.n_rows + u.row] = S, counts[(size_t)u.chunk * a.n_rows + u.row] = n;
}

__global__ __launch_bounds__(64) void pcen_carry_kernel(float *__restrict__ carry, float *__restrict__ state, const float *__restrict__ sums,
                                                       const uint32_t *__restrict__ counts, const float *__restrict__ apow, const float *__restrict__ image,
                                                       const PcenArgs a, uint32_t first_rule) {
    const uint32_t row = blockIdx.x * 64u + threadIdx.x;
    if (row >= a.n_rows) return;
    float M;
    if (first_rule) {  // M[-1] = x[0] if finite, else 0
        const float x0 = a.gain * image[row];
        M = finite(x0) ? x0 : 0.0f;
    } else {
        M = state[row];
    }
    for (uint32_t c0 = 0; c0 < a.n_chunks; c0 += AHEAD) {
        float S[AHEAD], p[AHEAD];
#pragma unroll
        for (uint32_t i = 0; i < AHEAD; i++) {
            const bool here = c0 + i < a.n_chunks;
            const size_t at = (size_t)(c0 + i) * a.n_rows + row;
            const uint32_t n = here ? counts[at] : 0u;
            S[i] = here ? sums[at] : 0.0f, p[i] = apow[n < CHUNK ? n : CHUNK];
        }
#pragma unroll
        for (uint32_t i = 0; i < AHEAD; i++)
            if (c0 + i < a.n_chunks) {
                carry[(size_t)(c0 + i) * a.n_rows + row] = M;
                M = __builtin_fmaf(p[i], M, S[i]);
            }
    }
    state[row] = M;
}

__global__ __launch_bounds__(256) void pcen_apply_kernel(void *__restrict__ out, const float *__restrict__ image, const float *__restrict__ carry,
                                                        const float *__restrict__ thr, const PcenArgs a) {
    __shared__ float thr_l[pcen::N_THR + 1];
    if (a.u8 && threadIdx.x < pcen::N_THR) thr_l[threadIdx.x] = thr[threadIdx.x];
    __syncthreads();
    Unit u;
    if (!unit_of(a, &u)) return;
    float M = u.live ? carry[(size_t)u.chunk * a.n_rows + u.row] : 0.0f;
    const float dr = power(a.delta, a.r);
    for (uint32_t k0 = 0; k0 < u.len; k0 += AHEAD) {
        float v[AHEAD];
        load_ahead(v, image, a, u, k0);
#pragma unroll
        for (uint32_t i = 0; i < AHEAD; i++) {
            if (k0 + i >= u.len) break;  // wave-uniform
            const float x = a.gain * v[i];
            const bool fin = finite(x);
            const float next = __builtin_fmaf(a.a, M, a.s * x);
            M = fin ? next : M;
            const float y = x / power(a.eps + M, a.alpha) + a.delta;
            const float V = fin ? power(y, a.r) - dr : __builtin_inff();
            if (u.live) {
                const size_t at = u.first + (size_t)(k0 + i) * a.n_rows;
                if (a.u8)
                    static_cast<uint8_t *>(out)[at] = (uint8_t)code_of(thr_l, V);
                else
                    static_cast<float *>(out)[at] = V;
            }
        }
    }
}

}  // namespace

void launch_pcen(hipStream_t s, void *out, const float *image, size_t n_frames, uint32_t n_rows, const pcen::Plan &plan, const PcenScratch &sc, bool first_rule) {
    if (n_frames == 0) return;
    const bool u8 = plan.format == BN_PCEN_U8;
    if (!out || !image || !sc.sums || !sc.counts || !sc.carry || !sc.state || !sc.apow || (u8 && !sc.thr) || n_rows == 0 ||
        n_frames > (((size_t)1 << 26) / n_rows) || (!u8 && plan.format != BN_PCEN_F32)) {
        launch_error("pcen: a plan the kernels cannot take");
        return;
    }
    const uint32_t n_chunks = (uint32_t)pcen::chunks(n_frames), rb = pcen::row_blocks(n_rows);
    const PcenArgs a{n_rows, (uint32_t)n_frames, n_chunks, rb, u8 ? 1u : 0u, plan.a, plan.s, plan.gain, plan.alpha, plan.delta, plan.r, plan.eps};
    const uint32_t blocks = (uint32_t)(((size_t)n_chunks * rb + pcen::WAVES - 1) / pcen::WAVES);
    hipLaunchKernelGGL(pcen_chunk_kernel, dim3(blocks), dim3(pcen::LANES), 0, s, sc.sums, sc.counts, image, a);
    hipLaunchKernelGGL(pcen_carry_kernel, dim3(rb), dim3(64), 0, s, sc.carry, sc.state, sc.sums, sc.counts, sc.apow, image, a, first_rule ? 1u : 0u);
    hipLaunchKernelGGL(pcen_apply_kernel, dim3(blocks), dim3(pcen::LANES), 0, s, out, image, sc.carry, sc.thr, a);
}

}  // namespace bn
