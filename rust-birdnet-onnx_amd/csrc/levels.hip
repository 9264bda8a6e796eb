// Kernels that read chosen windows of recordings, in front of an unchanged plan (launched by recording.cpp; declarations in levels.h).
//
//   * levels_kernel -- the level meter of bn_recording_levels: one workgroup of 256 lanes per window, templated on the reader
//     (pcm_read.h) like kernels.hip's windows_kernel, so a sample is exactly the f32 value bn_recording_windows returns, 0 past
//     the end.  Lane t of the workgroup reads frames t + 256 j of the window, j = 0, 1, ...: the 64 lanes of a wave read 64
//     neighbouring frames.  Overlapping windows are read again; nothing is shared between windows, so a window's bits cannot
//     depend on the step.
//
//     THE TREE (include/birdnet_hip.h, BN_LEVEL_SUM_DEPTH; every addition is a plain f32 addition, the library is built with
//     -ffp-contract=off, x * x is rounded before it is added).  Position i of the window, 0 <= i < S rounded up to 1024, goes
//     to lane t = i % 256 and that lane's accumulator u = (i / 256) % 4; positions at or past S, like frames past the end of
//     the recording, contribute 0.  Per accumulator the terms are added in ascending i, starting from 0.0f:
//         chain      acc[u] = acc[u] + term                      ceil(S / 1024) additions
//         lane       (acc[0] + acc[1]) + (acc[2] + acc[3])       2
//         wave       v = v + v(lane ^ m), m = 32, 16, ..., 1      6  (a + b == b + a bit for bit: every lane holds the same value)
//         workgroup  (w[0] + w[1]) + (w[2] + w[3]) through LDS   2
//     and the sum is divided by (float)S once.  The peak is a maximum over the same tree (exact whatever the order); the
//     non-finite flag an OR.  The tree is a function of S alone: not of the window's number, the launch's first window or
//     count, the step, the recording's length or its layout.
//     No atomics, no scratch; the result of a window is one 16-byte vector store by lane 0.
//
//   * window_list_kernel -- the gather of bn_step_window_list / bn_recording_window_list: row b of the launch is S frames of SOME
//     recording from an arbitrary start, its descriptor (the reader's fields at that start, the frames that exist, the
//     destination row) a kernel argument as live.hip's LiveRow is.  The reader and its fields are the ones pcm_visit makes for the
//     row's layout at that start (launch_window_list), so there is one reader choice and one `inv` in the library.  One lane =
//     4 consecutive frames (one float4 store; S % 4 == 0), frames at or past `valid` are 0: windows_kernel's loads, conversions
//     and store for the same samples, so the rows carry the same bits.  One instantiation per reader; the host groups a list's rows by reader and launches once per
//     group (window_list_plan.h).  grid (ceil(S/1024), rows)
#include "levels.h"

#include <type_traits>

#include "kernels.h"
#include "pcm_read.h"

namespace bn {
namespace {

constexpr uint32_t LEVEL_LANES = 256, LEVEL_ACC = 4, LEVEL_WAVES = LEVEL_LANES / 64;
// the chain for S <= 2^20 plus the three fixed stages: what the header declares
static_assert(((1u << 20) / (LEVEL_LANES * LEVEL_ACC)) + 2 + 6 + 2 == BN_LEVEL_SUM_DEPTH, "BN_LEVEL_SUM_DEPTH is this tree's depth");
static_assert(BN_LEVEL_NONFINITE == 1u && BN_LEVEL_PADDED == 2u, "the flag bits of the header");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

template <class R>
__global__ __launch_bounds__(256) void levels_kernel(WindowLevel *__restrict__ out, const R src, uint64_t n_samples, uint64_t first_start,
                                                    uint64_t step, uint32_t S) {
    __shared__ float w_sum[LEVEL_WAVES], w_sq[LEVEL_WAVES], w_peak[LEVEL_WAVES];
    __shared__ uint32_t w_bad[LEVEL_WAVES];
    const uint32_t t = threadIdx.x;
    const uint64_t start = first_start + (uint64_t)blockIdx.x * step;
    // frames of the window that the recording holds
    const uint64_t valid = start < n_samples ? (n_samples - start < S ? n_samples - start : (uint64_t)S) : 0;
    float sum[LEVEL_ACC], sq[LEVEL_ACC];
#pragma unroll
    for (uint32_t u = 0; u < LEVEL_ACC; u++) sum[u] = 0.0f, sq[u] = 0.0f;
    float peak = 0.0f;
    uint32_t bad = 0;
    for (uint64_t base = 0; base < S; base += LEVEL_LANES * LEVEL_ACC) {
#pragma unroll
        for (uint32_t u = 0; u < LEVEL_ACC; u++) {
            const uint64_t i = base + u * LEVEL_LANES + t;
            float x = 0.0f;
            if (i < valid) x = src(start + i);
            const float a = fabsf(x);
            bad |= !(a < __builtin_inff());  // NaN or +-Inf
            peak = fmaxf(peak, a);
            sum[u] = sum[u] + x;
            sq[u] = sq[u] + x * x;
        }
    }
    float s = (sum[0] + sum[1]) + (sum[2] + sum[3]);
    float q = (sq[0] + sq[1]) + (sq[2] + sq[3]);
    s = wave_sum(s);
    q = wave_sum(q);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        peak = fmaxf(peak, __shfl_xor(peak, m));
        bad |= __shfl_xor(bad, m);
    }
    if ((t & 63u) == 0) {
        w_sum[t >> 6] = s;
        w_sq[t >> 6] = q;
        w_peak[t >> 6] = peak;
        w_bad[t >> 6] = bad;
    }
    __syncthreads();
    if (t != 0) return;
    s = (w_sum[0] + w_sum[1]) + (w_sum[2] + w_sum[3]);
    q = (w_sq[0] + w_sq[1]) + (w_sq[2] + w_sq[3]);
    peak = fmaxf(fmaxf(w_peak[0], w_peak[1]), fmaxf(w_peak[2], w_peak[3]));
    bad = w_bad[0] | w_bad[1] | w_bad[2] | w_bad[3];
    const float fS = (float)S;
    float mean = s / fS, mean_square = q / fS;
    uint32_t flags = valid < S ? BN_LEVEL_PADDED : 0u;
    if (bad) {  // never "quiet": the sums of such a window mean nothing
        flags |= BN_LEVEL_NONFINITE;
        peak = __builtin_inff();
        mean_square = __builtin_inff();
        mean = 0.0f;
    }
    *reinterpret_cast<float4 *>(out + blockIdx.x) = make_float4(peak, mean, mean_square, __uint_as_float(flags));
}

// the reader of a row: the launch's kind with the row's fields
template <class R>
struct RowReader;
template <class T>
struct RowReader<PcmMono<T>> {
    static __device__ __forceinline__ PcmMono<T> at(const WindowListRow &d) { return PcmMono<T>{static_cast<const T *>(d.base)}; }
};
template <int FORMAT>
struct RowReader<PcmFrames<FORMAT>> {
    static __device__ __forceinline__ PcmFrames<FORMAT> at(const WindowListRow &d) {
        return PcmFrames<FORMAT>{static_cast<const uint8_t *>(d.base), (uint32_t)d.channels, (int32_t)d.channel, d.inv};
    }
};

template <class R>
__global__ __launch_bounds__(256) void window_list_kernel(float *__restrict__ dst, uint32_t S, WindowListRows rows) {
    const uint32_t i = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i >= S) return;
    const WindowListRow d = rows.r[blockIdx.y];
    const R src = RowReader<R>::at(d);
    float v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++) {
        if (i + u < d.valid) v[u] = src((uint64_t)(i + u));
        else v[u] = 0.0f;
    }
    *reinterpret_cast<float4 *>(dst + (uint64_t)d.dst * S + i) = make_float4(v[0], v[1], v[2], v[3]);
}

// a row's descriptor from the reader pcm_visit made for it: the kernel rebuilds exactly that reader (RowReader)
template <class T>
void describe(WindowListRow &d, const PcmMono<T> &rd) {
    d.base = rd.p;
    d.channels = 1, d.channel = 0, d.inv = 1.0f;
}
template <int FORMAT>
void describe(WindowListRow &d, const PcmFrames<FORMAT> &rd) {
    d.base = rd.p;
    d.channels = (uint16_t)rd.channels, d.channel = (int16_t)rd.channel, d.inv = rd.inv;
}

}  // namespace

void launch_levels(hipStream_t s, WindowLevel *out, const PcmSrc &src, uint64_t n_samples, uint64_t first_start, uint64_t step, uint32_t S, uint32_t count) {
    if (count == 0 || S == 0) return;
    pcm_visit(src, [&](auto rd) {
        hipLaunchKernelGGL(levels_kernel<decltype(rd)>, dim3(count), dim3(LEVEL_LANES), 0, s, out, rd, n_samples, first_start, step, S);
    });
}

void launch_window_list(hipStream_t s, float *dst, uint32_t S, const WindowListSrc *rows, uint32_t n) {
    if (n == 0 || S == 0) return;
    if (n > (uint32_t)WINDOW_LIST_ROWS) {
        launch_error("window list gather: more than 128 rows in one launch");
        return;
    }
    // the launch's reader is the first row's; every row must be given the same one
    const bool known = pcm_visit(rows[0].src, [&](auto first) {
        using R = decltype(first);
        WindowListRows args;
        bool same = true;
        for (uint32_t i = 0; i < n; i++) {
            bool match = false;
            const bool ok = pcm_visit(rows[i].src, [&](auto rd) {
                if constexpr (std::is_same_v<decltype(rd), R>) {
                    describe(args.r[i], rd);
                    match = true;
                }
            });
            same = same && ok && match;
            args.r[i].valid = rows[i].valid;
            args.r[i].dst = rows[i].dst;
        }
        for (uint32_t i = n; i < (uint32_t)WINDOW_LIST_ROWS; i++) args.r[i] = WindowListRow{nullptr, 0, 0, 1, 0, 1.0f};
        if (!same) {
            launch_error("window list gather: rows of different readers in one launch");
            return;
        }
        hipLaunchKernelGGL(window_list_kernel<R>, dim3((S / 4 + 255) / 256, n), dim3(256), 0, s, dst, S, args);
    });
    if (!known) launch_error("window list gather: a layout no reader knows");
}

}  // namespace bn
