// spectrogram_bins_kernel, spectrogram_bank_kernel -- the kernels of bn_recording_spectrogram (launched by recording.cpp;
// declarations in spectrogram.h, geometry and the packed bank in spectrogram_plan.h, the rule in include/birdnet_hip.h,
// "Spectrograms").  Templated on the frame length N and on the reader (pcm_read.h) like band_levels_kernel and
// spectral_profile_kernel, around the same transform (band_fft.h: one frame in one wave's registers), with the third data flow:
// band levels reduces over the bins of a frame, the profile over time, these keep both axes.
//
// TILE.  A workgroup of 256 lanes owns spectro::TILE_FRAMES = 16 consecutive frames, one column block of the matrix instruction.
// Wave w transforms frames w, w + 4, w + 8, w + 12 of the tile with BandFft<N>::frame, each frame as a window of its own (start =
// the frame's first sample, base 0), so a frame's bits depend on its N samples alone; frames at or past n_frames are skipped
// wave-uniformly.  A frame's non-finite flag is or-ed over its wave and kept per frame in LDS: at the store such a frame reads
// +Inf (code 255) in every row.  Both kernels keep the 255 thresholds of the U8 codes in LDS; a code is the number of thresholds
// that are not above the value, found by a branch-free binary search of eight LDS reads -- the table's answer for every input.
//
// BINS.  The power goes to LDS as f32 rows [frame][N/2 + 1], each row swizzled as the profile's rows (spectro::lds_index ==
// profile::lds_index): a wave stores one register of its 64 lanes, RR floats apart, into ONE row at a time, so the profile's
// argument holds as it stands and every ds_write is conflict free.  After one barrier the tile's output, nf * n_rows elements, is
// one contiguous 64-byte-aligned range of `out` (a tile starts at a multiple of 16 frames), and the lanes walk it flat, four
// consecutive elements each: one 16-byte store for F32, four codes in one dword store for U8, contiguous over the lanes.  The
// issue's form writes the head and tail of a ROW apart where n_rows is no multiple of 4; walking the TILE flat needs that for
// the tile's last up to three elements only.  The reads of consecutive bins stay inside aligned blocks of 32, at most 2-way.
//
// BANK.  E[m][t] = sum_k W[m][k] P[t,k] on v_mfma_f32_16x16x32_bf16 with bf16x3.h's f32-complete arithmetic.
//   * Planes.  A lane splits its RR consecutive powers once (split3_pair, in bin order, i.e. registers bitrev(2p), bitrev(2p + 1))
//     and stores RR bf16 per plane with one contiguous store into three planes [frame][stride]; lanes 0 .. 15 of the wave store
//     bin N/2 (lane 0 holds it) and the zeros that pad K = N/2 + 1 to depth = N/2 + 32.
//   * B fragments.  Lane (i = lane & 15, g = lane >> 4) needs at step s the eight bf16 of frame i at bins 32 s + 8 g ..: one
//     ds_read_b128 per plane at byte i * R + 16 g + 64 s, R = 2 * stride.  ds_read_b128 is served in four 16-lane groups
//     (gemm_b3.hip, fir.hip): {0-3, 12-15, 20-27} is g = 0 with i in {0..3, 12..15} and g = 1 with i in {4..11}.  The 16-byte
//     slot of a lane in the 256-byte bank row is (i r + g) mod 16, r = R / 16.  stride = depth + 16 makes R = 32 mod 64, r = 2 q
//     with q odd: i r mod 16 = 2 (q i mod 8), a bijection of i mod 8 onto the even slots.  Both i-sets of a group are complete
//     residue systems mod 8, so g = 0 takes the eight even slots and g = 1 the eight odd ones: sixteen distinct slots, no conflict;
//     {4-11, 16-19, 28-31} and the two groups of g = 2, 3 likewise.  The padding costs 16 of up to 1072 elements per row.
//   * A fragments.  bn_filterbank_create packed W on the host in fragment order (spectro::pack_bank), only the K steps between each
//     row tile's first and last non-zero column, with (first step, count, offset) per tile.  Wave w takes row tiles w, w + 4, ...;
//     per step it loads the next step's three 1-KiB fragments while it multiplies (as fir.hip does) and runs mm6 in its fixed
//     order, k ascending.  A skipped step would add +0.0f to a non-negative sum: skipping changes no bit.
//   * Store.  The accumulator lane (i, g) holds rows 16 j + 4 g .. + 3 of frame i: one 16-byte store for F32, one dword of four
//     codes for U8, where n_rows is a multiple of 4; element by element, masked to n_rows, otherwise.
//
// Dynamic LDS (spectro::bins_lds_bytes, bank_lds_bytes): 66 688 / 104 000 bytes at frame 2048, which need the opt-in beyond
// 64 KiB (spectrogram_prepare).  No atomics, no private segment, no inline assembly, vector stores only.  Registers and LDS per
// instantiation (frames 256 / 512 / 1024 / 2048, over the seven readers): bins 59-66 / 90-106 / 157-189 / 256 + 92 AGPRs and
// 9 344 / 17 536 / 33 920 / 66 688 bytes; bank 63-67 / 91-105 / 153-184 / 256 + 78 AGPRs and 17 984 / 30 272 / 54 848 / 104 000 bytes
// ("Spectrogram").
#include "spectrogram.h"

#include <mutex>

#include "band_fft.h"
#include "bf16x3.h"
#include "capi_internal.h"
#include "device_common.h"
#include "kernels.h"
#include "pcm_read.h"

namespace bn {
namespace {

// b(t,k)'s relative part: x*x, y*y and their sum count as 2; the scale and its f32 constant as 2; 2 spare
static_assert(2 + 2 + 2 == BN_SPECTROGRAM_POW_DEPTH, "BN_SPECTROGRAM_POW_DEPTH is a bin's fixed depth");
// a bank row: six accumulations per step (mm6), every one of them one rounding of the non-negative running sum, over the steps of
// the longest frame; 8 as FIR filtering allows for the instruction's own sum.  The splits of weights and powers are exact
static_assert(6 * spectro::steps(band::FRAME_MAX) + 8 == BN_SPECTROGRAM_BANK_DEPTH, "BN_SPECTROGRAM_BANK_DEPTH is the accumulation chain at frame 2048");
static_assert(spectro::lds_index(2048, 777) == (777u ^ ((777u >> 5) & 31u)), "the profile's swizzle");

constexpr uint32_t HEAD_WORDS = spectro::HEAD_BYTES / 4, THR_WORDS = spectro::N_THR + 1;

// what the kernels need of a plan, as kernel arguments (scalar registers)
struct SpecArgs {
    uint32_t lo, n_rows, hop, n_frames, u8;
    float scale;
};

// the number of thresholds thr[0 .. 254] (non-decreasing) that are not above v; a NaN is above all of them
__device__ __forceinline__ uint32_t code_of(const float *thr, float v) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t step = 128; step > 0; step >>= 1) {
        const uint32_t to = c + step;  // thr[to - 1] is the to-th threshold
        if (to <= spectro::N_THR && !(v < thr[to - 1])) c = to;
    }
    return c;
}

// The frames of tile t0 that wave `wave` owns, transformed and handed to store(f, e, e_top); the frame's flag goes to bad_l[f]
template <uint32_t N, class R, class Store>
__device__ __forceinline__ void transform_tile(const R &src, uint64_t n_samples, uint64_t start, const float *__restrict__ tab, const SpecArgs &a, uint32_t t0,
                                               uint32_t lane, uint32_t wave, uint32_t *bad_l, band::BandFft<N> &fft, Store &&store) {
    constexpr uint32_t RR = N / 128;
    fft.load_tables(tab, lane);
    const float s_in = a.scale * 0.5f, s_edge = a.scale * 0.25f;  // c_k / 4: the unpack leaves 2 X_k
    for (uint32_t f = wave; f < spectro::TILE_FRAMES; f += spectro::WAVES) {
        if (t0 + f >= a.n_frames) break;  // wave-uniform
        const uint64_t at = start + (uint64_t)(t0 + f) * a.hop;
        const uint64_t valid = at < n_samples ? (n_samples - at < N ? n_samples - at : (uint64_t)N) : 0;
        float e[RR], e_top;
        uint32_t bad = 0;
        fft.frame(src, at, 0u, valid, lane, s_in, s_edge, bad, e, e_top);
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) bad |= __shfl_xor(bad, m);
        if (lane == 0) bad_l[f] = bad;
        store(f, e, e_top);
    }
}

template <uint32_t N, class R>
__global__ __launch_bounds__(256) void spectrogram_bins_kernel(void *__restrict__ out, const R src, uint64_t n_samples, uint64_t start,
                                                              const float *__restrict__ tab, const float *__restrict__ thr, const SpecArgs a) {
    constexpr uint32_t M = N / 2, RR = M / 64, ROW = spectro::bins_row(N);
    extern __shared__ __align__(16) uint32_t spec_lds[];
    float *thr_l = reinterpret_cast<float *>(spec_lds);
    uint32_t *bad_l = spec_lds + THR_WORDS;
    float *rows = reinterpret_cast<float *>(spec_lds + HEAD_WORDS);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = __builtin_amdgcn_readfirstlane(t >> 6), t0 = blockIdx.x * spectro::TILE_FRAMES;
    if (a.u8 && t < spectro::N_THR) thr_l[t] = thr[t];
    band::BandFft<N> fft;
    transform_tile<N>(src, n_samples, start, tab, a, t0, lane, wave, bad_l, fft, [&](uint32_t f, const float(&e)[RR], float e_top) {
        float *row = rows + f * ROW;
#pragma unroll
        for (uint32_t r = 0; r < RR; r++) row[spectro::lds_index(N, fft.bin(r))] = e[r];
        if (lane == 0) row[M] = e_top;
    });
    __syncthreads();

    const uint32_t nf = a.n_frames - t0 < spectro::TILE_FRAMES ? a.n_frames - t0 : spectro::TILE_FRAMES;
    const uint32_t total = nf * a.n_rows;  // <= 16 * 1025
    const size_t tile_at = (size_t)t0 * a.n_rows;
    auto value = [&](uint32_t i) {
        const uint32_t f = i / a.n_rows, j = i - f * a.n_rows;
        const float v = rows[f * ROW + spectro::lds_index(N, a.lo + j)];
        return bad_l[f] ? __builtin_inff() : v;
    };
    if (!a.u8) {
        float *o = static_cast<float *>(out) + tile_at;
        for (uint32_t i = 4 * t; i < total; i += 4 * spectro::LANES) {
            if (i + 3 < total) {
                *reinterpret_cast<floatx4 *>(o + i) = floatx4{value(i), value(i + 1), value(i + 2), value(i + 3)};
            } else {
                for (uint32_t r = 0; i + r < total; r++) o[i + r] = value(i + r);
            }
        }
    } else {
        uint8_t *o = static_cast<uint8_t *>(out) + tile_at;
        for (uint32_t i = 4 * t; i < total; i += 4 * spectro::LANES) {
            if (i + 3 < total) {
                const uint32_t c0 = code_of(thr_l, value(i)), c1 = code_of(thr_l, value(i + 1)), c2 = code_of(thr_l, value(i + 2)), c3 = code_of(thr_l, value(i + 3));
                *reinterpret_cast<uint32_t *>(o + i) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            } else {
                for (uint32_t r = 0; i + r < total; r++) o[i + r] = (uint8_t)code_of(thr_l, value(i + r));
            }
        }
    }
}

template <uint32_t N, class R>
__global__ __launch_bounds__(256) void spectrogram_bank_kernel(void *__restrict__ out, const R src, uint64_t n_samples, uint64_t start,
                                                              const float *__restrict__ tab, const float *__restrict__ thr, const u32x4 *__restrict__ image,
                                                              const spectro::BankTiles *__restrict__ tiles, uint32_t n_tiles, const SpecArgs a) {
    constexpr uint32_t M = N / 2, RR = M / 64, W = RR / 2, LR = band::ilog2(RR);
    constexpr uint32_t SW = spectro::bank_stride(N) / 2, PW = spectro::TILE_FRAMES * SW;  // words of a row, of a plane
    extern __shared__ __align__(16) uint32_t spec_lds[];
    float *thr_l = reinterpret_cast<float *>(spec_lds);
    uint32_t *bad_l = spec_lds + THR_WORDS;
    uint32_t *planes = spec_lds + HEAD_WORDS;  // hi, mid, lo: [frame][SW] words each
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = __builtin_amdgcn_readfirstlane(t >> 6), t0 = blockIdx.x * spectro::TILE_FRAMES;
    if (a.u8 && t < spectro::N_THR) thr_l[t] = thr[t];
    band::BandFft<N> fft;
    transform_tile<N>(src, n_samples, start, tab, a, t0, lane, wave, bad_l, fft, [&](uint32_t f, const float(&e)[RR], float e_top) {
        uint32_t *row = planes + f * SW;
        uint32_t h[W], m[W], l[W];
#pragma unroll
        for (uint32_t p = 0; p < W; p++) split3_pair(e[band::bitrev(2 * p, LR)], e[band::bitrev(2 * p + 1, LR)], h[p], m[p], l[p]);
        uint32_t *at = row + fft.L * W;  // bins L RR ..: W words, a multiple of W words in
        if constexpr (W >= 4) {
#pragma unroll
            for (uint32_t q = 0; q < W; q += 4) {
                *reinterpret_cast<u32x4 *>(at + q) = u32x4{h[q], h[q + 1], h[q + 2], h[q + 3]};
                *reinterpret_cast<u32x4 *>(at + PW + q) = u32x4{m[q], m[q + 1], m[q + 2], m[q + 3]};
                *reinterpret_cast<u32x4 *>(at + 2 * PW + q) = u32x4{l[q], l[q + 1], l[q + 2], l[q + 3]};
            }
        } else if constexpr (W == 2) {
            *reinterpret_cast<uint2 *>(at) = uint2{h[0], h[1]};
            *reinterpret_cast<uint2 *>(at + PW) = uint2{m[0], m[1]};
            *reinterpret_cast<uint2 *>(at + 2 * PW) = uint2{l[0], l[1]};
        } else {
            at[0] = h[0], at[PW] = m[0], at[2 * PW] = l[0];
        }
        // bin N/2 and the zeros up to the padded depth: words M/2 .. M/2 + 15 (e_top is 0.0f in every lane but 0)
        if (lane < 16) {
            uint32_t th, tm, tl;
            split3_pair(e_top, 0.0f, th, tm, tl);
            row[M / 2 + lane] = th, row[PW + M / 2 + lane] = tm, row[2 * PW + M / 2 + lane] = tl;
        }
    });
    __syncthreads();

    const uint32_t li = lane & 15u, lg = lane >> 4;
    // 16-byte units: a row is SW / 4 of them, a plane PW / 4; the lane's window at step s starts at frag + 4 s
    const u32x4 *bh = reinterpret_cast<const u32x4 *>(planes) + li * (SW / 4) + lg, *bm = bh + PW / 4, *bl = bm + PW / 4;
    const bool here = t0 + li < a.n_frames;  // the frame of this lane's column exists
    const bool bad = here && bad_l[li] != 0;
    const size_t row_at = (size_t)(t0 + li) * a.n_rows;
    for (uint32_t j = wave; j < n_tiles; j += spectro::WAVES) {
        const uint32_t s0 = tiles->first[j], cnt = tiles->count[j];
        const u32x4 *img = image + (size_t)tiles->offset[j] * 192 + lane;
        floatx4 acc{0.0f, 0.0f, 0.0f, 0.0f};
        u32x4 ah = img[0], am = img[64], al = img[128];
        for (uint32_t s = 0; s < cnt; s++) {
            const uint32_t sn = s + 1 < cnt ? s + 1 : s;  // the last step loads itself again: no read past the tile's fragments
            const u32x4 nh = img[sn * 192], nm = img[sn * 192 + 64], nl = img[sn * 192 + 128];
            acc = mm6(ah, am, al, bh[4 * (s0 + s)], bm[4 * (s0 + s)], bl[4 * (s0 + s)], acc);
            ah = nh, am = nm, al = nl;
        }
        if (!here) continue;
        const uint32_t m0 = spectro::TILE_ROWS * j + 4 * lg;  // this lane's first row
        if (m0 >= a.n_rows) continue;
        if (bad) acc = floatx4{__builtin_inff(), __builtin_inff(), __builtin_inff(), __builtin_inff()};
        if (!a.u8) {
            float *o = static_cast<float *>(out) + row_at + m0;
            if ((a.n_rows & 3u) == 0) {
                *reinterpret_cast<floatx4 *>(o) = acc;
            } else {
#pragma unroll
                for (uint32_t r = 0; r < 4; r++)
                    if (m0 + r < a.n_rows) o[r] = acc[r];
            }
        } else {
            uint8_t *o = static_cast<uint8_t *>(out) + row_at + m0;
            const uint32_t c0 = code_of(thr_l, acc[0]), c1 = code_of(thr_l, acc[1]), c2 = code_of(thr_l, acc[2]), c3 = code_of(thr_l, acc[3]);
            if ((a.n_rows & 3u) == 0) {
                *reinterpret_cast<uint32_t *>(o) = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
            } else {
                const uint32_t c[4] = {c0, c1, c2, c3};
#pragma unroll
                for (uint32_t r = 0; r < 4; r++)
                    if (m0 + r < a.n_rows) o[r] = (uint8_t)c[r];
            }
        }
    }
}

template <uint32_t N, class R>
void launch_one(hipStream_t s, void *out, const R &rd, uint64_t n_samples, uint64_t start, uint32_t blocks, const float *tab, const float *thr, const void *image,
                const spectro::BankTiles *tiles, uint32_t n_tiles, bool bank, const SpecArgs &args) {
    if (bank)
        hipLaunchKernelGGL((spectrogram_bank_kernel<N, R>), dim3(blocks), dim3(spectro::LANES), spectro::bank_lds_bytes(N), s, out, rd, n_samples, start, tab, thr,
                           static_cast<const u32x4 *>(image), tiles, n_tiles, args);
    else
        hipLaunchKernelGGL((spectrogram_bins_kernel<N, R>), dim3(blocks), dim3(spectro::LANES), spectro::bins_lds_bytes(N), s, out, rd, n_samples, start, tab, thr, args);
}

LdsOptIn g_spectrogram_lds;

// the kernels of frame 2048, for every reader pcm_visit knows
template <class... R>
hipError_t opt_in(int device) {
    constexpr uint32_t N = band::FRAME_MAX;
    return g_spectrogram_lds.prepare(device, {LdsOptIn::Kernel{(const void *)spectrogram_bins_kernel<N, R>, spectro::bins_lds_bytes(N)}...,
                                              LdsOptIn::Kernel{(const void *)spectrogram_bank_kernel<N, R>, spectro::bank_lds_bytes(N)}...});
}

}  // namespace

hipError_t spectrogram_prepare(int device) {
    return opt_in<PcmMono<int16_t>, PcmMono<float>, PcmFrames<BN_PCM_I16>, PcmFrames<BN_PCM_F32>, PcmFrames<BN_PCM_I24>, PcmFrames<BN_PCM_I32>,
                  PcmFrames<BN_PCM_U8>>(device);
}

void launch_spectrogram(hipStream_t s, void *out, const PcmSrc &src, uint64_t n_samples, uint64_t start, uint32_t n_frames, const spectro::Plan &plan,
                        const float *tab, float scale, const float *thr, const void *image, const spectro::BankTiles *tiles, uint32_t n_tiles) {
    if (n_frames == 0) return;
    const bool u8 = plan.format == BN_SPECTROGRAM_U8;
    if (!band::frame_ok(plan.N) || plan.hop == 0 || plan.hop > plan.N || plan.n_rows == 0 || start > n_samples || n_frames > spectro::piece_frames(plan.n_rows) ||
        !tab || !out || !ptr_aligned16(out) || (u8 && !thr) ||
        (plan.bank ? (!image || !tiles || !ptr_aligned16(image) || n_tiles != (plan.n_rows + spectro::TILE_ROWS - 1) / spectro::TILE_ROWS || n_tiles > spectro::MAX_ROW_TILES)
                   : (plan.lo >= plan.hi || plan.hi > plan.N / 2 + 1 || plan.n_rows != plan.hi - plan.lo))) {
        launch_error("spectrogram: a plan the kernels cannot take");
        return;
    }
    const SpecArgs args{plan.lo, plan.n_rows, plan.hop, n_frames, u8 ? 1u : 0u, scale};
    const uint32_t blocks = (n_frames + spectro::TILE_FRAMES - 1) / spectro::TILE_FRAMES;
    const bool known = pcm_visit(src, [&](auto rd) {
        using R = decltype(rd);
        switch (plan.N) {
            case 256: launch_one<256, R>(s, out, rd, n_samples, start, blocks, tab, thr, image, tiles, n_tiles, plan.bank, args); break;
            case 512: launch_one<512, R>(s, out, rd, n_samples, start, blocks, tab, thr, image, tiles, n_tiles, plan.bank, args); break;
            case 1024: launch_one<1024, R>(s, out, rd, n_samples, start, blocks, tab, thr, image, tiles, n_tiles, plan.bank, args); break;
            default: launch_one<2048, R>(s, out, rd, n_samples, start, blocks, tab, thr, image, tiles, n_tiles, plan.bank, args); break;
        }
    });
    if (!known) launch_error("spectrogram: a layout no reader knows");
}

}  // namespace bn
