// template_match_kernel -- the kernel of bn_recording_template_match (launched by recording.cpp; declaration in template.h, geometry,
// the packed templates and the launch pieces in template_plan.h, the rule in include/birdnet_hip.h, "Template matching").  Stage 1
// of a call is launch_spectrogram writing a U8 code image to the device; this is stage 2: for every template q and frame offset t
// the exact integer sums A = sum tau s, S1 = sum s, S2 = sum s^2 over the template's W_q x R patch at t, and from them the Pearson
// correlation in int64 and double.  A[q][t] = sum_{w,j} tau_q[w][j] s[t + w][j] is a Toeplitz product on
// v_mfma_i32_16x16x64_i8, read straight out of an LDS copy of the image: no im2col.  Templated on the number of 16-template tiles.
//
// TILE.  A workgroup of 256 lanes owns tmatch::TILE_OFFSETS = 64 consecutive offsets, each wave 16 of them, one column block of the
// matrix instruction.  It copies the 63 + Wmax frame rows it needs (and three spare rows, below) from the image into LDS rows
// `stride` bytes apart and flips bit 7 of every byte: s = c - 128 as an int8 is c ^ 0x80.  A row is U = ceil(R / 16) UNITS of 16
// bytes; P = the power of two at or above U consecutive lanes take one row, a unit each, so a wave moves 64 / P rows at a time.
// The global reads are one 16-byte load per unit where R is a multiple of 16 (every row of the image is then aligned), four dword
// loads where it is a multiple of 4, sixteen byte loads otherwise; the LDS write is one ds_write_b128 either way.  The bytes
// R .. 16 U - 1 of a row, rows past the image and the spare rows are written as 0, the value that multiplies to nothing.
//   * Sums.  While a unit is in registers the lane adds up its sixteen s and s^2; the P lanes of a row combine them by
//     log2 P exchanges and the row's first lane keeps both per frame in LDS.  After a barrier wave 0 turns the 63 + Wmax row sums into
//     exclusive prefixes (three rows per lane, one wave scan): S1 and S2 of any (offset, length) are two subtractions, so templates
//     of any lengths in one set cost nothing.  Every prefix fits: 191 * 512 * 128^2 < 2^31.
//   * Frames past the image's end belong to offsets at or past n_offsets only; those lanes are masked at the store.
//
// B OPERAND.  K is ordered (frame w, then unit): unit u = w U + ju.  A K step is four units and lane (i = lane & 15, g = lane >> 4)
// reads unit 4 sigma + g of offset i: ONE ds_read_b128 at row (offset + w), byte 16 ju.  A step may straddle two frames (or, for
// U < 4, more): each lane carries its own (w, ju) as an LDS address and steps it by four units with one conditional wrap, no
// division in the loop.  The last step of the longest tile can reach up to three units past Wmax U, where every A byte is zero:
// the three spare rows keep those reads inside the image's LDS.
//   Bank conflicts.  ds_read_b128 is served in four 16-lane groups (gemm_b3.hip, spectrogram.hip): {0-3, 12-15, 20-27} is g = 0 with
//   i in {0..3, 12..15} and g = 1 with i in {4..11}.  Inside one frame the lane's 16-byte slot in the 256-byte bank row is
//   ((offset + w) r + ju0 + g) mod 16, r = stride / 16.  tmatch::stride pads a row to 32 bytes mod 64, so r = 2 q with q odd and
//   i r mod 16 = 2 (q i mod 8) is a bijection of i mod 8 onto the even slots; both i-sets of a group are complete residue systems
//   mod 8, so g = 0 takes eight slots of one parity and g = 1 the eight of the other: sixteen distinct slots, no conflict;
//   {4-11, 16-19, 28-31} and the two groups of g = 2, 3 likewise (spectrogram.hip's argument with the row offset ju0 added to both).
//   Where a step straddles frames between g and g + 1 the second set is shifted by r - U instead of 1: the parities still differ when
//   U is even, and when U is odd the two sets of eight can meet, at most 2-way, in the one or two steps per frame that straddle.
//   The padding costs at most 48 bytes a row.
//
// A OPERAND.  bn_templates_create packed the templates on the host in fragment order (tmatch::pack): per tile of 16 templates and
// step one 1-KiB fragment, lane (i, g) holding the sixteen tau of template 16 j + i at unit 4 sigma + g, zeros for the rows
// R .. 16 U - 1, behind a template's own W_q U units and for the templates past n_templates.  A tile runs to the step count of its
// longest member (tmatch::Tiles); the wave loops to the longest tile's and a shorter tile drops out wave-uniformly.
//
// ACCUMULATE.  One int32x4 accumulator per tile, NT <= 4.  Per step: the next step's NT fragments are requested from global memory,
// the B fragment is read once from LDS, one MFMA per tile (as fir.hip and the spectrogram's bank kernel do).  |A| <= 2^30.
//
// FINISH AND STORE.  Lane (i, g) holds A of templates 16 j + 4 g .. + 3 at offset i.  With the template's K, T1, dT
// (tmatch::Meta) and S1, S2 from the prefixes: num = K A - T1 S1 and dS = K S2 - S1^2 in int64, score = (float)((double)num /
// sqrt((double)dT * (double)dS)), +0.0f where dS == 0; the product, the root and the quotient are IEEE double operations (no
// contraction, correctly rounded sqrt and division).  The scores go to LDS as [template][68] floats over the image's bytes, once
// every wave is past its last B read (68: the four g of a write fall 16 banks apart), and leave as one contiguous run of up to 64
// floats per template, a dword per lane, masked to n_offsets and n_templates: rows of the output start at any dword, so dword
// stores are the full-width form.
//
// Dynamic LDS (tmatch::lds_bytes): the two prefixes (1 536 bytes), then (66 + Wmax) rows of `stride` bytes or the scores, whichever
// is more: 107 072 bytes at 128 frames x 512 rows, which needs the opt-in beyond 64 KiB (template_match_prepare).  No atomics, no
// private segment, no inline assembly, vector stores only.  Registers per instantiation NT = 1 / 2 / 3 / 4: 36 / 48 / 64 / 80 VGPRs, no
// AGPRs, 87 SGPRs; LDS 5 888 bytes at one template of 1 x 1 up to the 107 072 ("Template matching").
#include "template.h"

#include "capi_internal.h"
#include "device_common.h"
#include "kernels.h"
#include "plan_rules.h"

namespace bn {
namespace {

typedef int intx4 __attribute__((ext_vector_type(4)));
constexpr uint32_t SCORE_LD = tmatch::SCORE_LD;

// what the kernel needs of a launch, as kernel arguments (scalar registers)
struct MatchArgs {
    uint32_t n_rows, units, lp;     // R, U, log2 P
    uint32_t stride;                // bytes of an LDS row
    uint32_t wmax;                  // the set's longest template
    uint32_t align;                 // 16, 4 or 1: what R is a multiple of
    uint32_t n_image_frames, n_offsets, n_templates;
};

// sixteen codes of image row `p` from byte j0 on, bit 7 flipped, 0 at and past byte R
__device__ __forceinline__ u32x4 load_unit(const uint8_t *__restrict__ p, uint32_t j0, uint32_t R, uint32_t align) {
    u32x4 v{0u, 0u, 0u, 0u};
    if (align == 16) {
        v = *reinterpret_cast<const u32x4 *>(p + j0) ^ 0x80808080u;
    } else if (align == 4) {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++)
            if (j0 + 4 * k < R) v[k] = *reinterpret_cast<const uint32_t *>(p + j0 + 4 * k) ^ 0x80808080u;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            uint32_t d = 0;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++)
                if (j0 + 4 * k + b < R) d |= ((uint32_t)p[j0 + 4 * k + b] ^ 0x80u) << (8 * b);
            v[k] = d;
        }
    }
    return v;
}

template <int NT>
__global__ __launch_bounds__(256) void template_match_kernel(float *__restrict__ out, const uint8_t *__restrict__ img, const u32x4 *__restrict__ frag,
                                                            const tmatch::Meta *__restrict__ meta, const tmatch::Tiles tiles, const MatchArgs a) {
    extern __shared__ __align__(16) uint32_t tm_lds[];
    int32_t *p1 = reinterpret_cast<int32_t *>(tm_lds);  // [192]: row sums of s, then their exclusive prefix
    uint32_t *p2 = tm_lds + tmatch::PREFIX_ROWS;        // ... of s^2
    uint8_t *rows = reinterpret_cast<uint8_t *>(tm_lds + 2 * tmatch::PREFIX_ROWS);
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = __builtin_amdgcn_readfirstlane(t >> 6), t0 = blockIdx.x * tmatch::TILE_OFFSETS;
    const uint32_t U = a.units, n_sum = tmatch::sum_rows(a.wmax), n_rows_lds = tmatch::lds_rows(a.wmax);

    // ---- the image's rows to LDS, their sums on the way
    {
        const uint32_t P = 1u << a.lp, ju = lane & (P - 1), per = 64u >> a.lp;  // rows a wave moves at a time
        for (uint32_t rb = wave * per; rb < n_rows_lds; rb += tmatch::WAVES * per) {
            const uint32_t row = rb + (lane >> a.lp);
            const bool mine = row < n_rows_lds && ju < U;
            u32x4 v{0u, 0u, 0u, 0u};
            if (mine && t0 + row < a.n_image_frames) v = load_unit(img + (size_t)(t0 + row) * a.n_rows, ju * tmatch::UNIT, a.n_rows, a.align);
            int32_t s1 = 0, s2 = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
#pragma unroll
                for (uint32_t b = 0; b < 4; b++) {
                    const int32_t x = (int32_t)(v[k] << (24 - 8 * b)) >> 24;
                    s1 += x, s2 += x * x;
                }
            }
#pragma unroll
            for (uint32_t m = 1; m < 32; m <<= 1) {
                if (m < P) s1 += __shfl_xor(s1, (int)m), s2 += __shfl_xor(s2, (int)m);  // wave-uniform
            }
            if (mine) *reinterpret_cast<u32x4 *>(rows + row * a.stride + ju * tmatch::UNIT) = v;
            if (ju == 0 && row < n_sum) p1[row] = s1, p2[row] = (uint32_t)s2;
        }
    }
    __syncthreads();
    // ---- exclusive prefixes over the rows, entries 0 .. n_sum: lane L of wave 0 owns entries 3 L .. 3 L + 2
    if (wave == 0) {
        int32_t x[3];
        uint32_t y[3];
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            const bool in = 3 * lane + k < n_sum;
            x[k] = in ? p1[3 * lane + k] : 0, y[k] = in ? p2[3 * lane + k] : 0u;
        }
        int32_t sx = x[0] + x[1] + x[2];
        uint32_t sy = y[0] + y[1] + y[2];
#pragma unroll
        for (uint32_t m = 1; m < 64; m <<= 1) {
            const int32_t ox = __shfl_up(sx, m);
            const uint32_t oy = __shfl_up(sy, m);
            if (lane >= m) sx += ox, sy += oy;
        }
        int32_t bx = sx - (x[0] + x[1] + x[2]);
        uint32_t by = sy - (y[0] + y[1] + y[2]);
#pragma unroll
        for (uint32_t k = 0; k < 3; k++) {
            p1[3 * lane + k] = bx, p2[3 * lane + k] = by;
            bx += x[k], by += y[k];
        }
    }
    __syncthreads();

    // ---- the product
    const uint32_t li = lane & 15u, lg = lane >> 4, off = wave * 16 + li;
    uint32_t cnt[NT], smax = 0;
    const u32x4 *fr[NT];
    intx4 acc[NT];
    u32x4 ac[NT], an[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
        cnt[j] = tiles.count[j];
        smax = cnt[j] > smax ? cnt[j] : smax;
        fr[j] = frag + (size_t)tiles.offset[j] * 64 + lane;
        acc[j] = intx4{0, 0, 0, 0};
        ac[j] = fr[j][0];  // a tile has at least one step
        an[j] = ac[j];
    }
    tmatch::UnitWalk walk(off, lg, U, a.stride);  // this lane's unit g of step 0, then four units on per step
    for (uint32_t s = 0; s < smax; s++) {
#pragma unroll
        for (int j = 0; j < NT; j++)
            if (s + 1 < cnt[j]) an[j] = fr[j][(size_t)(s + 1) * 64];
        const u32x4 b = *reinterpret_cast<const u32x4 *>(rows + walk.addr);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            if (s < cnt[j]) acc[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8((intx4)ac[j], (intx4)b, acc[j], 0, 0, 0);
            ac[j] = an[j];
        }
        walk.next();
    }
    __syncthreads();  // every wave is past its last read of the image: the scores take its place

    // ---- finish: lane (li, lg) holds templates 16 j + 4 lg + r at offset `off`
    float *sc = reinterpret_cast<float *>(rows);
    const int32_t base1 = p1[off];
    const uint32_t base2 = p2[off];
#pragma unroll
    for (int j = 0; j < NT; j++) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t q = tmatch::TILE_TEMPLATES * j + 4 * lg + r;
            const tmatch::Meta m = meta[q];  // a slot past n_templates is zeros: frames 0, K 0
            const int64_t S1 = p1[off + m.frames] - base1, S2 = (int64_t)(uint32_t)(p2[off + m.frames] - base2);
            const int64_t K = m.K, num = K * (int64_t)acc[j][r] - (int64_t)m.T1 * S1, dS = K * S2 - S1 * S1;
            float score = 0.0f;
            if (dS != 0) score = (float)((double)num / __builtin_sqrt((double)m.dT * (double)dS));
            sc[q * SCORE_LD + off] = score;
        }
    }
    __syncthreads();
    const bool here = t0 + lane < a.n_offsets;
    for (uint32_t q = wave; q < (uint32_t)NT * tmatch::TILE_TEMPLATES && q < a.n_templates; q += tmatch::WAVES)
        if (here) out[(size_t)q * a.n_offsets + t0 + lane] = sc[q * SCORE_LD + lane];
}

LdsOptIn g_template_lds;

}  // namespace

hipError_t template_match_prepare(int device) {
    constexpr size_t B = tmatch::MAX_LDS_BYTES;
    return g_template_lds.prepare(device, {LdsOptIn::Kernel{(const void *)template_match_kernel<1>, B}, LdsOptIn::Kernel{(const void *)template_match_kernel<2>, B},
                                           LdsOptIn::Kernel{(const void *)template_match_kernel<3>, B}, LdsOptIn::Kernel{(const void *)template_match_kernel<4>, B}});
}

void launch_template_match(hipStream_t s, float *out, const uint8_t *image, size_t n_image_frames, size_t n_offsets, const TemplateSet &set) {
    if (n_offsets == 0) return;
    if (!out || !image || !set.image || !set.meta || !ptr_aligned16(image) || !ptr_aligned16(set.image) || set.n_rows == 0 || set.n_rows > BN_TEMPLATE_MAX_ROWS ||
        set.max_frames == 0 || set.max_frames > BN_TEMPLATE_MAX_FRAMES || set.n_templates == 0 || set.n_templates > BN_TEMPLATE_MAX_COUNT ||
        set.n_tiles != (set.n_templates + tmatch::TILE_TEMPLATES - 1) / tmatch::TILE_TEMPLATES ||
        n_offsets > tmatch::piece_offsets(set.n_rows, set.max_frames, set.n_templates) || n_image_frames < n_offsets + (set.max_frames - 1) ||
        n_image_frames > spectro::piece_frames(set.n_rows)) {
        launch_error("template match: a plan the kernel cannot take");
        return;
    }
    for (uint32_t j = 0; j < set.n_tiles; j++)
        if (set.tiles.count[j] == 0 || set.tiles.count[j] > tmatch::steps(set.max_frames, set.n_rows)) {
            launch_error("template match: a tile's steps reach past the set's longest template");
            return;
        }
    const uint32_t U = tmatch::units(set.n_rows);
    uint32_t lp = 0;
    while ((1u << lp) < U) lp++;
    const MatchArgs a{set.n_rows, U, lp, tmatch::stride(set.n_rows), set.max_frames, set.n_rows % 16 == 0 ? 16u : (set.n_rows % 4 == 0 ? 4u : 1u),
                      (uint32_t)n_image_frames, (uint32_t)n_offsets, set.n_templates};
    const uint32_t blocks = (uint32_t)((n_offsets + tmatch::TILE_OFFSETS - 1) / tmatch::TILE_OFFSETS);
    const uint32_t lds = tmatch::lds_bytes(set.max_frames, set.n_rows, set.n_tiles);
    const u32x4 *frag = static_cast<const u32x4 *>(set.image);
    switch (set.n_tiles) {
        case 1: hipLaunchKernelGGL(template_match_kernel<1>, dim3(blocks), dim3(tmatch::LANES), lds, s, out, image, frag, set.meta, set.tiles, a); break;
        case 2: hipLaunchKernelGGL(template_match_kernel<2>, dim3(blocks), dim3(tmatch::LANES), lds, s, out, image, frag, set.meta, set.tiles, a); break;
        case 3: hipLaunchKernelGGL(template_match_kernel<3>, dim3(blocks), dim3(tmatch::LANES), lds, s, out, image, frag, set.meta, set.tiles, a); break;
        default: hipLaunchKernelGGL(template_match_kernel<4>, dim3(blocks), dim3(tmatch::LANES), lds, s, out, image, frag, set.meta, set.tiles, a); break;
    }
}

}  // namespace bn
