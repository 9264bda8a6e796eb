// The host-side arithmetic of the spectral profile (recording.cpp: bn_recording_spectral_profile; kernel in spectral_profile.hip) that
// needs neither a device nor the runtime: a spec checked and copied, the frames of a window (band_plan.h's, which this header
// includes: frames, span, the unread tail, the last sample a window range reads), the run of consecutive frames each wave owns and
// the one frame past it that it transforms for the difference across the boundary, the LDS a workgroup takes and where a bin lies in
// it, the floats of `out_bins` without a product that can wrap, and the windows of one launch.  Host code only, so that a stand-alone
// program can run it under a sanitizer (tools/asan_profile_plan.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>

#include "band_plan.h"

namespace bn {
namespace profile {

constexpr uint32_t LANES = band::LANES, WAVES = band::WAVES;  // one workgroup per window, wave w owns frames [w q, (w + 1) q)
using band::last_sample_read;

// a checked spec with what follows from it and S
struct Plan {
    uint32_t N = 0, hop = 0, lo = 0, hi = 0;
    uint32_t n_bins = 0;    // hi - lo
    uint32_t n_frames = 0;  // (S - N) / hop + 1
    uint32_t span = 0;      // window positions [0, span) are read
    uint32_t unread = 0;    // S - span < hop
    uint32_t run = 0;       // q = ceil(n_frames / WAVES): the frames a wave owns
};

// The plan of (spec, S).  Refuses a NULL spec and a spec_size below the struct's; the frame, hop, S and the bin range are band
// levels' refusals of a spec with this one band (band::check_spec).  The spec is read through memcpy: any alignment
inline bn_status check_spec(const bn_profile_spec *spec, size_t spec_size, uint64_t S, Plan *out) {
    if (!spec) return set_last_error(BN_ERR_INVALID_ARG, "null profile spec");
    if (spec_size < sizeof(bn_profile_spec)) return set_last_error(BN_ERR_INVALID_ARG, "spec_size is below sizeof(bn_profile_spec)");
    bn_profile_spec s;
    memcpy(&s, spec, sizeof(s));
    bn_band_spec b{};
    b.frame = s.frame, b.hop = s.hop, b.n_bands = 1, b.bin_lo[0] = s.bin_lo, b.bin_hi[0] = s.bin_hi;
    band::Plan bp;
    if (bn_status st = band::check_spec(&b, sizeof(b), S, &bp); st != BN_OK) return st;
    *out = Plan{};
    out->N = bp.N, out->hop = bp.hop, out->lo = bp.lo[0], out->hi = bp.hi[0], out->n_bins = bp.hi[0] - bp.lo[0];
    out->n_frames = bp.n_frames, out->span = bp.span, out->unread = bp.unread;
    out->run = bp.n_frames / WAVES + (bp.n_frames % WAVES != 0);  // no n_frames + 3: n_frames may be 2^32 - 256
    return BN_OK;
}

// Wave w of a window of F frames in runs of q: it owns frames [*first, *end) -- they add to all three planes -- and, if *extra, also
// transforms frame *end, the first of the next run, for the one difference |A[end] - A[end - 1]| (plane 2 only).  A wave past the
// last frame owns nothing (*first == *end, no extra).  w * q is formed in 64 bits
constexpr void wave_frames(uint32_t F, uint32_t q, uint32_t w, uint32_t *first, uint32_t *end, bool *extra) {
    const uint64_t f0 = (uint64_t)w * q, f1 = f0 + q;
    *first = (uint32_t)(f0 < F ? f0 : F);
    *end = (uint32_t)(f1 < F ? f1 : F);
    *extra = *first < *end && *end < F;
}

// Where bin k of a frame of N samples lies in a wave's row of N/2 + 1 floats.  A lane holds RR = N / 128 consecutive bins, so one
// store of a register puts the 64 lanes RR floats apart; the low bits of the index are xor-ed with the bits above bit 4, which
// spreads each half of the wave (32 lanes, as the LDS takes them) over all 32 banks.  A bijection of [0, N/2]; bin N/2 stays
constexpr uint32_t lds_index(uint32_t N, uint32_t k) { return k ^ ((k >> 5) & (N / 64 - 1)); }

// What a workgroup holds in LDS: per wave and plane a row of N/2 + 1 partial sums, and per wave its total, its share of the ACI and
// its non-finite flag
constexpr uint32_t lds_bytes(uint32_t N) { return WAVES * (BN_PROFILE_PLANES * (N / 2 + 1) + 3) * (uint32_t)sizeof(float); }

// count * BN_PROFILE_PLANES * n_bins, the floats of out_bins; false if that is not a size_t's worth of bytes
inline bool bins_floats(size_t count, uint32_t n_bins, size_t *out) {
    const size_t per = (size_t)BN_PROFILE_PLANES * n_bins;  // <= 3 * 1025
    if (per == 0 || count > SIZE_MAX / sizeof(float) / per) return false;
    *out = count * per;
    return true;
}

// windows per launch: at most 2^20 (band levels' cut), and planes of at most 2^26 floats on the device
constexpr size_t piece_windows(uint32_t n_bins) {
    const size_t by_planes = ((size_t)1 << 26) / ((size_t)BN_PROFILE_PLANES * (n_bins ? n_bins : 1));
    return by_planes < ((size_t)1 << 20) ? by_planes : ((size_t)1 << 20);
}

}  // namespace profile
}  // namespace bn
