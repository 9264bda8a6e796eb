// What the scans that stream an index's slab in 64-row tiles for up to 64 lists (queries, classes) of a pass have in common by
// definition: the constants and the layout of their dynamic LDS.  index.hip (index_scan_kernel), subset.hip (subset_scan_kernel),
// peaks.hip (peaks_scan_kernel) and rank.hip (rank_scan_kernel) carve their LDS from Layout's offsets and size their launches by
// Layout::BYTES.  Each keeps its own copy of the tile loop: written as instantiations of one templated body the subset, peaks and
// exact-search kernels measured slower than their hand-written forms ("One layout and one host path").  above.hip
// (above_scan_kernel) keeps a copy of the loop too, over the smaller AboveLayout below.
// Include from a .hip file.
#pragma once
#include <cstddef>

#include "topm_select.h"

namespace bn {
namespace scan {

using topm::Cand;
using topm::MMAX;
using topm::PEND;

constexpr int KC = 128;        // k-step of the scan; slab, query and weight rows are padded to a multiple of it
constexpr int TILE = 64;       // rows per workgroup tile: 4 waves x 16 rows
constexpr int LP = 64;         // lists per scan pass
constexpr int QS_LD = KC + 4;  // words of a list's k chunk in LDS
constexpr int S_LD = TILE + 1;
constexpr int PLANE = LP * S_LD;  // words of one tile's scores; a multiple of 64, so several planes share their bank phase

// the dynamic LDS of a scan that keeps PLANES tiles of scores, as byte offsets
template <int PLANES>
struct Layout {
    static constexpr size_t B = 0;                                           // float [LP][QS_LD]: the lists' current k chunk
    static constexpr size_t S = B + (size_t)LP * QS_LD * 4;                  // float [PLANES][LP][S_LD]: tile scores
    static constexpr size_t PENDING = S + (size_t)PLANES * PLANE * 4;        // Cand [LP][PEND]
    static constexpr size_t SCRATCH = PENDING + (size_t)LP * PEND * sizeof(Cand);  // Cand [4][MMAX]: one merge scratch per wave
    static constexpr size_t THR = SCRATCH + 4 * MMAX * sizeof(Cand);         // Cand [LP]: a full list's M-th entry
    static constexpr size_t LEN = THR + LP * sizeof(Cand);                   // int [LP]: entries of the running list
    static constexpr size_t PN = LEN + LP * sizeof(int);                     // int [LP]: entries of the pending list
    static constexpr size_t BYTES = PN + LP * sizeof(int);
};
static_assert(Layout<1>::BYTES == 125184 && Layout<3>::BYTES == 158464, "the scans' LDS sizes are part of their launch contract");
static_assert(Layout<3>::BYTES <= 160 * 1024, "gfx950 has 160 KB of LDS per workgroup");
static_assert(Layout<1>::S % 16 == 0 && PLANE % 64 == 0, "float4 stores of the k chunk; planes of equal bank phase");

// the dynamic LDS of the threshold scan (above.hip, above_scan_kernel): Layout<1>'s k chunk and score plane at the same offsets, then
// one threshold and one running hit count per list.  It selects nothing, so it has no pending lists, merge scratch or running M-th
struct AboveLayout {
    static constexpr size_t B = Layout<1>::B;                 // float [LP][QS_LD]
    static constexpr size_t S = Layout<1>::S;                 // float [LP][S_LD]
    static constexpr size_t THR = S + (size_t)PLANE * 4;      // float [LP]: min_score of the list
    static constexpr size_t CNT = THR + LP * sizeof(float);   // uint32 [LP]: hits of the list in this workgroup's tiles so far
    static constexpr size_t BYTES = CNT + LP * sizeof(unsigned);
};
static_assert(AboveLayout::BYTES == 50944, "the threshold scan's LDS size is part of its launch contract");
static_assert(AboveLayout::BYTES <= 64 * 1024, "below the size from which a kernel must opt in; three workgroups fit a CU's 160 KB");

}  // namespace scan
}  // namespace bn
