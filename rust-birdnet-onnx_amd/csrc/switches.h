// Every BN_* environment switch the library reads, declared ONCE: BN_SWITCH_TABLE below has one row per switch -- kind, name, default and
// one line on what it does -- and the typed accessors behind it are the only callers of getenv in csrc/.  A switch that is not a row, or
// an accessor of the wrong kind for a row, does not compile (every row is a constant of its kind's type in bn::sw).  Host-only: no HIP
// include, so the sanitizer build of the planner (tools/asan_plan.cpp) takes it as it is.
//
// Kinds (what the VALUE of the variable means; every read of a switch goes through exactly one of them):
//   present      set at all means on -- whatever the value, BN_X=0 included
//   on_unless_0  on by default; the exact text 0 turns it off (00, an empty value and any other text leave it on)
//   integer      atoi of the value (an empty or non-numeric value reads as 0), the default when unset
//   int64        atoll of the value, the default when unset
//   real         atof of the value, the default when unset
//   text         the value itself, the default when unset; sites compare it with the words the row names, any other word is the row's
//                "otherwise" case
// Where a row says "unset: ..." the default is computed at the reading site (sw_is_set) and the default column is not used.
//
// Nothing is cached here: a site that keeps a value in a `static const` reads it once per process, every other site reads per call,
// because the tests flip switches between the contexts they create.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

// clang-format off
#define BN_SWITCH_TABLE(X) \
    /* ---- C ABI layer (capi.cpp) */ \
    X(present,     BN_ALLOW_ANY_ARCH,     false,  "bn_model_load / bn_ctx_create accept a device that is not gfx950 (presence only: =0 also allows)") \
    X(present,     BN_NO_GRAPH,           false,  "every context runs its plan launch by launch, as with BN_CTX_NO_GRAPH (presence only: =0 also disables graphs)") \
    X(integer,     BN_STRICT_GRAPH,       0,      "non-zero: a capture that does not become a graph is an error instead of a counted fall-back (read once)") \
    X(on_unless_0, BN_CTX_STREAM_PRIO,    true,   "0 creates a context's stream at the default priority, in the queue pool the null stream and the caller's streams use (read once)") \
    X(integer,     BN_INPUT_MEMCPY,      0,      "non-zero: a caller's device input reaches the context's buffer by hipMemcpyAsync, not by the copy kernel (read once)") \
    X(integer,     BN_SDMA_COPY,          0,      "non-zero: results reach pinned host memory by hipMemcpyAsync, not by the kernel's own stores (read once)") \
    X(int64,       BN_STAGE_THREADS,      0,      "threads that stage host slices into pinned memory, clamped to 0 .. 64; unset: min(6, half the hardware threads)") \
    /* ---- recordings (recording.cpp), device groups (group.cpp) and live pools (live.cpp) */ \
    X(integer,     BN_UPLOAD_CHUNK_MB,    4,      "MiB per piece of a constants upload (at least 1)") \
    X(text,        BN_RCCL_LIB,           "",     "RCCL library to load and nothing else; unset: librccl.so.1, librccl.so, then the ROCm install's") \
    X(integer,     BN_GROUP_FORCE_RCCL,   0,      "non-zero: take the RCCL branch for ranks that share a device too (the test stub accepts such a communicator)") \
    X(present,     BN_GROUP_NO_RCCL,      false,  "gather with device copies even where RCCL would serve (presence only: =0 also disables RCCL)") \
    X(text,        BN_LIVE_SCATTER,       "direct", "copy = one async copy of the staging block, then the scatter on device memory; otherwise the kernel reads pinned memory") \
    /* ---- planner: graph rewrites, lowering, plan passes (engine.cpp, onnx_rewrite.cpp, dft_bank.cpp, plan_passes.cpp) */ \
    X(integer,     BN_CANON_SPECTRO,      1,      "0 keeps the STFT / DFT exporter dialects as written instead of rewriting them into the framing-conv form") \
    X(integer,     BN_CONVMERGE,          -1,     "framing Conv -> Transpose -> MatMul as one filter bank: 0 never, 1 wherever the pattern matches, otherwise where it is cheaper") \
    X(text,        BN_CONVFOLD,           "1",    "0 = no symmetric fold of framing convs (only the exact text 0)") \
    X(real,        BN_CONVFOLD_TOL,       1.1920929e-7, "x max|w|: how far the halves of a filter row may differ and still count as (anti)symmetric") \
    X(integer,     BN_CONVFOLD2,          1,      "0 keeps the half fold where the quarter fold of a cosine bank would apply (planner and launcher)") \
    X(text,        BN_STFT,               "auto", "which DFT banks run as FFT launches: 0 none, 1 every recognised bank (BN_CONVMERGE then merges only when =1), otherwise by estimated cost") \
    X(int64,       BN_STFT_MINBINS,       0,      "banks with fewer live bins than this stay on the matrix path") \
    X(real,        BN_STFT_TOL,           4e-7,   "x max|row|: how far a filter bank's taps may lie from the windowed DFT model it is recognised as") \
    X(present,     BN_STFT_DEBUG,         false,  "the PLANNER prints what its DFT-bank recognition found (presence only); not BN_STFT_DBG") \
    X(text,        BN_STFT_MEL,           "1",    "mel bank inside the STFT launch: 0 never, force also with tiles of 8 frames where 16 do not fit, otherwise where 16 fit") \
    X(on_unless_0, BN_STFT_MELMFMA,       true,   "0 keeps the absorbed mel bank's (column, weight) lists on the vector ALU") \
    X(on_unless_0, BN_STFT_PRE,           true,   "0 keeps the per-sample scalar chain ahead of an STFT a launch of its own") \
    X(on_unless_0, BN_STFT_POWER,         true,   "0 keeps the power / magnitude pass behind a cos | sin bank a launch of its own") \
    X(integer,     BN_STFT_PAD,           1,      "0 keeps the zero-padded copy of the signal a padded framing conv reads") \
    X(integer,     BN_FRAME_PRE,          1,      "0: a folded framing GEMM does not take the signal's scalar chain into its span load") \
    X(on_unless_0, BN_GEMMPOST,           true,   "0 keeps elementwise chains behind a GEMM out of its epilogue") \
    X(integer,     BN_GEMMGAP,            1,      "0 keeps GlobalAveragePool behind a 1x1 conv a launch of its own") \
    X(integer,     BN_SEGEMM,             0,      "exactly 1: squeeze-excite in the prologue of the project GEMM (measured slower, kept under test)") \
    X(text,        BN_SEFUSE,             "0",    "squeeze-excite finished by the launch that produced the sums: dw, mb, or 1 for both; otherwise off (measured slower)") \
    X(on_unless_0, BN_REDUCE_SHIFT,       true,   "0 keeps max(x - s) / min(x - s) as written instead of reducing x itself") \
    X(on_unless_0, BN_REDUCE_SPLIT,       true,   "0 keeps a whole-segment min / max one block per sample") \
    X(on_unless_0, BN_REDUCE_PAIR,        true,   "0 keeps min and max over the same input separate launches") \
    X(on_unless_0, BN_DWMAP,              true,   "0 keeps small feature maps off the whole-map depthwise kernel") \
    X(integer,     BN_DWMAPT,             1,      "0 keeps the whole-map depthwise conv off the instances with the map size at compile time") \
    X(text,        BN_MBFUSE,             "auto", "expand conv + depthwise conv in one launch: 0 never (stem included), force every eligible pair, otherwise by the shape rule") \
    X(integer,     BN_MBFUSE_MAXK,        48,     "largest expand K the fused MBConv takes (the kernel caps it at 48)") \
    X(real,        BN_MBFUSE_HALO,        3.0,    "largest halo recompute factor the fused MBConv accepts") \
    X(on_unless_0, BN_STEMFUSE,           true,   "0 keeps the stem conv out of the fused MBConv launch") \
    X(text,        BN_MBMAP,              "0",    "the exact text 1: round 1's whole-map fused MBConv (measured slower); otherwise off") \
    X(int64,       BN_MBMAP_MAXHW,        512,    "largest map (pixels) the whole-map fused MBConv forms take") \
    X(text,        BN_MBROW,              "auto", "row-streaming MBConv: 0 keeps the tiled kernels, force takes it regardless of strip utilisation, otherwise from 0.7 up") \
    X(text,        BN_MBROW_TR,           "auto", "row-streaming MBConv along the map's height: 0 never, 1 wherever the kernel supports it, otherwise by utilisation") \
    X(integer,     BN_MBROW_B3,           1,      "0 keeps the row-streaming MBConv's expand on the exact-f32 instruction") \
    X(integer,     BN_MBROW_TOH,          0,      "band height of the row-streaming MBConv (at least 1); unset: 8 or 12 rows, balanced over the map") \
    /* ---- shape rules shared by planner and launchers (plan_rules.h, kernels.h) */ \
    X(integer,     BN_FRAMELDS,           1,      "0 keeps folded framing GEMMs off the LDS-resident kernels") \
    X(integer,     BN_FRAME2_B3,          1,      "0 keeps the quarter-folded framing GEMM on the f32 forms (other bits)") \
    X(integer,     BN_FRAME2_WPK,         1,      "0 keeps the quarter-folded framing GEMM off its half-height form") \
    X(integer,     BN_GEMM3,              2,      "bf16x3 GEMMs: 0 exact-f32 kernels everywhere (fused MBConv expands too), 1 the LDS-DMA form only, 2 and above the register-staged form where it applies") \
    X(integer,     BN_GEMM3_KS,           0,      "1 or 2: K slices of the bf16x3 LDS-DMA GEMM; otherwise by K") \
    X(integer,     BN_GEMMDMA,            1,      "LDS-DMA GEMM: 0 never, 2 every eligible shape (tests), otherwise where it pays") \
    X(integer,     BN_GEMMDMA_KS,         0,      "1 or 2: K slices of the LDS-DMA GEMM; otherwise by K") \
    X(integer,     BN_GEMMDMA_SMALLN,     1,      "0 keeps the gated project convs with N <= 32 on the tiled kernel") \
    X(integer,     BN_SEGEMM_MAXC,        768,    "largest channel count whose excite products a GEMM block computes for itself (0 = never)") \
    X(integer,     BN_SPLITK_MINK,        256,    "smallest K the split-K GEMM takes (read once)") \
    X(integer,     BN_SPLITK_MAXROWS,     256,    "most rows per sample the split-K GEMM takes (read once)") \
    X(integer,     BN_MBMAP2,             1,      "0 keeps fused MBConv blocks off the LDS-resident small-map kernels") \
    X(integer,     BN_MBMAP3,             0,      "non-zero: round 4's small-map configurations (transposed, padded k, bands; measured slower)") \
    X(integer,     BN_MBMAP_BANDS,        1,      "0: with BN_MBMAP3, keeps the exact-f32 banded 8 x 32 configuration off") \
    X(integer,     BN_MBMAP_B3,           1,      "0 keeps the small-map kernels' expand on the exact-f32 instruction (and with it the wave-specialised kernel off)") \
    X(integer,     BN_MBMAP_WS,           1,      "0 keeps the small maps on mbmap.hip instead of the wave-specialised kernel") \
    X(integer,     BN_MBMAP_WS_SMALL,     1,      "0 keeps the 3 x 16 / 4 x 16 maps off the wave-specialised kernel") \
    X(integer,     BN_MBMAP_WS_BANDS,     1,      "0 keeps the 8 x 32 map in two bands off the wave-specialised kernel") \
    X(integer,     BN_MBMAP_WS_TR,        1,      "0: a 32 x 8 map is not walked transposed by the banded wave-specialised kernel") \
    X(integer,     BN_MBMAP_WS_DEEP,      1,      "0 keeps the 16 x 4 map with eight K steps off the wave-specialised kernel") \
    /* ---- launchers (*.hip): grids and tiles, never the arithmetic unless the row says so */ \
    X(int64,       BN_GEMMDMA_MINBLOCKS,  0,      "blocks a big tile must give before both LDS-DMA GEMMs take it; unset: 64, or 1 on a shared device") \
    X(integer,     BN_GEMMB3_MT,          0,      "2, 3 or 4: 16-row tiles per block of the register-staged bf16x3 GEMM") \
    X(integer,     BN_GEMMB3_NTW,         0,      "channel tiles per wave of the register-staged bf16x3 GEMM: 1 never two, 2 two wherever the block shape allows") \
    X(integer,     BN_FORCE_BN,           0,      "32, 64, 96 or 128: N tile of the tiled GEMM (experiments; read once)") \
    X(integer,     BN_FOLD_BN,            0,      "the same for folded framing GEMMs with N > 200 (experiments; read once)") \
    X(integer,     BN_FOLD_BN_NARROW,     0,      "the same for folded framing GEMMs with N <= 200; unset: BN_FOLD_BN (experiments; read once)") \
    X(integer,     BN_DEEPK_BN,           0,      "64, 96 or 128: N tile of the tiled GEMM for K >= 1024 (experiments; read once)") \
    X(integer,     BN_FORCE_SPLITK_BN,    0,      "32, 64 or 96: N tile of the split-K GEMM (experiments; read once)") \
    X(integer,     BN_FRAME_WN,           0,      "2 .. 5: wave columns of the LDS-resident framing GEMM (experiments; read once)") \
    X(integer,     BN_FRAME_KS,           2,      "anything but 2: no K slices in the framing GEMM with three wave columns (other bits)") \
    X(integer,     BN_FRAME_WALK,         -1,     "0 / positive: a framing GEMM block never / always walks all N tiles of its rows; negative: from 256 row blocks") \
    X(integer,     BN_SEFC_G,             0,      "exactly 4: a block of the squeeze-excite FC kernel serves four samples; otherwise one (read per call)") \
    X(integer,     BN_MBPIPE,             -1,     "software-pipelined fused MBConv: 0 never, 1 always, otherwise by the shape (bit-identical)") \
    X(integer,     BN_MBMAP2_NCH,         0,      "positive: channel chunks per block of the small-map kernels") \
    X(integer,     BN_MBMAP_SHARE,        0,      "positive: the share of the CUs the small-map kernels size their grid for (1 = the latency form); otherwise 2 on a shared device") \
    X(integer,     BN_MM_DBG,             0,      "bit mask: mbmap.hip skips phases to time the rest (wrong results)") \
    X(integer,     BN_STFT_DBG,           0,      "bit mask: the STFT KERNEL skips phases to time the rest (wrong results); not BN_STFT_DEBUG") \
    X(present,     BN_TOPK_EXACT,         false,  "top-K by the exact heap kernel alone, without the flagged fast path (presence only: =0 also forces it)") \
    X(present,     BN_TOPK_TWOPASS,       false,  "the fast top-K path by its general kernel even where the in-register one serves the row length (presence only)") \
    X(present,     BN_PRIOR_GENERAL,      false,  "priors attached or applied from here on keep the select kernel's keys in global scratch, as rows over 16384 species do (presence only)")
// clang-format on

namespace bn {

template <class T, int Kind>
struct SwRow {
    const char *name;
    T dflt;
};
using Sw_present = SwRow<bool, 0>;
using Sw_on_unless_0 = SwRow<bool, 1>;
using Sw_integer = SwRow<int, 2>;
using Sw_int64 = SwRow<int64_t, 3>;
using Sw_real = SwRow<double, 4>;
using Sw_text = SwRow<const char *, 5>;

namespace sw {
#define BN_SW_ROW(kind, name, dflt, doc) inline constexpr Sw_##kind name{#name, dflt};
BN_SWITCH_TABLE(BN_SW_ROW)
#undef BN_SW_ROW
}  // namespace sw

// the table as data: what the accessor test prints and compares with the rows above
struct SwInfo {
    const char *kind, *name, *dflt, *doc;
};
#define BN_SW_ROW(kind, name, dflt, doc) {#kind, #name, #dflt, doc},
inline constexpr SwInfo kSwitchTable[] = {BN_SWITCH_TABLE(BN_SW_ROW)};
#undef BN_SW_ROW

template <class T, int Kind>
inline bool sw_is_set(const SwRow<T, Kind> &s) { return getenv(s.name) != nullptr; }
inline bool sw_present(const Sw_present &s) { return sw_is_set(s); }
inline bool sw_on(const Sw_on_unless_0 &s) {
    const char *e = getenv(s.name);
    return !(e && strcmp(e, "0") == 0);
}
inline int sw_int(const Sw_integer &s) {
    const char *e = getenv(s.name);
    return e ? atoi(e) : s.dflt;
}
inline int64_t sw_i64(const Sw_int64 &s) {
    const char *e = getenv(s.name);
    return e ? atoll(e) : s.dflt;
}
inline double sw_double(const Sw_real &s) {
    const char *e = getenv(s.name);
    return e ? atof(e) : s.dflt;
}
inline const char *sw_text(const Sw_text &s) {
    const char *e = getenv(s.name);
    return e ? e : s.dflt;
}
inline bool sw_is(const Sw_text &s, const char *word) { return strcmp(sw_text(s), word) == 0; }

}  // namespace bn
