// A depthwise conv and the launch before it as one fused MBConv launch: the two rules that allow it (stem conv producer, 1x1 expand
// GEMM producer) and the one builder of the fused launch.  Reads the plan and the finished depthwise launch only; see plan_build.h.
#include "plan_build.h"
#include "plan_rules.h"

namespace bn {
namespace {

// What the fused launch takes from its producer, whichever rule accepted it.
struct Producer {
    const char *prefix = "";  // of the launch's name
    int32_t K = 0;            // depth of the first product: the GEMM's K, or the stem's im2col row k1 * k1 * Cin1
    int32_t act = ACT_NONE, has_bias = 0;
    float p0 = 0, p1 = 0;
    int64_t in_bs = 0;
    int32_t k1 = 0, s1 = 0, pt1 = 0, pl1 = 0, H1 = 0, W1 = 0, Cin1 = 0;  // stem only (MbDesc); k1 == 0: a 1x1 expand
    // how the kernel wants the producer's filters
    enum Pack {
        AS_IS,       // [C][K] as the GEMM had it
        ROWS,        // [C][K] rows padded with zeros to `KP`
        STEM_ROWS,   // [K][C] as lowered for the direct kernel -> [C][KP]: im2col column order (ky, kx, c)
        MBMAP_W3F,   // mbmap.hip's bf16x3 form: the filters in the order of its LDS chunk image (plan_rules.h)
        MBMAP_W3P    // mbmap_ws.hip: the filters as bf16 planes in fragment order (plan_rules.h)
    } pack = AS_IS;
    int64_t KP = 0;
    // small maps (expand only): 0 the tiled / row-streaming kernels, 1 round 1's whole-map kernel, 2 mbmap.hip / mbmap_ws.hip by `shape`
    int32_t whole_map = 0, map_b3 = 0, map_ws = 0;
    MbmapShape shape;
};

// `rows` rows of K floats as rows of KP >= K, the rest zeros; k_major: the source is [K][rows]
std::vector<float> pad_rows(const float *src, int64_t rows, int64_t K, int64_t KP, bool k_major = false) {
    std::vector<float> out((size_t)(rows * KP), 0.0f);
    for (int64_t r = 0; r < rows; r++)
        for (int64_t k = 0; k < K; k++) out[r * KP + k] = k_major ? src[k * rows + r] : src[r * K + k];
    return out;
}

// Fused MBConv blocks the row-streaming kernel takes (mbrow.hip: one wave per (band of output rows, strip of output
// columns, 32 mid channels), nothing in LDS): tiles_x / tiles_y become strips / bands -- the squeeze partials follow --
// and `halo` the pixels it expands per sample.  Per-sample shapes only, so a segment's bits do not depend on its batch.
// BN_MBROW=0 keeps the tiled kernels.
void row_streaming(MbDesc &m, double &halo) {
    if (sw_is(sw::BN_MBROW, "0")) return;
    if (!mbconv_row_supported(m)) return;
    const int outw = mbconv_row_outw(m.k, m.s);
    // a strip expands 32 halo columns for `outw` outputs whatever the map's width: on narrow maps (Perch: 32 or 16
    // columns against strips of 30 / 28 / 14) half of every strip is idle and the tiled kernel wins (measured: 0.53-0.57
    // utilisation -> 1.2-2.5x slower, 0.71 and above -> faster).  Round 3: such maps are usually TALL (Perch: 125 x 32,
    // 63 x 16) -- the kernel then streams along the map's rows' direction instead (MbDesc::row_tr: strips across the
    // height), if that fills its strips.  BN_MBROW=force takes the row kernel regardless (tests), BN_MBROW_TR=0 never
    // transposes, =1 always does where the kernel supports it
    const bool force = sw_is(sw::BN_MBROW, "force");
    const int strips = (m.OW + outw - 1) / outw, strips_t = (m.OH + outw - 1) / outw;
    const double util = (double)m.OW / (double)(strips * outw), util_t = (double)m.OH / (double)(strips_t * outw);
    bool tr = m.k1 == 0 && m.k == 3 && util_t >= 0.7 && util_t > util + 0.08;  // (5 x 5 instances: no register to spare for the second addressing form)
    if (sw_is(sw::BN_MBROW_TR, "0")) tr = false;
    if (sw_is(sw::BN_MBROW_TR, "1")) tr = m.k1 == 0 && m.k == 3;
    if (tr) {
        MbDesc probe = m;
        probe.row_tr = 1;
        if (!mbconv_row_supported(probe)) tr = false;
    }
    if (!force && !tr && util < 0.7) return;
    m.row_mode = 1;
    m.row_tr = tr ? 1 : 0;
    m.row_b3 = (sw_int(sw::BN_MBROW_B3) != 0 && sw_int(sw::BN_GEMM3) != 0 && m.k1 == 0 && m.Cin % 8 == 0) ? 1 : 0;
    const int rows_k = tr ? m.OW : m.OH, cols_k = tr ? m.OH : m.OW;  // the kernel's output rows / columns
    // band height: a band of toh output rows expands (toh - 1) s + k halo rows, so taller bands recompute less (12 rows of a
    // 5x5 block: 16 halo rows instead of 2 x 10) -- what several contexts sharing the chip pay for; a block with one or two
    // 32-channel chunks keeps 8 so that one context alone still has enough waves (stem: 38 us at 8, 48 us at 12)
    // (bands balanced: 16 rows are one band of 16, not 12 + 4)
    const int toh_target = (m.C + 31) / 32 >= 3 ? 12 : 8;
    const int nbands = std::max(1, (rows_k + toh_target / 2 - 1) / toh_target);
    const int toh_default = (rows_k + nbands - 1) / nbands;
    m.toh = std::min<int32_t>(rows_k, sw_is_set(sw::BN_MBROW_TOH) ? std::max(1, sw_int(sw::BN_MBROW_TOH)) : toh_default);
    m.tiles_x = (cols_k + outw - 1) / outw;
    m.tiles_y = (rows_k + m.toh - 1) / m.toh;
    halo = 32.0 * m.tiles_x * (double)m.tiles_y * ((m.toh - 1) * m.s + m.k);
}

// `pe` wrote, whole and at offset 0, the storage `dw` reads
bool feeds(const PlanOp &pe, const PlanOp &dw) {
    return pe.r.out.space == Space::ARENA && pe.r.out.id == dw.r.a.id && pe.r.out.offset == 0 && dw.r.a.offset == 0;
}

// Stem variant: the producer is a dense k1 x k1 convolution with few input channels (k1*k1*Cin1 <= 48,
// e.g. the 3x3 stride-2 conv over the 2-channel spectrogram image).  Its output tile is rebuilt from im2col
// rows staged in LDS and never written to HBM either (same kernel, different staging).  BN_STEMFUSE=0 disables.
bool stem_rule(const PlanOp &pe, const PlanOp &dw, Producer &p) {
    if (!sw_on(sw::BN_STEMFUSE)) return false;
    const DwDesc &d = dw.dw;
    const ConvDesc &cd = pe.conv;
    const bool stem = pe.kind == OpKind::CONV && feeds(pe, dw) && cd.groups == 1 && cd.kh == cd.kw && cd.sh == cd.sw && cd.dh == 1 && cd.dw == 1 &&
                      !cd.has_res && cd.Cin <= 4 && cd.kh * cd.kw * cd.Cin <= 48 && cd.OH == d.H && cd.OW == d.W && cd.Cout == d.C &&
                      act_keeps_zero(cd.act, cd.p0, cd.p1) && ((int64_t)d.H * d.W >= 3072 || sw_is(sw::BN_MBFUSE, "force"));
    if (!stem) return false;
    MbDesc probe{};
    probe.k = d.kw; probe.s = d.sw; probe.Cin = cd.kh * cd.kw * cd.Cin; probe.C = d.C;
    if (mbconv_lds_bytes(probe) > 150 * 1024) return false;
    p.prefix = "stem:";
    p.K = cd.kh * cd.kw * cd.Cin;
    p.act = cd.act; p.p0 = cd.p0; p.p1 = cd.p1; p.has_bias = cd.has_bias; p.in_bs = cd.in_bs;
    p.k1 = cd.kh; p.s1 = cd.sh; p.pt1 = cd.pt; p.pl1 = cd.pl; p.H1 = cd.H; p.W1 = cd.W; p.Cin1 = cd.Cin;
    p.pack = Producer::STEM_ROWS;
    p.KP = (p.K + 7) / 8 * 8;  // 8-wide K groups
    return true;
}

// expand 1x1 conv immediately before, consumed only here?  Then both run in one launch with the
// expanded tensor kept in LDS (mbconv_expand_dw_kernel): the 6x-expanded activation never
// touches HBM.  Measured on MI355X (batch 32, per pair): 48x256x16->96 s2: 101 -> 79 us,
// 24x128x24->144 s1: 80 -> 54 us, 5x5 s2: 60 -> 52 us, 12x64x40->240 5x5 s1: 54 -> 50 us; on
// the 6x32 maps (2 tiles per sample) and for K >= 80 the separate launches win, so the rule
// below keeps those unfused.  The rule only looks at per-sample shapes (batch invariance).
// BN_MBFUSE=0 disables, BN_MBFUSE=force fuses every eligible pair (tests).
bool expand_rule(const Plan &plan, const PlanOp &pe, const PlanOp &dw, Producer &p) {
    const DwDesc &d = dw.dw;
    const GemmDesc &g = pe.gemm;
    const int64_t H = d.H, W = d.W, OH = d.OH, OW = d.OW, k = d.kw, s = d.sw;
    const int maxk = std::min(48, sw_int(sw::BN_MBFUSE_MAXK));  // kernel: <= 6 K groups in registers
    // the kernel relies on act(0) == 0 for the expand activation (pixels outside the image)
    const bool act_zero = act_keeps_zero(g.act, g.p0, g.p1);
    const double maxhalo = sw_double(sw::BN_MBFUSE_HALO);
    // small feature maps can take the whole-map kernel (one block = 32 mid channels x the whole map:
    // no halo, any K up to 256, complete squeeze sums).  Opt-in (BN_MBMAP=1): measured on MI355X at
    // batch 32 it saves 10 launches and ~1% of single-stream latency, but its per-block fixed costs
    // (filter slab + A rows per 32-channel chunk, half the waves idle on 3x16 maps) make the
    // marginal cost per extra batch ~30% higher than GEMM + whole-map depthwise, and the three-
    // context throughput drops from 34.2k to 33.1k seg/s.
    const bool map_off = !sw_is(sw::BN_MBMAP, "1");
    const int64_t map_maxhw = sw_i64(sw::BN_MBMAP_MAXHW);
    const bool producer0 = pe.kind == OpKind::GEMM && feeds(pe, dw) && !g.has_scale && !g.has_res && g.rows == H * W && g.N == d.C && g.lda == g.K &&
                           g.K % 4 == 0 && pe.r.a.offset % 4 == 0 && !g.fold && !g.npost &&
                           (pe.r.a.space != Space::ARENA || plan.storages[pe.r.a.id].elems % 4 == 0);
    // Whole-map form with the INPUT resident in LDS (mbmap.hip, round 3): one block = one sample's map x a group of
    // mid channels, input fetched once per block by LDS-DMA, no staging on the vector ALU.  Default wherever a
    // configuration fits (192- and 48-pixel maps); BN_MBMAP2=0 disables.
    int map2 = 0;
    if (producer0) {
        MbDesc q{};
        q.H = d.H; q.W = d.W; q.Cin = g.K; q.C = d.C; q.OH = d.OH; q.OW = d.OW;
        q.k = d.kw; q.s = d.sw; q.pt = d.pt; q.pl = d.pl;
        q.act1 = g.act; q.act2 = d.act; q.in_bs = g.a_bs;
        p.shape = mbmap_shape(q);
        map2 = p.shape.cfg;
        p.map_b3 = mbmap_b3_steps(q, p.shape);
        p.map_ws = mbmap_ws_steps(q, p.shape);
    }
    const bool whole_map = map2 != 0 || (!map_off && H * W <= map_maxhw);
    const bool producer = producer0 && (map2 != 0 || g.K <= (whole_map ? 256 : maxk));
    // halo recompute factor of the expand conv: staged halo pixels / image pixels
    const int toh0 = s == 1 ? 8 : 4, tow0 = s == 1 ? 16 : 8;
    const int64_t hp = ((toh0 - 1) * s + k) * ((tow0 - 1) * s + k);
    const double halo_factor = (double)((hp + 31) / 32 * 32) * ((OW + tow0 - 1) / tow0) * ((OH + toh0 - 1) / toh0) / (double)(H * W);
    const bool force = sw_is(sw::BN_MBFUSE, "force");  // tests: small feature maps too
    // (round 3: stride-2 blocks on 768-pixel maps too -- with the row-streaming kernel the 12x64x40->240 s2 pair
    // runs in 17.5 us instead of 16.5 + 16.4, marginal cost per extra batch 8.6 against 24 us)
    const bool big_enough = H * W >= 768;
    MbDesc probe{};
    probe.k = d.kw; probe.s = d.sw; probe.Cin = producer ? g.K : 4; probe.C = d.C;
    probe.H = d.H; probe.W = d.W; probe.whole_map = whole_map ? 1 : 0;
    const bool fits = map2 != 0 || mbconv_lds_bytes(probe) <= 150 * 1024;
    const bool tiled_ok = act_zero && ((halo_factor <= maxhalo && big_enough) || force);
    if (!(producer && fits && (whole_map || tiled_ok))) return false;
    p.prefix = "mbconv:";
    p.K = g.K;
    p.act = g.act; p.p0 = g.p0; p.p1 = g.p1; p.has_bias = g.has_bias; p.in_bs = g.a_bs;
    p.whole_map = !whole_map ? 0 : map2 ? 2 : 1;
    // expand filters repacked for the kernel: [C][KP] rows = Cin weights | zeros (the bias starts the accumulators)
    if (p.whole_map == 2 && p.map_ws) p.pack = Producer::MBMAP_W3P;
    else if (p.whole_map == 2 && p.shape.cin_pad != g.K) {
        // mbmap.hip with padded k: the filter rows get the zeros the input rows get from the zero page
        p.pack = Producer::ROWS;
        p.KP = p.shape.cin_pad;
    } else if (p.whole_map == 2 && p.map_b3) p.pack = Producer::MBMAP_W3F;
    else if (whole_map) p.pack = Producer::AS_IS;
    else {
        p.pack = Producer::ROWS;
        p.KP = (g.K + 7) / 8 * 8;  // 8-wide K groups
    }
    return true;
}

// The one fused launch: `pe` (plan.ops.back()) described by `p`, then the depthwise conv `dw`
PlanOp fused_op(Plan &plan, const PlanOp &pe, const PlanOp &dw, const Producer &p, const std::string &node_name) {
    const DwDesc &d = dw.dw;
    PlanOp mb;
    mb.kind = OpKind::MBCONV;
    mb.name = p.prefix + pe.name.substr(pe.name.find(':') + 1) + "+" + node_name;
    mb.r.out = dw.r.out;
    mb.r.a = pe.r.a;
    const auto w0 = [&] { return plan.consts[pe.r.w.id].data() + pe.r.w.offset; };  // the producer's filters, where a packing reads them
    switch (p.pack) {
        case Producer::AS_IS: mb.r.w = pe.r.w; break;
        case Producer::ROWS: mb.r.w = Ref{Space::CONSTS, add_const(plan, pad_rows(w0(), d.C, p.K, p.KP)), 0}; break;
        case Producer::STEM_ROWS: mb.r.w = Ref{Space::CONSTS, add_const(plan, pad_rows(w0(), d.C, p.K, p.KP, true)), 0}; break;
        case Producer::MBMAP_W3F: mb.r.w = Ref{Space::CONSTS, add_const(plan, pack_mbmap_w3f(w0(), d.C, p.K)), 0}; break;
        case Producer::MBMAP_W3P: mb.r.w = Ref{Space::CONSTS, add_const(plan, pack_mbmap_w3p(w0(), d.C, p.K)), 0}; break;
    }
    mb.r.bias = pe.r.bias;
    mb.r.w2 = dw.r.w; mb.r.bias2 = dw.r.bias;
    MbDesc &m = mb.mb;
    m.H = d.H; m.W = d.W; m.Cin = p.K; m.C = d.C; m.OH = d.OH; m.OW = d.OW;
    m.k = d.kw; m.s = d.sw; m.pt = d.pt; m.pl = d.pl;
    m.act1 = p.act; m.p0_1 = p.p0; m.p1_1 = p.p1; m.has_bias1 = p.has_bias;
    m.act2 = d.act; m.p0_2 = d.p0; m.p1_2 = d.p1; m.has_bias2 = d.has_bias;
    m.in_bs = p.in_bs; m.out_bs = d.out_bs;
    m.k1 = p.k1; m.s1 = p.s1; m.pt1 = p.pt1; m.pl1 = p.pl1; m.H1 = p.H1; m.W1 = p.W1; m.Cin1 = p.Cin1;
    const int toh = m.s == 1 ? 8 : 4, tow = m.s == 1 ? 16 : 8;
    m.tiles_x = (m.OW + tow - 1) / tow; m.tiles_y = (m.OH + toh - 1) / toh;
    double halo = (double)((toh - 1) * m.s + m.k) * ((tow - 1) * m.s + m.k) * m.tiles_x * m.tiles_y;  // pixels expanded per sample
    if (p.whole_map) {
        m.whole_map = p.whole_map;
        m.tiles_x = m.tiles_y = 1;  // one squeeze partial per sample
        halo = (double)d.H * d.W;
        if (p.whole_map == 2) {
            m.map_bands = p.shape.bands; m.map_tr = p.shape.tr; m.cin_pad = p.shape.cin_pad;
            m.map_b3 = p.map_b3; m.map_ws = p.map_ws;
            m.tiles_y = p.shape.bands;  // ... per band
            // expand work performed: every band expands the 6 rows it loads (the rows two bands share twice), over the padded k
            if (p.shape.bands > 1) halo = (double)p.shape.bands * 6.0 * (double)(p.shape.tr ? d.H : d.W);
            halo *= (double)p.shape.cin_pad / (double)p.K;
        }
    } else {
        row_streaming(m, halo);
    }
    const double in_elems = p.k1 ? (double)p.H1 * p.W1 * p.Cin1 : (double)d.H * d.W * p.K;
    mb.macs = dw.macs;  // depthwise part (VALU)
    mb.weight_bytes = dw.weight_bytes + pe.weight_bytes;
    mb.bytes = 4.0 * (in_elems + (double)d.OH * d.OW * d.C);
    mb.mfma = false;
    mb.macs_mfma_extra = halo * (double)p.K * d.C;  // first product incl. halo recompute
    mb.macs_recompute = std::max(0.0, mb.macs_mfma_extra - (double)d.H * d.W * (double)p.K * d.C);
    return mb;
}

}  // namespace

bool fuse_mbconv(Plan &plan, const PlanOp &dw, const std::string &node_name, bool only_reader) {
    const DwDesc &d = dw.dw;
    if (!d.tiled || d.kh != d.kw || d.sh != d.sw || sw_is(sw::BN_MBFUSE, "0") || plan.ops.empty() || !only_reader) return false;
    const PlanOp &pe = plan.ops.back();
    Producer p;
    if (!stem_rule(pe, dw, p) && !expand_rule(plan, pe, dw, p)) return false;
    PlanOp mb = fused_op(plan, pe, dw, p, node_name);
    plan.ops.pop_back();
    push_op(plan, std::move(mb));
    return true;
}

}  // namespace bn
