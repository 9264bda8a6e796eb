// Rewrites of the ONNX graph before it is lowered (see plan_build.h): they edit nodes and constants and know nothing of the plan.
// Builder::run calls canonicalize_spectrogram_dialects before its liveness walk and the other two after it.
#include <cmath>

#include "dft_bank.h"
#include "plan_build.h"
#include "plan_rules.h"

namespace bn {
namespace {

// Sole live consumer of tensor `t` (and t is not itself a wanted graph output), else -1.  (Nothing is absorbed yet: lowering has not begun.)
int sole_consumer(const LiveGraph &g, const std::string &t) {
    if (g.wanted.count(t)) return -1;
    auto it = g.consumers.find(t);
    return it != g.consumers.end() && it->second.size() == 1 ? it->second[0] : -1;
}
const std::vector<int> &live_consumers(const LiveGraph &g, const std::string &t) {
    static const std::vector<int> none;
    auto it = g.consumers.find(t);
    return it != g.consumers.end() ? it->second : none;
}

}  // namespace

// ------------------------------------------------------------- one spelling for the real / imaginary part of a spectrogram (round 5)
// Three exporter dialects write "the real part of an STFT" (what BirdNET v2.4 feeds its mel banks):
//   (a) Conv1D with the windowed cosine basis as weights -> Transpose                                  (the form every node-level pass below knows)
//   (b) STFT(signal, step, window) -> Gather(index c, last axis)                                        (torch.stft exports, opset 17)
//   (c) Reshape -> Gather(affine selector) -> Reshape  [tf.signal.frame]  -> Mul(window) -> Unsqueeze -> DFT(onesided) -> Gather(index c)
// (b) and (c) are rewritten into (a) here, before liveness and the passes that prune mel-dead bins, merge the mel product and pick the
// fold, so that all three spellings reach the same plan.  Only the exact patterns are rewritten (every intermediate has ONE consumer and
// is no graph output); anything else keeps its nodes and goes through lower_stft / lower_dft, which map the general case.
void canonicalize_spectrogram_dialects(const OnnxModel &m, std::vector<OnnxNode> &nodes, std::map<std::string, Val> &vals) {
    if (sw_int(sw::BN_CANON_SPECTRO) == 0) return;
    std::map<std::string, int> uses;
    for (auto &nd : nodes)
        for (auto &i : nd.inputs)
            if (!i.empty()) uses[i]++;
    for (auto &o : m.outputs) uses[o.name] += 2;  // a graph output is never an intermediate
    std::map<std::string, int> producer;
    for (size_t k = 0; k < nodes.size(); k++)
        for (auto &o : nodes[k].outputs) producer[o] = (int)k;
    auto cval = [&](const std::string &name) -> const Val * {
        auto it = vals.find(name);
        return it != vals.end() && it->second.is_const ? &it->second : nullptr;
    };
    auto ints = [&](const std::string &name, std::vector<int64_t> &out) {
        const Val *v = cval(name);
        if (!v) return false;
        out = v->is_int ? v->i : std::vector<int64_t>(v->f.begin(), v->f.end());
        return true;
    };
    auto sole_prod = [&](const std::string &t, const char *op) -> int {  // producer of t if it is `op` and t has one use
        auto it = producer.find(t);
        if (it == producer.end() || nodes[it->second].op_type != op || uses[t] != 1) return -1;
        return it->second;
    };
    std::vector<char> dead(nodes.size(), 0);
    std::vector<std::vector<OnnxNode>> repl(nodes.size());
    int serial = 0;
    for (size_t gk = 0; gk < nodes.size(); gk++) {
        const OnnxNode &pick = nodes[gk];
        if (pick.op_type != "Gather" || pick.inputs.size() != 2) continue;
        std::vector<int64_t> ci;
        const Val *civ = cval(pick.inputs[1]);
        if (!civ || civ->numel() != 1 || !civ->dims.empty() || !ints(pick.inputs[1], ci) || (ci[0] != 0 && ci[0] != 1)) continue;
        const int64_t gax = pick.attr_i("axis", 0);
        if (gax != 3 && gax != -1) continue;
        std::string signal;
        std::vector<float> window;
        int64_t N = 0, hop = 0;
        std::vector<int> chain;
        int k1 = sole_prod(pick.inputs[0], "STFT");
        if (k1 >= 0) {                                                      // ---- (b)
            const OnnxNode &st = nodes[k1];
            std::vector<int64_t> stepv, lenv;
            if (st.attr_i("onesided", 1) == 0 || st.inputs.size() < 2 || !ints(st.inputs[1], stepv) || stepv.size() != 1) continue;
            const Val *w = st.inputs.size() > 2 && !st.inputs[2].empty() ? cval(st.inputs[2]) : nullptr;
            if (st.inputs.size() > 2 && !st.inputs[2].empty() && (!w || w->is_int)) continue;
            if (st.inputs.size() > 3 && !st.inputs[3].empty()) { if (!ints(st.inputs[3], lenv) || lenv.size() != 1) continue; N = lenv[0]; }
            else if (w) N = w->numel();
            if (N < 2 || (w && w->numel() != N)) continue;
            if (w) window = w->f;
            hop = stepv[0];
            signal = st.inputs[0];
            chain = {k1};
        } else if ((k1 = sole_prod(pick.inputs[0], "DFT")) >= 0) {            // ---- (c)
            const OnnxNode &df = nodes[k1];
            if (df.attr_i("onesided", 0) == 0 || df.attr_i("inverse", 0) != 0 || df.inputs.size() != 1) continue;
            const int64_t dax = df.has("axis") ? df.attr_i("axis", 1) : (m.opset >= 20 ? -2 : 1);
            if (dax != 2 && dax != -2) continue;
            const int ku = sole_prod(df.inputs[0], "Unsqueeze");
            if (ku < 0) continue;
            std::vector<int64_t> ax = nodes[ku].attr_ints("axes");
            if (ax.empty() && (nodes[ku].inputs.size() < 2 || !ints(nodes[ku].inputs[1], ax))) continue;
            if (ax.size() != 1 || (ax[0] != 3 && ax[0] != -1)) continue;
            std::string fr = nodes[ku].inputs[0];
            chain = {k1, ku};
            const int km = sole_prod(fr, "Mul");
            if (km >= 0) {
                const OnnxNode &mu = nodes[km];
                const Val *w0 = cval(mu.inputs[0]), *w1 = cval(mu.inputs[1]);
                const Val *w = w0 ? w0 : w1;
                if (!w || (w0 && w1) || w->is_int) continue;
                int nu = 0;
                for (auto d : w->dims) nu += d != 1;
                if (nu != 1 || w->dims.empty() || w->dims.back() != w->numel()) continue;  // along the frames' last axis
                window = w->f;
                fr = mu.inputs[w0 ? 1 : 0];
                chain.push_back(km);
            }
            // tf.signal.frame: Reshape [0|-1, S / sub, sub] -> Gather(axis 1, selector[f][j] = f * h + j) -> Reshape [0|-1, F, L]
            const int kr2 = sole_prod(fr, "Reshape");
            if (kr2 < 0) continue;
            std::vector<int64_t> shp2, shp0;
            if (!ints(nodes[kr2].inputs[1], shp2) || shp2.size() != 3) continue;
            const int kg = sole_prod(nodes[kr2].inputs[0], "Gather");
            if (kg < 0 || nodes[kg].attr_i("axis", 0) != 1) continue;
            const Val *sel = cval(nodes[kg].inputs[1]);
            if (!sel || !sel->is_int || sel->dims.size() != 2) continue;
            const int kr0 = sole_prod(nodes[kg].inputs[0], "Reshape");
            if (kr0 < 0 || !ints(nodes[kr0].inputs[1], shp0) || shp0.size() != 3) continue;
            const int64_t F = sel->dims[0], J = sel->dims[1], sub = shp0[2];
            if (sub < 1 || F < 1 || J < 1 || shp2[1] != F || shp2[2] != J * sub) continue;
            const int64_t h = F > 1 ? sel->i[(size_t)J] - sel->i[0] : 1;
            bool affine = sel->i[0] == 0 && h >= 1;
            for (int64_t f = 0; f < F && affine; f++)
                for (int64_t j = 0; j < J && affine; j++) affine = sel->i[(size_t)(f * J + j)] == f * h + j;
            // (the Conv frames the WHOLE signal: the selector must take every frame that fits)
            if (!affine || shp0[1] < (F - 1) * h + J || F != (shp0[1] - J) / h + 1) continue;
            N = J * sub;
            hop = h * sub;
            if (!window.empty() && (int64_t)window.size() != N) continue;
            signal = nodes[kr0].inputs[0];
            chain.insert(chain.end(), {kr2, kg, kr0});
        } else continue;
        if (hop < 1 || N > 8192) continue;
        const int64_t bins = N / 2 + 1;
        Val basis;
        basis.is_const = true;
        basis.dims = {bins, 1, N};
        basis.f.resize((size_t)(bins * N));
        for (int64_t k = 0; k < bins; k++)
            for (int64_t t = 0; t < N; t++) {
                const double wv = window.empty() ? 1.0 : (double)window[(size_t)t];
                const double th = 2.0 * M_PI * (double)((k * t) % N) / (double)N;
                basis.f[(size_t)(k * N + t)] = (float)(ci[0] == 0 ? wv * std::cos(th) : -wv * std::sin(th));
            }
        const std::string base = "spectro" + std::to_string(serial++) + ":" + pick.outputs[0];
        vals[base + "/basis"] = std::move(basis);
        vals[base + "/shape"] = make_const_i({3}, {0, 1, -1});
        OnnxNode rs = synth_node("Reshape", base + "/signal", {signal, base + "/shape"}, base + "/signal");
        OnnxNode conv = synth_node("Conv", (pick.name.empty() ? pick.outputs[0] : pick.name) + (ci[0] == 0 ? "~re" : "~im"), {base + "/signal", base + "/basis"}, base + "/bank");
        set_ints(conv, "strides", {hop});
        set_ints(conv, "kernel_shape", {N});
        OnnxNode tr = synth_node("Transpose", base + "/t", {base + "/bank"}, pick.outputs[0]);
        set_ints(tr, "perm", {0, 2, 1});
        repl[gk] = {rs, conv, tr};
        dead[gk] = 1;
        for (int c : chain) dead[(size_t)c] = 1;
    }
    if (!serial) return;
    std::vector<OnnxNode> out;
    for (size_t k = 0; k < nodes.size(); k++) {
        for (auto &r : repl[k]) out.push_back(r);
        if (!dead[k]) out.push_back(nodes[k]);
    }
    nodes = std::move(out);
}

// ------------------------------------------------------------- pruning
// Conv(out channels c) -> [Transpose] -> MatMul(const W[c, :]): output channels whose W row is
// all zero never influence the result, drop them (mel filterbanks cover a fraction of the bins).
void prune_zero_rows(const LiveGraph &g) {
    for (size_t k = 0; k < g.nodes.size(); k++) {
        if (!g.live[k] || g.nodes[k].op_type != "Conv") continue;
        OnnxNode &conv = g.nodes[k];
        int c1 = sole_consumer(g, conv.outputs[0]);
        if (c1 < 0) continue;
        int mm = -1;
        if (g.nodes[c1].op_type == "Transpose") {
            auto perm = g.nodes[c1].attr_ints("perm");
            if (perm != std::vector<int64_t>{0, 2, 1}) continue;
            mm = sole_consumer(g, g.nodes[c1].outputs[0]);
        } else continue;
        if (mm < 0 || g.nodes[mm].op_type != "MatMul") continue;
        auto wi = g.vals.find(g.nodes[mm].inputs[1]);
        auto cw = g.vals.find(conv.inputs[1]);
        if (wi == g.vals.end() || cw == g.vals.end() || !wi->second.is_const || !cw->second.is_const) continue;
        Val &W = wi->second;
        Val &CW = cw->second;
        if (W.dims.size() != 2 || CW.dims.empty() || W.dims[0] != CW.dims[0] || W.is_int) continue;
        // weights must not be shared with other nodes
        if (live_consumers(g, g.nodes[mm].inputs[1]).size() != 1 || live_consumers(g, conv.inputs[1]).size() != 1) continue;
        int64_t C = W.dims[0], N = W.dims[1];
        std::vector<int64_t> keep;
        for (int64_t c = 0; c < C; c++) {
            bool nz = false;
            for (int64_t j = 0; j < N && !nz; j++) nz = W.f[c * N + j] != 0.0f;
            if (nz) keep.push_back(c);
        }
        if ((int64_t)keep.size() == C || keep.empty()) continue;
        // keep a multiple of 4 channels (a few dead neighbours stay): the consumer GEMM's K is then a whole number
        // of float4 loads for both operands instead of scalar loads (K = 309 -> 312, 127 -> 128)
        {
            std::vector<char> kept((size_t)C, 0);
            for (int64_t c : keep) kept[(size_t)c] = 1;
            for (int64_t c = keep.back() + 1; c < C && keep.size() % 4; c++) { kept[(size_t)c] = 1; keep.push_back(c); }
            for (int64_t c = keep.front() - 1; c >= 0 && keep.size() % 4; c--) { kept[(size_t)c] = 1; keep.push_back(c); }
            std::sort(keep.begin(), keep.end());
            if ((int64_t)keep.size() == C) continue;
        }
        int64_t per = CW.numel() / C;
        std::vector<float> nw(keep.size() * per), nW(keep.size() * N);
        for (size_t r = 0; r < keep.size(); r++) {
            std::copy(CW.f.begin() + keep[r] * per, CW.f.begin() + (keep[r] + 1) * per, nw.begin() + r * per);
            std::copy(W.f.begin() + keep[r] * N, W.f.begin() + (keep[r] + 1) * N, nW.begin() + r * N);
        }
        CW.f = nw; CW.dims[0] = (int64_t)keep.size();
        W.f = nW; W.dims[0] = (int64_t)keep.size();
        if (conv.inputs.size() > 2 && !conv.inputs[2].empty()) {
            auto bi = g.vals.find(conv.inputs[2]);
            if (bi != g.vals.end() && bi->second.is_const && live_consumers(g, conv.inputs[2]).size() == 1) {
                std::vector<float> nb(keep.size());
                for (size_t r = 0; r < keep.size(); r++) nb[r] = bi->second.f[keep[r]];
                bi->second.f = nb; bi->second.dims[0] = (int64_t)keep.size();
            }
        }
    }
}

// ------------------------------------------------------------- framing conv x constant product -> one framing conv (round 4)
// Conv1D(one input channel, C filters of length L) -> Transpose -> MatMul(const W[C, N]) is ONE linear map of the frame when nothing
// sits between the two (v2.4 takes the REAL PART of its STFT straight into the mel bank): N filters  sum_c W[c][n] w_c  of length L,
// bias  sum_c W[c][n] b_c.  Worth it when N filters cost less than the C filters (as an FFT or as folded matrix products) plus the
// product: v2.4's 312 mel-live bins of the 1024-point branch -> 96 mel filters of 512 folded taps (the rows stay symmetric about the
// frame centre), against an FFT of every frame plus the mel phase; NOT its 127 bins of the 2048-point branch, which the quarter fold
// evaluates in 512 taps each where 96 merged filters would need 1024.  Costs in f32-MFMA SIMD-cycles per frame, the scale emit_stft
// calibrated.  The filters are summed in double and rounded once.  BN_CONVMERGE=0 disables, =1 merges wherever the pattern matches.
void merge_framing_products(const LiveGraph &g) {
    const int mode = sw_int(sw::BN_CONVMERGE);
    if (mode == 0) return;
    if (sw_is(sw::BN_STFT, "1") && mode != 1) return;  // every recognised bank as an FFT: the banks stay banks
    for (size_t k = 0; k < g.nodes.size(); k++) {
        if (!g.live[k] || g.nodes[k].op_type != "Conv") continue;
        OnnxNode &conv = g.nodes[k];
        const int c1 = sole_consumer(g, conv.outputs[0]);
        if (c1 < 0 || g.nodes[c1].op_type != "Transpose" || g.nodes[c1].attr_ints("perm") != std::vector<int64_t>{0, 2, 1}) continue;
        const int mm = sole_consumer(g, g.nodes[c1].outputs[0]);
        if (mm < 0 || g.nodes[mm].op_type != "MatMul" || g.nodes[mm].inputs[0] != g.nodes[c1].outputs[0]) continue;
        auto wi = g.vals.find(g.nodes[mm].inputs[1]);
        auto cw = g.vals.find(conv.inputs[1]);
        if (wi == g.vals.end() || cw == g.vals.end() || !wi->second.is_const || !cw->second.is_const || wi->second.is_int || cw->second.is_int) continue;
        Val &W = wi->second;
        Val &CW = cw->second;
        if (W.dims.size() != 2 || CW.dims.size() != 3 || CW.dims[1] != 1 || W.dims[0] != CW.dims[0]) continue;  // [C, 1, L] x [C, N]
        if (live_consumers(g, g.nodes[mm].inputs[1]).size() != 1 || live_consumers(g, conv.inputs[1]).size() != 1) continue;
        if (conv.attr_i("group", 1) != 1) continue;
        const int64_t C = CW.dims[0], L = CW.dims[2], N = W.dims[1];
        if (L < 128 || N >= C) continue;
        Val *bias = nullptr;
        if (conv.inputs.size() > 2 && !conv.inputs[2].empty()) {
            auto bi = g.vals.find(conv.inputs[2]);
            if (bi == g.vals.end() || !bi->second.is_const || bi->second.is_int || live_consumers(g, conv.inputs[2]).size() != 1) continue;
            bias = &bi->second;
        }
        // symmetry of the rows about the frame centre (the fold rule's test, its tolerance)
        float maxabs = 0.0f;
        for (float v : CW.f) maxabs = std::max(maxabs, std::fabs(v));
        const float eps = 1.1920929e-7f * maxabs;
        bool all_sym = L % 64 == 0, all_folded = L % 64 == 0;
        for (int64_t c = 0; c < C && all_folded; c++) {
            const float *w = &CW.f[(size_t)(c * L)];
            bool sym = std::fabs(w[0]) <= eps, anti = sym && std::fabs(w[L / 2]) <= eps;
            for (int64_t t = 1; t < L / 2 && (sym || anti); t++) {
                if (!(std::fabs(w[t] - w[L - t]) <= eps)) sym = false;
                if (!(std::fabs(w[t] + w[L - t]) <= eps)) anti = false;
            }
            all_sym = all_sym && sym;
            all_folded = all_folded && (sym || anti);
        }
        // separate: the cheapest form the bank may take + the product; merged: N filters, folded if every row is symmetric
        const bool fft_size = L <= 2048 && ((L & (L - 1)) == 0 || fft_five_pow2(L));
        double bank = (double)C * (double)(all_folded ? L / 2 : L) / 32.0;
        bool product_inside = false;
        if (all_sym && L % 128 == 0 && C <= 160) bank = std::min(bank, (double)C * (double)(L / 4 + 1) / 32.0);  // quarter fold
        if (all_folded && fft_size && !sw_is(sw::BN_STFT, "0")) {
            const double fft = 0.18 * (double)L * std::log2((double)L);  // (with its mel phase: emit_stft's calibration)
            if (fft < bank) { bank = fft; product_inside = true; }
        }
        const double separate = bank + (product_inside ? 0.0 : (double)C * (double)N / 32.0);
        const double merged = (double)N * (double)(all_sym ? L / 2 : L) / 32.0;
        if (mode != 1 && !(merged < 0.9 * separate)) continue;
        std::vector<float> nw((size_t)(N * L));
        std::vector<double> acc((size_t)L);
        for (int64_t n2 = 0; n2 < N; n2++) {
            std::fill(acc.begin(), acc.end(), 0.0);
            for (int64_t c = 0; c < C; c++) {
                const double m = (double)W.f[(size_t)(c * N + n2)];
                if (m == 0.0) continue;
                const float *w = &CW.f[(size_t)(c * L)];
                for (int64_t t = 0; t < L; t++) acc[(size_t)t] += m * (double)w[t];
            }
            for (int64_t t = 0; t < L; t++) nw[(size_t)(n2 * L + t)] = (float)acc[(size_t)t];
            if (all_sym) {  // exactly symmetric again after the rounding (the fold keeps the first half)
                nw[(size_t)(n2 * L)] = 0.0f;
                for (int64_t t = 1; t < L / 2; t++) nw[(size_t)(n2 * L + L - t)] = nw[(size_t)(n2 * L + t)];
            }
        }
        if (bias) {
            std::vector<float> nb((size_t)N);
            for (int64_t n2 = 0; n2 < N; n2++) {
                double a = 0.0;
                for (int64_t c = 0; c < C; c++) a += (double)W.f[(size_t)(c * N + n2)] * (double)bias->f[(size_t)c];
                nb[(size_t)n2] = (float)a;
            }
            bias->f = nb;
            bias->dims[0] = N;
        }
        CW.f = nw;
        CW.dims[0] = N;
        // the product is gone: its node hands the transposed conv result on
        OnnxNode &prod = g.nodes[mm];
        prod.op_type = "Identity";
        prod.inputs.resize(1);
    }
}

}  // namespace bn
