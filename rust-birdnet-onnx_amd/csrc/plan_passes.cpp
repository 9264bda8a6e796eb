// Passes over the lowered plan: launches fused into their neighbours, weights repacked, then the memory plan.  They read and write the
// Plan alone (see plan_build.h); run_plan_passes at the end of this file is their one fixed order.
#include <algorithm>
#include <cmath>

#include "plan_build.h"
#include "plan_rules.h"

namespace bn {
namespace {

// --------------------------------------------------------- elementwise chain fusion
void recompute_liveness(Plan &plan) {
    for (auto &st : plan.storages) { st.first = -1; st.last = -1; }
    for (size_t k = 0; k < plan.ops.size(); k++) for_each_ref(plan.ops[k].r, [&](const Ref &r) { touch(plan, r, (int)k); });
}
// per arena storage: the launches that name it in any operand, ascending
std::vector<std::vector<int>> arena_users(const Plan &plan) {
    std::vector<std::vector<int>> users(plan.storages.size());
    for (size_t k = 0; k < plan.ops.size(); k++)
        for_each_ref(plan.ops[k].r, [&](const Ref &r) {
            if (r.space == Space::ARENA && (users[r.id].empty() || users[r.id].back() != (int)k)) users[r.id].push_back((int)k);
        });
    return users;
}
// how many operands of `op` name `space`:`id`
int refs_to(const PlanOp &op, Space space, int id) {
    int n = 0;
    for_each_ref(op.r, [&](const Ref &r) { n += r.space == space && r.id == id; });
    return n;
}
// An ELT launch whose result is read by exactly one later ELT launch, as that launch's primary
// operand over the very same index space, is folded into it (its stages are prepended).
void fuse_elementwise_chains(Plan &plan) {
    bool changed = true;
    while (changed) {
        changed = false;
        recompute_liveness(plan);
        const auto users = arena_users(plan);
        for (size_t j = 0; j < plan.ops.size() && !changed; j++) {
            PlanOp &cons = plan.ops[j];
            if (cons.kind != OpKind::ELT || cons.r.a.space != Space::ARENA) continue;
            const auto &u = users[cons.r.a.id];
            if (u.size() != 2 || u[1] != (int)j || plan.storages[cons.r.a.id].pinned) continue;
            PlanOp &prod = plan.ops[u[0]];
            if (prod.kind != OpKind::ELT || prod.r.out.space != Space::ARENA || prod.r.out.id != cons.r.a.id) continue;
            const int64_t delta = cons.r.a.offset - prod.r.out.offset;  // consumer may read a shifted / reversed view
            if (prod.elt.nstages + cons.elt.nstages > ELT_MAX_STAGES) continue;
            // (A) same index space: the consumer reads exactly what the producer wrote, or
            // (B) the producer is a flat map over a dense buffer (offset in == offset out), so the
            //     consumer's own strides address the producer's operands directly
            const EltDesc &pe = prod.elt, &ce = cons.elt;
            if (pe.bo != ce.ba) continue;
            bool same = pe.nd == ce.nd && delta == 0;
            for (int k = 0; same && k < pe.nd; k++) same = pe.size[k] == ce.size[k] && (pe.size[k] == 1 || pe.so[k] == ce.sa[k]);
            bool flat_prod = pe.nd == 1 && pe.so[0] == 1 && pe.sa[0] == 1 && pe.per_sample == ce.per_sample;
            for (int k = 0; flat_prod && k < pe.nstages; k++)
                flat_prod = pe.st[k].bin == BIN_NONE || pe.st[k].sb[0] == 0 || pe.st[k].sb[0] == 1;
            // (C) the consumer is a flat map over the dense intermediate: it adopts the producer's index
            //     space (its own strides scale by the producer's row-major runs)
            bool flat_cons = !same && !flat_prod && ce.nd == 1 && ce.sa[0] == 1 && delta == 0 && pe.per_sample == ce.per_sample;
            int64_t runs[ELT_MAX_DIMS] = {0};
            if (flat_cons) {
                int64_t run = 1;
                for (int k = pe.nd - 1; k >= 0; k--) {
                    if (pe.size[k] != 1 && pe.so[k] != run) flat_cons = false;
                    runs[k] = run;
                    run *= pe.size[k];
                }
            }
            if (!same && !flat_prod && !flat_cons) continue;
            // the consumer must not also use the intermediate as a stage operand
            {
                bool clash = false;
                for (int k = 0; k < ce.nstages; k++) clash = clash || (cons.r.chain[k].space == Space::ARENA && cons.r.chain[k].id == cons.r.a.id);
                if (clash) continue;
            }
            // nothing between the two may overwrite the producer's inputs: storages are single-assignment
            // except concat targets, which are only read after all their writers ran -> safe.
            PlanOp fused = cons;
            fused.name = prod.name + "+" + cons.name;
            fused.r.a = prod.r.a;
            EltDesc &fe = fused.elt;
            fe.ba = pe.ba;
            fe.nstages = pe.nstages + ce.nstages;
            if (same) {
                for (int k = 0; k < pe.nd; k++) fe.sa[k] = pe.sa[k];
                for (int k = 0; k < pe.nstages; k++) { fe.st[k] = pe.st[k]; fused.r.chain[k] = prod.r.chain[k]; }
            } else if (flat_cons) {
                fe.nd = pe.nd;
                for (int k = 0; k < pe.nd; k++) { fe.size[k] = pe.size[k]; fe.sa[k] = pe.sa[k]; fe.so[k] = ce.so[0] * runs[k]; }
                for (int k = 0; k < pe.nstages; k++) { fe.st[k] = pe.st[k]; fused.r.chain[k] = prod.r.chain[k]; }
            } else {
                // flat producer: its primary operand and every full-size stage operand are addressed
                // with the strides the consumer used for the intermediate (fe.sa is already ce.sa)
                fused.r.a.offset += delta;
                for (int k = 0; k < pe.nstages; k++) {
                    fe.st[k] = pe.st[k];
                    fused.r.chain[k] = prod.r.chain[k];
                    const bool full = pe.st[k].bin != BIN_NONE && pe.st[k].sb[0] == 1;
                    if (full) fused.r.chain[k].offset += delta;
                    for (int q = 0; q < ELT_MAX_DIMS; q++) fe.st[k].sb[q] = (q < ce.nd && full) ? ce.sa[q] : 0;
                }
            }
            for (int k = 0; k < ce.nstages; k++) {
                fe.st[pe.nstages + k] = ce.st[k];
                fused.r.chain[pe.nstages + k] = cons.r.chain[k];
                if (flat_cons)
                    for (int q = 0; q < ELT_MAX_DIMS; q++) fe.st[pe.nstages + k].sb[q] = q < pe.nd ? ce.st[k].sb[0] * runs[q] : 0;
            }
            fused.bytes = prod.bytes + cons.bytes - 8.0 * (double)pe.per_sample;  // the intermediate never touches memory
            plan.ops[j] = fused;
            plan.ops.erase(plan.ops.begin() + u[0]);
            changed = true;
        }
        // (D) a stage operand that is the square x*x of some view, produced only for this stage, is
        //     read straight from x and squared in the consumer (|z|^2 = re*re + im*im in one launch)
        for (size_t j = 0; j < plan.ops.size() && !changed; j++) {
            PlanOp &cons = plan.ops[j];
            if (cons.kind != OpKind::ELT) continue;
            EltDesc &ce = cons.elt;
            for (int k = 0; k < ce.nstages && !changed; k++) {
                EltStage &cs = ce.st[k];
                const Ref &br = cons.r.chain[k];
                if (cs.bin == BIN_NONE || cs.bsq || br.space != Space::ARENA || plan.storages[br.id].pinned) continue;
                const auto &u = users[br.id];
                if (u.size() != 2 || u[1] != (int)j) continue;
                const PlanOp &prod = plan.ops[u[0]];
                const EltDesc &pe = prod.elt;
                if (prod.kind != OpKind::ELT || prod.r.out.space != Space::ARENA || prod.r.out.id != br.id || prod.r.out.offset != br.offset) continue;
                if (pe.nstages != 1 || pe.st[0].bin != BIN_MUL || pe.st[0].act != ACT_NONE || pe.st[0].bsq) continue;
                if (prod.r.chain[0].space != prod.r.a.space || prod.r.chain[0].id != prod.r.a.id || prod.r.chain[0].offset != prod.r.a.offset || pe.st[0].bb != pe.ba) continue;
                if (cons.r.a.space == Space::ARENA && cons.r.a.id == br.id) continue;
                bool match = pe.nd == ce.nd && pe.bo == cs.bb;
                for (int q = 0; match && q < pe.nd; q++)
                    match = pe.size[q] == ce.size[q] && pe.so[q] == cs.sb[q] && pe.st[0].sb[q] == pe.sa[q];
                if (!match) continue;
                cons.r.chain[k] = prod.r.a;
                for (int q = 0; q < ELT_MAX_DIMS; q++) cs.sb[q] = q < pe.nd ? pe.sa[q] : 0;
                cs.bb = pe.ba;
                cs.bsq = 1;
                cons.name += "+sq(" + prod.name + ")";
                cons.bytes += prod.bytes - 12.0 * (double)pe.per_sample + 4.0 * (double)pe.per_sample;
                plan.ops.erase(plan.ops.begin() + u[0]);
                changed = true;
            }
        }
    }
}

// (I) The two small squeeze-excite products move into the prologue of the GEMM that consumes their gate, when that GEMM
// runs on the LDS-DMA kernel (gemm_dma.hip): every block of a sample recomputes the gate from the squeeze partial sums
// while its first K steps are in flight.  One launch less per MBConv block -- 7 - 8 us of the serial chain of a step,
// of which 3.6 us are the launch itself -- for C x Cr x 8 bytes of L2 reads per block; only up to BN_SEGEMM_MAXC
// channels (default 768: at C = 1152 the 442 KB of excite weights per block cost more than the launch they save).
// MEASURED (batch 32, v2.4): slower.  A block has 2 - 8 waves for two products the stand-alone excite kernel spreads
// over 80 per sample; the prologue is a chain of load latencies (K = 672: project conv 20 -> 52 us against 20 + 8 for
// the two launches), four contexts 52.7 k -> 47.2 k segments/s.  Opt-in (BN_SEGEMM=1), kept under test.
void absorb_se_into_gemms(Plan &plan) {
    if (!(sw_int(sw::BN_SEGEMM) == 1)) return;
    const int max_c = gemm_dma_se_max_channels();
    for (size_t j = 0; j < plan.ops.size(); j++) {
        if (plan.ops[j].kind != OpKind::SEFC || plan.ops[j].r.out.space != Space::ARENA) continue;
        const int gate_id = plan.ops[j].r.out.id;
        if (plan.storages[gate_id].pinned) continue;
        int cons = -1, users = 0;
        for (size_t k = 0; k < plan.ops.size(); k++)
            if (k != j && refs_to(plan.ops[k], Space::ARENA, gate_id)) { users++; cons = (int)k; }
        if (users != 1 || cons < (int)j) continue;
        PlanOp &g = plan.ops[cons];
        const PlanOp &se = plan.ops[j];
        if (g.kind != OpKind::GEMM || !g.gemm.has_scale || g.r.gate.space != Space::ARENA || g.r.gate.id != gate_id || g.r.gate.offset != 0 || g.se_fused) continue;
        if (se.se.C != g.gemm.K || se.se.C > max_c || se.se.C % 4 || !gemm_dma_shape(g.gemm)) continue;
        g.se_fused = 1;
        g.se = se.se;
        g.gemm.se_inline = 1;
        g.r.se.partial = se.r.a;  // squeeze partial sums
        g.r.se.w1 = se.r.w;       // W1 [Cr][C]
        g.r.se.b1 = se.r.bias;
        g.r.se.w2t = se.r.w2;     // W2 transposed [Cr][C]
        g.r.se.b2 = se.r.bias2;
        g.name = se.name + "+" + g.name;
        g.macs_valu_extra += se.macs;
        g.weight_bytes += se.weight_bytes;
        g.bytes += se.bytes;
        plan.ops.erase(plan.ops.begin() + (long)j);
        j--;
    }
}

// (G) Neighbours of an STFT launch move into it:
//  * the mel filter bank -- a GEMM over the spectrum rows with a SPARSE constant matrix (triangular filters: a few
//    bins per band) -- together with whatever rule E put into that GEMM's epilogue (compression chain, layout copy
//    into the spectrogram image): the spectrum rows never leave LDS.  BN_STFT_MEL=0 disables.
//  * the elementwise chain that produced the signal, when every stage operand is one number per sample (the
//    min-max normalisation of the v2.4 graph) and every reader of its result is an STFT launch: the chain runs
//    while the span is loaded, the normalised segment is never written.  BN_STFT_PRE=0 disables.
void absorb_into_stft(Plan &plan) {
    const bool mel_on = !sw_is(sw::BN_STFT_MEL, "0");
    const bool pre_on = sw_on(sw::BN_STFT_PRE);
    //  * (round 3) the power / magnitude pass behind a cos | sin bank: an elementwise launch  re*re + im*im [-> sqrt]  over
    //    the two halves of every spectrum row, whose only reader it is -- the launch computes both linear forms of a bin
    //    in one lane and stores f(u^2 + v^2): half the spectrum bytes written, none read back, one launch less, and the
    //    mel bank that follows becomes a direct neighbour (next rule).  BN_STFT_POWER=0 disables.
    if (sw_on(sw::BN_STFT_POWER)) {
        bool again = true;
        while (again) {
            again = false;
            const auto users = arena_users(plan);
            for (size_t i = 0; i < plan.ops.size() && !again; i++) {
                PlanOp &f = plan.ops[i];
                FftDesc &d = f.fft;
                if (f.kind != OpKind::FFT || d.nmel || d.power || d.has_bias || d.npost || f.r.out.space != Space::ARENA || plan.storages[f.r.out.id].pinned) continue;
                if (d.nout % 2 || d.ldc != d.nout || d.out_rs != d.nout || d.out_cs != 1) continue;
                const auto &u = users[f.r.out.id];
                if (u.size() != 2 || u[0] != (int)i) continue;
                PlanOp &el = plan.ops[u[1]];
                const EltDesc &e = el.elt;
                const int64_t nb = d.nout / 2;
                if (el.kind != OpKind::ELT || e.nd != 2 || e.size[0] != d.frames || e.size[1] != nb || e.sa[0] != d.nout || e.sa[1] != 1 || e.ba != d.c_bs) continue;
                if (el.r.a.space != Space::ARENA || el.r.a.id != f.r.out.id || el.r.a.offset != f.r.out.offset) continue;
                if (el.r.out.space != Space::ARENA || e.so[1] != 1 || e.so[0] < nb) continue;
                // stage 0: x * x (the operand is the same view); stage 1: + y^2 with y the other half of the row; [stage 2: sqrt]
                if (e.nstages < 2 || e.nstages > 3) continue;
                const EltStage &s0 = e.st[0], &s1 = e.st[1];
                const Ref &r0 = el.r.chain[0], &r1 = el.r.chain[1];
                if (s0.bin != BIN_MUL || s0.bsq || s0.act != ACT_NONE || r0.space != Space::ARENA || r0.id != f.r.out.id || r0.offset != f.r.out.offset ||
                    s0.sb[0] != d.nout || s0.sb[1] != 1 || s0.bb != d.c_bs)
                    continue;
                if (s1.bin != BIN_ADD || !s1.bsq || s1.act != ACT_NONE || r1.space != Space::ARENA || r1.id != f.r.out.id || r1.offset != f.r.out.offset + nb ||
                    s1.sb[0] != d.nout || s1.sb[1] != 1 || s1.bb != d.c_bs)
                    continue;
                if (e.nstages == 3 && !(e.st[2].bin == BIN_NONE && e.st[2].act == ACT_SQRT)) continue;
                // the two halves must be the two forms of the SAME bins in the same order (same buffer positions)
                const std::vector<float> &ot = plan.consts[f.r.fft.otab.id];
                bool same = (int64_t)ot.size() >= f.r.fft.otab.offset + d.nout * 8;
                for (int64_t c = 0; c < nb && same; c++) {
                    const float *u0 = &ot[(size_t)(f.r.fft.otab.offset + c * 8)], *v0 = &ot[(size_t)(f.r.fft.otab.offset + (c + nb) * 8)];
                    same = u0[0] == v0[0] && u0[1] == v0[1];
                }
                if (!same) continue;
                std::vector<float> ot2((size_t)nb * 12, 0.0f);
                for (int64_t c = 0; c < nb; c++) {
                    const float *u0 = &ot[(size_t)(f.r.fft.otab.offset + c * 8)], *v0 = &ot[(size_t)(f.r.fft.otab.offset + (c + nb) * 8)];
                    float *o = &ot2[(size_t)c * 12];
                    for (int q = 0; q < 6; q++) o[q] = u0[q];
                    for (int q = 0; q < 4; q++) o[8 + q] = v0[2 + q];
                }
                FftDesc probe = d;
                probe.nout = (int32_t)nb; probe.otab_stride = 12; probe.power = e.nstages == 3 ? 2 : 1;
                if (stft_lds_bytes(probe, 8) > 156 * 1024) continue;
                d = probe;
                d.ldc = e.so[0]; d.out_rs = e.so[0]; d.out_cs = 1; d.c_bs = e.bo;
                f.r.fft.otab = Ref{Space::CONSTS, add_const(plan, ot2), 0};
                f.r.out = el.r.out;
                f.name += "+" + el.name;
                f.weight_bytes += 4.0 * (double)ot2.size() - 4.0 * 8.0 * (double)(2 * nb);
                f.bytes -= 4.0 * (double)d.frames * (double)nb;  // one value per bin is written instead of two; the cos | sin rows are never read back
                f.macs += 2.0 * (double)d.frames * (double)nb;
                f.flops_fft += 3.0 * (double)d.frames * (double)nb;
                plan.ops.erase(plan.ops.begin() + u[1]);
                again = true;
            }
        }
    }
    bool changed = mel_on;
    while (changed) {
        changed = false;
        const auto users = arena_users(plan);
        for (size_t i = 0; i < plan.ops.size() && !changed; i++) {
            PlanOp &f = plan.ops[i];
            if (f.kind != OpKind::FFT || f.fft.nmel || f.r.out.space != Space::ARENA || plan.storages[f.r.out.id].pinned) continue;
            if (f.fft.tpb & (f.fft.tpb - 1)) continue;  // the mel phases index a tile's frames by shifts / 16-frame matrix tiles (M = 5 q banks: tiles of 24)
            const auto &u = users[f.r.out.id];
            if (u.size() != 2 || u[0] != (int)i) continue;
            PlanOp &g = plan.ops[u[1]];
            const GemmDesc &gd = g.gemm;
            if (g.kind != OpKind::GEMM || g.r.a.space != Space::ARENA || g.r.a.id != f.r.out.id || g.r.a.offset != f.r.out.offset) continue;
            if (gd.fold || gd.has_scale || gd.has_res || gd.rows != f.fft.frames || gd.K != f.fft.nout || gd.lda != gd.K || gd.a_bs != f.fft.c_bs ||
                f.fft.ldc != f.fft.nout || g.r.w.space != Space::CONSTS)
                continue;
            bool stages_ok = stft_act_supported(gd.act);
            for (int q = 0; q < gd.npost; q++) stages_ok = stages_ok && stft_act_supported(gd.post_act[q]);
            if (!stages_ok) continue;
            const std::vector<float> &W = plan.consts[g.r.w.id];  // [N][K]
            const int64_t N = gd.N, K = gd.K;
            std::vector<float> mstart, ment;  // row starts; (column, value) pairs
            for (int64_t nn = 0; nn < N; nn++) {
                mstart.push_back((float)(ment.size() / 2));
                for (int64_t k = 0; k < K; k++) {
                    const float v = W[(size_t)(g.r.w.offset + nn * K + k)];
                    if (v != 0.0f) { ment.push_back((float)k); ment.push_back(v); }
                }
            }
            mstart.push_back((float)(ment.size() / 2));
            const size_t nnz_count = ment.size() / 2;
            if ((double)nnz_count > 0.3 * (double)N * (double)K || nnz_count >= (1u << 23) || N > 1024) continue;  // dense: stays a GEMM
            FftDesc probe = f.fft;
            probe.nmel = (int32_t)N;
            probe.mel_nnz = (int32_t)nnz_count;
            // the tile's spectrum rows join the LDS image.  Where 16 frames per tile no longer fit (v3.0: 513 bins, 128 bands)
            // tiles of 8 would, but the launch then loses to FFT + dense mel GEMM (200 us against 97 + 66 at batch 64,
            // 41.5 k against 44.0 k segments/s): BN_STFT_MEL=force takes the smaller tile anyway (tests)
            if (sw_is(sw::BN_STFT_MEL, "force"))
                while (stft_lds_bytes(probe, 8) > 156 * 1024 && probe.tpb > 8 && (probe.tpb / 2) % probe.F == 0) probe.tpb /= 2;
            if (stft_lds_bytes(probe, 8) > 156 * 1024) continue;
            FftDesc &d = f.fft;
            d.tpb = probe.tpb;
            d.nmel = (int32_t)N;
            d.mel_nnz = (int32_t)nnz_count;
            d.mel_mode = 0; d.mel_groups = 0; d.spec_stride = d.nout;
            // the bank as 16 x 16 tiles for the matrix cores (kernels.h, FftDesc::mel_mode): tile rows of 16 bands, of each
            // only the 16-bin groups that hold a non-zero; a tile is stored in the lane order of the A fragment (lane (i, q)
            // holds band i, bins 16 g + 4 q + 0..3).  BN_STFT_MELMFMA=0 keeps the (column, weight) lists on the vector ALU.
            if (sw_on(sw::BN_STFT_MELMFMA) && d.tpb == 16) {
                const int64_t ntile = (N + 15) / 16, ngrp = (K + 15) / 16;
                std::vector<float> tab((size_t)ntile + 1, 0.0f), glist, pack;
                for (int64_t t = 0; t < ntile; t++) {
                    tab[(size_t)t] = (float)glist.size();
                    for (int64_t gq = 0; gq < ngrp; gq++) {
                        bool any = false;
                        for (int64_t i = 0; i < 16 && !any; i++)
                            for (int64_t k = 0; k < 16 && !any; k++) {
                                const int64_t nn = 16 * t + i, kk = 16 * gq + k;
                                any = nn < N && kk < K && W[(size_t)(g.r.w.offset + nn * K + kk)] != 0.0f;
                            }
                        if (!any) continue;
                        glist.push_back((float)gq);
                        for (int lane = 0; lane < 64; lane++)
                            for (int j = 0; j < 4; j++) {
                                const int64_t nn = 16 * t + (lane & 15), kk = 16 * gq + 4 * (lane >> 4) + j;
                                pack.push_back(nn < N && kk < K ? W[(size_t)(g.r.w.offset + nn * K + kk)] : 0.0f);
                            }
                    }
                }
                tab[(size_t)ntile] = (float)glist.size();
                FftDesc probe2 = d;
                probe2.mel_mode = 1; probe2.mel_groups = (int32_t)glist.size(); probe2.spec_stride = (int32_t)(16 * ngrp + 8);
                if (!glist.empty() && glist.size() < (1u << 22) && stft_lds_bytes(probe2, 8) <= 156 * 1024) {
                    d = probe2;
                    tab.insert(tab.end(), glist.begin(), glist.end());
                    mstart = tab;
                    ment = pack;
                }
            }
            if (ment.empty()) { ment.push_back(0.0f); ment.push_back(0.0f); }
            d.mel_has_bias = gd.has_bias;
            d.mel_act = gd.act; d.mel_p0 = gd.p0; d.mel_p1 = gd.p1;
            d.npost = gd.npost;
            for (int q = 0; q < 4; q++) { d.post_act[q] = gd.post_act[q]; d.post_p0[q] = gd.post_p0[q]; d.post_p1[q] = gd.post_p1[q]; }
            d.c_bs = gd.c_bs;
            if (gd.out_strided) { d.out_rs = gd.out_rs; d.out_cs = gd.out_cs; }
            else { d.out_rs = gd.ldc; d.out_cs = 1; }
            f.r.mel.start = Ref{Space::CONSTS, add_const(plan, mstart), 0};
            f.r.mel.entries = Ref{Space::CONSTS, add_const(plan, ment), 0};
            f.r.mel.bias = g.r.bias;
            f.r.out = g.r.out;
            f.name += "+" + g.name;
            const double nnz = d.mel_mode == 1 ? 256.0 * (double)d.mel_groups : (double)nnz_count;  // multiply-adds performed per frame
            f.flops_fft += 2.0 * nnz * (double)d.frames;
            f.macs += nnz * (double)d.frames;
            f.weight_bytes += 4.0 * (mstart.size() + ment.size());
            f.bytes += g.bytes - 8.0 * (double)d.frames * (double)d.nout;  // the spectrum rows never touch memory
            plan.dft_gemm_macs += g.macs;  // the dense mel product belongs to the matrix-product count of the front end
            plan.dft_performed_macs += nnz * (double)d.frames;
            plan.dft_fft_equiv_flops += 2.0 * nnz * (double)d.frames;
            plan.ops.erase(plan.ops.begin() + u[1]);
            changed = true;
        }
    }
    changed = pre_on;
    while (changed) {
        changed = false;
        const auto users = arena_users(plan);
        for (size_t e = 0; e < plan.ops.size() && !changed; e++) {
            PlanOp &el = plan.ops[e];
            const EltDesc &ed = el.elt;
            if (el.kind != OpKind::ELT || el.r.out.space != Space::ARENA || plan.storages[el.r.out.id].pinned) continue;
            if (ed.nd != 1 || ed.so[0] != 1 || ed.sa[0] != 1 || el.r.out.offset != 0) continue;
            bool scalar_ops = true;
            for (int k = 0; k < ed.nstages; k++)
                scalar_ops = scalar_ops && stft_act_supported(ed.st[k].act) &&
                             (ed.st[k].bin == BIN_NONE || (ed.st[k].sb[0] == 0 && !ed.st[k].bsq && stft_bin_supported(ed.st[k].bin)));
            if (!scalar_ops) continue;
            const auto &u = users[el.r.out.id];
            if (u.size() < 2 || u[0] != (int)e) continue;
            // every reader is a launch that can apply the chain while it loads its span: an STFT, or (round 4) a folded framing GEMM that
            // is certain to run on its LDS-resident kernel (half fold: frame_fold_post_ok; quarter fold: always)
            auto framing_gemm = [&](const PlanOp &f) {
                const GemmDesc &g = f.gemm;
                if (f.kind != OpKind::GEMM || f.pre.n != 0 || f.se_fused || sw_int(sw::BN_FRAME_PRE) == 0) return false;
                if (!(g.fold == 2 ? frame_fold2_shape_ok(g, nullptr) : (g.fold == 1 || g.fold == -1) && frame_fold_post_ok(g))) return false;
                return g.a_bs == ed.bo && (g.rows - 1) * g.lda + g.fold_n <= ed.per_sample;
            };
            bool all_fft = true;
            for (size_t q = 1; q < u.size(); q++) {
                const PlanOp &f = plan.ops[u[q]];
                const bool stft_ok = f.kind == OpKind::FFT && f.fft.npre == 0 && f.fft.a_bs == ed.bo && (int64_t)(f.fft.frames - 1) * f.fft.hop + f.fft.L <= ed.per_sample;
                all_fft = all_fft && (stft_ok || framing_gemm(f)) && f.r.a.space == Space::ARENA && f.r.a.id == el.r.out.id && f.r.a.offset == 0;
                // (the launch must read the chain's result only through `a`)
                all_fft = all_fft && refs_to(f, Space::ARENA, el.r.out.id) == 1;
            }
            if (!all_fft) continue;
            for (size_t q = 1; q < u.size(); q++) {
                PlanOp &f = plan.ops[u[q]];
                f.r.a = el.r.a;
                if (f.kind == OpKind::FFT) {
                    f.fft.a_bs = ed.ba;
                    f.fft.npre = ed.nstages;
                } else {
                    f.gemm.a_bs = ed.ba;
                    f.pre.n = ed.nstages;
                }
                for (int k = 0; k < ed.nstages; k++) {
                    if (f.kind == OpKind::FFT) {
                        f.fft.pre_bin[k] = ed.st[k].bin; f.fft.pre_act[k] = ed.st[k].act;
                        f.fft.pre_p0[k] = ed.st[k].p0; f.fft.pre_p1[k] = ed.st[k].p1; f.fft.pre_bb[k] = ed.st[k].bb;
                    } else {
                        f.pre.bin[k] = ed.st[k].bin; f.pre.act[k] = ed.st[k].act;
                        f.pre.p0[k] = ed.st[k].p0; f.pre.p1[k] = ed.st[k].p1; f.pre.bb[k] = ed.st[k].bb;
                    }
                    f.r.chain[k] = el.r.chain[k];
                }
                f.name = el.name + "+" + f.name;
            }
            plan.ops.erase(plan.ops.begin() + (long)e);
            changed = true;
        }
    }
    // (round 5) the zero-padded copy of the signal a padded framing conv reads (pad_copy: one fill + one copy launch) in the STFT's span
    // load: where the only reader of that copy is an FFT launch, the launch reads the signal itself and zero-fills the positions that
    // fall into the padding (FftDesc::pad_l, in_len).  Perch's front end: two launches and a round trip of the signal less.
    changed = sw_int(sw::BN_STFT_PAD) != 0;
    while (changed) {
        changed = false;
        const auto users = arena_users(plan);
        for (size_t e = 0; e + 2 < plan.ops.size() && !changed; e++) {
            const PlanOp &fill = plan.ops[e], &copy = plan.ops[e + 1];
            if (fill.kind != OpKind::ELT || copy.kind != OpKind::ELT || fill.name.rfind("pad.fill:", 0) != 0 || copy.name.rfind("pad.copy:", 0) != 0) continue;
            if (fill.r.out.space != Space::ARENA || copy.r.out.space != Space::ARENA || fill.r.out.id != copy.r.out.id || fill.r.out.offset != 0 || plan.storages[fill.r.out.id].pinned) continue;
            const EltDesc &fd = fill.elt, &cd = copy.elt;
            if (fd.nd != 1 || cd.nd != 1 || fd.nstages != 1 || cd.nstages != 1 || cd.so[0] != 1 || cd.sa[0] != 1) continue;
            if (fd.st[0].bin != BIN_NONE || fd.st[0].act != ACT_NONE || cd.st[0].bin != BIN_NONE || cd.st[0].act != ACT_NONE) continue;
            if (fill.r.a.space != Space::CONSTS || plan.consts[(size_t)fill.r.a.id].empty() || plan.consts[(size_t)fill.r.a.id][(size_t)fill.r.a.offset] != 0.0f) continue;
            if (copy.r.a.space != Space::ARENA && copy.r.a.space != Space::INPUT) continue;
            const auto &u = users[fill.r.out.id];
            if (u.size() != 3 || u[0] != (int)e || u[1] != (int)e + 1) continue;
            PlanOp &f = plan.ops[(size_t)u[2]];
            if (f.kind != OpKind::FFT || f.fft.in_len != 0 || f.fft.npre != 0 || f.r.a.space != Space::ARENA || f.r.a.id != fill.r.out.id || f.r.a.offset != 0) continue;
            if (f.fft.a_bs != fd.bo || (int64_t)(f.fft.frames - 1) * f.fft.hop + f.fft.L > fd.per_sample || copy.r.out.offset + cd.per_sample > fd.per_sample) continue;
            if (cd.per_sample >= ((int64_t)1 << 30) || copy.r.out.offset >= ((int64_t)1 << 30)) continue;
            if (refs_to(f, Space::ARENA, fill.r.out.id) != 1) continue;
            f.r.a = copy.r.a;
            f.fft.a_bs = cd.ba;
            f.fft.pad_l = (int32_t)copy.r.out.offset;
            f.fft.in_len = (int32_t)cd.per_sample;
            f.bytes -= 4.0 * (double)(fd.per_sample - cd.per_sample);
            f.name = "pad+" + f.name;
            plan.ops.erase(plan.ops.begin() + (long)e, plan.ops.begin() + (long)e + 2);
            changed = true;
        }
    }
}

// (K, round 4) GlobalAveragePool behind a 1x1 conv whose 48 rows per sample sit in one block of the LDS-DMA GEMM (48-row tiles): the
// epilogue writes the mean over the rows instead of the rows (gemm_dma.hip; fixed order: m-tiles ascending, then a butterfly over the 16
// rows of a tile), the [48, N] tensor is neither written nor read and the reduction launch is gone.  v2.4's head: Conv_261 (320 -> 1024,
// ReLU) + GlobalAveragePool_264.  BN_GEMMGAP=0 disables.
void fuse_gap_into_gemm(Plan &plan) {
    if (sw_int(sw::BN_GEMMGAP) == 0) return;
    bool changed = true;
    while (changed) {
        changed = false;
        const auto users = arena_users(plan);
        for (size_t j = 0; j < plan.ops.size() && !changed; j++) {
            PlanOp &red = plan.ops[j];
            const ReduceDesc &r = red.red;
            if (red.kind != OpKind::REDUCE || r.op != RED_MEAN || r.pair || red.r.a.space != Space::ARENA || red.r.out.space != Space::ARENA) continue;
            const auto &u = users[red.r.a.id];
            if (u.size() != 2 || u[1] != (int)j || plan.storages[red.r.a.id].pinned) continue;
            PlanOp &g = plan.ops[u[0]];
            if (g.kind != OpKind::GEMM || g.r.out.space != Space::ARENA || g.r.out.id != red.r.a.id || g.r.out.offset != red.r.a.offset || g.se_fused) continue;
            GemmDesc d = g.gemm;
            if (d.gap || !gemm_gap_shape_ok(d) || gemm_dma_shape(d) != 2 || d.ldc != d.N || d.c_bs != d.rows * d.N) continue;
            // the reduction: every channel's mean over the sample's rows, [rows, N] -> [N], dense
            // (the reduced dims -- H, W of the map -- nest into one run of `rows` rows of N floats)
            bool rows_run = r.nr >= 1 && r.nr <= 3 && r.rin[r.nr - 1] == d.N;
            int64_t nrows = 1;
            for (int q = r.nr - 1; q >= 0 && rows_run; q--) {
                rows_run = r.rin[q] == d.N * nrows;
                nrows *= r.rsize[q];
            }
            if (r.nk != 1 || !rows_run || nrows != d.rows || r.ksize[0] != d.N || r.kin[0] != 1 || r.kout[0] != 1 || r.bi != d.c_bs) continue;
            if (red.r.out.offset % 4 != 0 || r.bo % 4 != 0) continue;  // (dwordx4 stores)
            d.gap = 1;
            d.c_bs = r.bo;
            g.gemm = d;
            g.r.out = red.r.out;
            g.name += "+" + red.name;
            g.bytes += red.bytes - 8.0 * (double)d.rows * d.N;  // the [rows, N] tensor never touches memory
            plan.ops.erase(plan.ops.begin() + (long)j);
            changed = true;
        }
    }
}

// The untangle table of every FFT launch goes from rows [nout][8 | 12] to PLANES: [nout][4] (two buffer positions, first two
// coefficients), [nout][2] (the other two), [nout][4] (power mode: the second linear form).  The kernel's lanes read consecutive
// outputs: 32-byte row strides put the 16-byte reads 2-way and the 8-byte reads 4-way on the LDS banks (53 % of the bin phase's
// LDS cycles were conflicts); consecutive 16- and 8-byte elements of a plane do not conflict.
void planar_stft_tables(Plan &plan) {
    for (PlanOp &f : plan.ops) {
        FftDesc &d = f.fft;
        if (f.kind != OpKind::FFT || d.otab_planar || f.r.fft.otab.space != Space::CONSTS) continue;
        const int stride = d.otab_stride > 0 ? d.otab_stride : 8;
        const std::vector<float> &ot = plan.consts[f.r.fft.otab.id];
        const int64_t n = d.nout;
        if ((int64_t)ot.size() < f.r.fft.otab.offset + n * stride) continue;
        std::vector<float> pl((size_t)(n * (d.power ? 10 : 6)), 0.0f);
        for (int64_t c = 0; c < n; c++) {
            const float *r = &ot[(size_t)(f.r.fft.otab.offset + c * stride)];
            for (int q = 0; q < 4; q++) pl[(size_t)(c * 4 + q)] = r[q];
            for (int q = 0; q < 2; q++) pl[(size_t)(4 * n + c * 2 + q)] = r[4 + q];
            if (d.power)
                for (int q = 0; q < 4; q++) pl[(size_t)(6 * n + c * 4 + q)] = r[8 + q];
        }
        f.r.fft.otab = Ref{Space::CONSTS, add_const(plan, pl), 0};
        d.otab_planar = 1;
    }
}

// (F) The chunk stages of a whole-range min and a whole-range max over the SAME input (the min-max normalisation
// after the max(x - s) rewrite) read it in one pass: the later launch is folded into the earlier one (kernels.h,
// ReduceDesc::pair).  Exact, order-independent operations: same bits.  BN_REDUCE_PAIR=0 disables.
void pair_minmax_reductions(Plan &plan) {
    if (!sw_on(sw::BN_REDUCE_PAIR)) return;
    for (size_t i = 0; i < plan.ops.size(); i++) {
        PlanOp &a = plan.ops[i];
        if (a.kind != OpKind::REDUCE || a.red.pair || a.red.op != RED_MIN) continue;
        for (size_t j = i + 1; j < plan.ops.size() && j < i + 4; j++) {
            PlanOp &b = plan.ops[j];
            if (b.kind != OpKind::REDUCE || b.red.pair || b.red.op != RED_MAX) continue;
            const ReduceDesc &x = a.red, &y = b.red;
            const bool same_in = a.r.a.space == b.r.a.space && a.r.a.id == b.r.a.id && a.r.a.offset == b.r.a.offset;
            const bool chunks = x.nk == 1 && x.nr == 1 && x.rin[0] == 1 && x.kout[0] == 1 && x.red % 4 == 0 && x.kin[0] % 4 == 0 && x.bi % 4 == 0 &&
                                a.r.a.offset % 4 == 0 && x.inner_kept == 0;
            const bool same_shape = y.nk == 1 && y.nr == 1 && y.rin[0] == 1 && y.kout[0] == 1 && x.ksize[0] == y.ksize[0] && x.kin[0] == y.kin[0] &&
                                    x.red == y.red && x.bi == y.bi && x.kept == y.kept;
            if (!same_in || !chunks || !same_shape) continue;
            // nothing in between may write the shared input or read the max partials (they are only read later)
            bool clash = false;
            for (size_t k = i + 1; k < j; k++) {
                const PlanOp &m = plan.ops[k];
                clash = clash || (m.r.out.space == a.r.a.space && m.r.out.id == a.r.a.id) || (m.r.a.space == b.r.out.space && m.r.a.id == b.r.out.id);
            }
            if (clash) continue;
            a.red.pair = 1;
            a.red.bo2 = y.bo;
            a.r.pair_out = b.r.out;
            a.name += "+" + b.name;
            a.bytes += 4.0 * (double)y.kept;
            plan.ops.erase(plan.ops.begin() + (long)j);
            break;
        }
    }
}

// (E) An elementwise chain of unary stages (power-law compression, affine maps, layout copies) whose primary
// operand is the dense result of the GEMM launched just for it moves into that GEMM's epilogue: the stages run
// on the accumulators and the store goes through the chain's output view (kernels.h, GemmDesc::npost /
// out_strided).  v2.4 front end: mel MatMul -> x^2 -> x^p -> flip / transpose into the 2-channel image, per
// branch one launch instead of two and no dense [frames, mels] round trip.  BN_GEMMPOST=0 disables.
void absorb_chains_into_gemms(Plan &plan) {
    if (!sw_on(sw::BN_GEMMPOST)) return;
    bool changed = true;
    while (changed) {
        changed = false;
        const auto users = arena_users(plan);
        for (size_t j = 0; j < plan.ops.size() && !changed; j++) {
            PlanOp &cons = plan.ops[j];
            if (cons.kind != OpKind::ELT || cons.r.a.space != Space::ARENA || cons.r.out.space != Space::ARENA) continue;
            const auto &u = users[cons.r.a.id];
            if (u.size() != 2 || u[1] != (int)j || plan.storages[cons.r.a.id].pinned) continue;
            PlanOp &prod = plan.ops[u[0]];
            if (prod.kind != OpKind::GEMM || prod.r.out.space != Space::ARENA || prod.r.out.id != cons.r.a.id) continue;
            GemmDesc g = prod.gemm;
            const EltDesc &ce = cons.elt;
            // (round 4: the LDS-resident folded framing GEMM carries a chain of the compact stage functions and the consumer's view too)
            const bool fold_post = (g.fold == 1 || g.fold == -1) && frame_fold_post_ok(g);
            if (g.npost || g.out_strided || !(gemm_accepts_post(g) || fold_post) || g.ldc != g.N || g.c_bs != g.rows * g.N || ce.ba != g.c_bs) continue;
            bool unary = true, compact = true;
            int npost = 0;
            for (int k = 0; k < ce.nstages; k++) {
                unary = unary && ce.st[k].bin == BIN_NONE;
                if (ce.st[k].act != ACT_NONE) { npost++; compact = compact && stft_act_supported(ce.st[k].act); }
            }
            if (!unary || npost > 4 || ce.per_sample != g.rows * g.N || (fold_post && !compact)) continue;
            // the chain's index space must be (a signed permutation of) rows x N
            int64_t rs = 0, cs = 0, base = cons.r.out.offset, want_delta = 0;
            bool ok = true, have_row = g.rows == 1, have_col = g.N == 1;
            for (int k = 0; k < ce.nd && ok; k++) {
                if (ce.size[k] == 1) continue;
                const int64_t sa = ce.sa[k], mag = sa < 0 ? -sa : sa;
                int64_t *dst = nullptr;
                if (!have_col && !have_row && sa == 1 && ce.size[k] == g.rows * g.N) {  // flat map over the dense result
                    rs = g.N * ce.so[k]; cs = ce.so[k]; have_row = have_col = true;
                    continue;
                }
                if (!have_col && mag == 1 && ce.size[k] == g.N) { dst = &cs; have_col = true; }
                else if (!have_row && mag == g.N && ce.size[k] == g.rows) { dst = &rs; have_row = true; }
                else { ok = false; break; }
                if (sa > 0) *dst = ce.so[k];
                else { *dst = -ce.so[k]; base += (ce.size[k] - 1) * ce.so[k]; want_delta += (ce.size[k] - 1) * mag; }
            }
            if (!ok || !have_row || !have_col || cons.r.a.offset - prod.r.out.offset != want_delta) continue;
            g.out_strided = 1;
            g.out_rs = rs; g.out_cs = cs;
            g.c_bs = ce.bo;
            g.npost = 0;
            for (int k = 0; k < ce.nstages; k++)
                if (ce.st[k].act != ACT_NONE) {
                    g.post_act[g.npost] = ce.st[k].act; g.post_p0[g.npost] = ce.st[k].p0; g.post_p1[g.npost] = ce.st[k].p1;
                    g.npost++;
                }
            prod.gemm = g;
            prod.r.out = Ref{cons.r.out.space, cons.r.out.id, base};
            prod.name += "+" + cons.name;
            prod.bytes += cons.bytes - 8.0 * (double)ce.per_sample;  // the dense intermediate never touches memory
            plan.ops.erase(plan.ops.begin() + j);
            changed = true;
        }
    }
}

// --------------------------------------------------------- memory plan
// (round 5) every GEMM the one-tile-per-block LDS-DMA kernel takes gets its weights as three exact bf16 planes (plan_rules.h, pack_w3):
// the launch then runs on the bf16 matrix pipe with f32-complete products (gemm_dma3.hip).  Last pass over the descriptors: gate, pooled
// epilogue, inline squeeze-excite are all decided.  The f32 copy goes away with it when no other launch reads it.
void pack_bf16x3_weights(Plan &plan) {
    for (auto &op : plan.ops) {
        if (op.kind != OpKind::GEMM || op.gemm.fold || op.gemm.w3 || op.r.w.space != Space::CONSTS) continue;
        if (!gemm_b3_shape_ok(op.gemm) && !gemm_dma3_wanted(op.gemm)) continue;
        const int64_t N = op.gemm.N, K = op.gemm.K;
        if ((int64_t)plan.consts[(size_t)op.r.w.id].size() < op.r.w.offset + N * K) continue;
        // BN_GEMM3: 0 = exact-f32 kernel, 1 = the LDS-DMA form everywhere, 2 (default) = the register-staged form wherever it applies
        const bool b3 = gemm_b3_shape_ok(op.gemm);
        std::vector<float> img = b3 ? pack_w3f(plan.consts[(size_t)op.r.w.id].data() + op.r.w.offset, N, K) : pack_w3(plan.consts[(size_t)op.r.w.id].data() + op.r.w.offset, N, K);
        int users = 0;
        for (const auto &o2 : plan.ops) users += refs_to(o2, Space::CONSTS, op.r.w.id);
        if (users == 1 && op.r.w.offset == 0) plan.consts[(size_t)op.r.w.id] = std::move(img);
        else op.r.w = Ref{Space::CONSTS, add_const(plan, img), 0};
        op.gemm.w3 = b3 ? 2 : 1;
        op.weight_bytes += 2.0 * (double)N * (double)((K + 31) / 32 * 32) + 4.0 * (double)N * (double)((K + 31) / 32 * 32 - K);  // 6 bytes per (padded) weight instead of 4
    }
}

void plan_memory(Plan &plan) {
    // greedy first-fit over the linear launch order; storages are per-sample extents,
    // rounded to 64 elements so that (offset * max_batch) stays 256-byte aligned.
    struct Block { int64_t off, size; };
    std::vector<Block> free_list;
    int64_t top = 0;
    auto alloc = [&](int64_t size) {
        int best = -1;
        for (size_t k = 0; k < free_list.size(); k++)
            if (free_list[k].size >= size && (best < 0 || free_list[k].size < free_list[best].size)) best = (int)k;
        if (best >= 0) {
            int64_t off = free_list[best].off;
            if (free_list[best].size == size) free_list.erase(free_list.begin() + best);
            else { free_list[best].off += size; free_list[best].size -= size; }
            return off;
        }
        int64_t off = top;
        top += size;
        return off;
    };
    auto release = [&](int64_t off, int64_t size) {
        free_list.push_back({off, size});
        std::sort(free_list.begin(), free_list.end(), [](const Block &a, const Block &b) { return a.off < b.off; });
        for (size_t k = 0; k + 1 < free_list.size();) {
            if (free_list[k].off + free_list[k].size == free_list[k + 1].off) { free_list[k].size += free_list[k + 1].size; free_list.erase(free_list.begin() + k + 1); }
            else k++;
        }
        // give the tail back
        if (!free_list.empty() && free_list.back().off + free_list.back().size == top) { top = free_list.back().off; free_list.pop_back(); }
    };
    auto rounded = [](int64_t e) { return (e + 63) / 64 * 64; };
    int nops = (int)plan.ops.size();
    std::vector<std::vector<int>> starts(nops), ends(nops);
    for (size_t s = 0; s < plan.storages.size(); s++) {
        auto &st = plan.storages[s];
        if (st.first < 0) continue;  // never touched
        starts[st.first].push_back((int)s);
        if (!st.pinned) ends[st.last].push_back((int)s);
    }
    int64_t peak = 0;
    for (size_t s = 0; s < plan.storages.size(); s++)
        if (plan.storages[s].persistent && plan.storages[s].first >= 0) plan.storages[s].arena_off = alloc(rounded(plan.storages[s].elems));
    for (int k = 0; k < nops; k++) {
        for (int s : starts[k])
            if (!plan.storages[s].persistent) plan.storages[s].arena_off = alloc(rounded(plan.storages[s].elems));
        peak = std::max(peak, top);
        for (int s : ends[k]) release(plan.storages[s].arena_off, rounded(plan.storages[s].elems));
    }
    plan.arena_elems = std::max<int64_t>(peak, 64);
    // constants arena
    int64_t coff = 0;
    plan.const_off.resize(plan.consts.size());
    for (size_t k = 0; k < plan.consts.size(); k++) { plan.const_off[k] = coff; coff += rounded((int64_t)plan.consts[k].size()); }
    plan.consts_elems = std::max<int64_t>(coff, 64);
}

}  // namespace

void run_plan_passes(Plan &plan) {
    fuse_elementwise_chains(plan);
    absorb_chains_into_gemms(plan);
    absorb_into_stft(plan);
    planar_stft_tables(plan);
    pair_minmax_reductions(plan);
    fuse_gap_into_gemm(plan);
    absorb_se_into_gemms(plan);
    recompute_liveness(plan);
    pack_bf16x3_weights(plan);
    plan_memory(plan);
}

}  // namespace bn
