// Host-side printer of a launch plan, by value (no device needed): two builds of the planner agree on a model exactly when their outputs
// here are the same text.  Built like tools/asan_plan.cpp, without the sanitizers:
//   g++ -std=c++17 -O1 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Irust-birdnet-onnx_amd/csrc tools/plan_digest.cpp
//       rust-birdnet-onnx_amd/csrc/{onnx_proto,engine,onnx_rewrite,dft_bank,mbconv_fuse,plan_passes,detect}.cpp -o /tmp/plan_digest
//   /tmp/plan_digest model.onnx [more.onnx ...]      (BN_* switches from the environment, as for the library)
// Every launch with its operands and every field of the descriptors its kind uses (field by field: struct padding is undefined), every
// storage, every output, the plan's totals, and the length and an FNV-1a-64 hash of every constant.  Doubles and floats print as %a.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "engine.h"

using namespace bn;

#define I(d, f) printf(" " #f "=%lld", (long long)(d).f)
#define X(d, f) printf(" " #f "=%a", (double)(d).f)
#define IA(d, f) do { printf(" " #f "="); for (auto v_ : (d).f) printf("%lld,", (long long)v_); } while (0)
#define XA(d, f) do { printf(" " #f "="); for (auto v_ : (d).f) printf("%a,", (double)v_); } while (0)

static int refs_printed;  // ... that were not NONE, per launch
static void ref(const char *name, const Ref &r) {
    printf(" %s=%d:%d:%lld", name, (int)r.space, (int)r.id, (long long)r.offset);
    refs_printed += r.space != Space::NONE;
}

static void print(const EltDesc &d) {
    printf("\n    elt:"); I(d, nd); IA(d, size); IA(d, so); IA(d, sa); I(d, bo); I(d, ba); I(d, per_sample); I(d, nstages);
    for (const EltStage &s : d.st) { printf("\n      stage:"); I(s, bin); I(s, act); X(s, p0); X(s, p1); IA(s, sb); I(s, bb); I(s, bsq); I(s, reserved); }
}
static void print(const ReduceDesc &d) {
    printf("\n    red:"); I(d, nk); I(d, nr); IA(d, ksize); IA(d, kin); IA(d, kout); IA(d, rsize); IA(d, rin); I(d, bi); I(d, bo); I(d, kept); I(d, red);
    I(d, op); I(d, inner_kept); I(d, pair); I(d, bo2);
}
static void print(const char *name, const GemmDesc &d) {
    printf("\n    %s:", name); I(d, rows); I(d, K); I(d, N); I(d, lda); I(d, a_bs); I(d, ldc); I(d, c_bs); I(d, ldr); I(d, r_bs); I(d, act); X(d, p0); X(d, p1);
    I(d, has_bias); I(d, has_res); I(d, has_scale); I(d, s_bs); I(d, fold); I(d, fold_n); I(d, fold_ne); I(d, fold_wpk); I(d, npost); I(d, out_strided);
    IA(d, post_act); XA(d, post_p0); XA(d, post_p1); I(d, out_rs); I(d, out_cs); I(d, se_inline); I(d, gap); I(d, w3);
}
static void print(const FramePre &d) { printf("\n    pre:"); I(d, n); IA(d, bin); IA(d, act); XA(d, p0); XA(d, p1); IA(d, bb); }
static void print(const ConvDesc &d) {
    printf("\n    conv:"); I(d, H); I(d, W); I(d, Cin); I(d, OH); I(d, OW); I(d, Cout); I(d, kh); I(d, kw); I(d, sh); I(d, sw); I(d, pt); I(d, pl); I(d, dh); I(d, dw);
    I(d, groups); I(d, act); X(d, p0); X(d, p1); I(d, has_bias); I(d, has_res); I(d, in_bs); I(d, out_bs);
}
static void print(const DwDesc &d) {
    printf("\n    dw:"); I(d, H); I(d, W); I(d, C); I(d, OH); I(d, OW); I(d, kh); I(d, kw); I(d, sh); I(d, sw); I(d, pt); I(d, pl); I(d, dh); I(d, dw); I(d, act);
    X(d, p0); X(d, p1); I(d, has_bias); I(d, in_bs); I(d, out_bs); I(d, tiled); I(d, tw); I(d, rpb); I(d, nblk); I(d, has_gap); I(d, gap_bs); I(d, mapt);
}
static void print(const MbDesc &d) {
    printf("\n    mb:"); I(d, H); I(d, W); I(d, Cin); I(d, C); I(d, OH); I(d, OW); I(d, k); I(d, s); I(d, pt); I(d, pl); I(d, act1); I(d, act2); X(d, p0_1); X(d, p1_1);
    X(d, p0_2); X(d, p1_2); I(d, has_bias1); I(d, has_bias2); I(d, in_bs); I(d, out_bs); I(d, tiles_x); I(d, tiles_y); I(d, whole_map); I(d, k1); I(d, s1);
    I(d, pt1); I(d, pl1); I(d, H1); I(d, W1); I(d, Cin1); I(d, has_gap); I(d, gap_bs); I(d, row_mode); I(d, toh); I(d, row_tr); I(d, dbg); I(d, map_bands);
    I(d, map_tr); I(d, cin_pad); I(d, row_b3); I(d, map_ws); I(d, map_b3);
}
static void print(const PoolDesc &d) {
    printf("\n    pool:"); I(d, H); I(d, W); I(d, C); I(d, OH); I(d, OW); I(d, kh); I(d, kw); I(d, sh); I(d, sw); I(d, pt); I(d, pl); I(d, is_max);
    I(d, count_include_pad); I(d, in_bs); I(d, out_bs);
}
static void print(const GapDesc &d) { printf("\n    gap:"); I(d, HW); I(d, C); I(d, splits); I(d, in_bs); I(d, out_bs); }
static void print(const SeFcDesc &d) {
    printf("\n    se:"); I(d, C); I(d, Cr); I(d, splits); X(d, inv_hw); I(d, act1); I(d, act2); X(d, p0_1); X(d, p1_1); X(d, p0_2); X(d, p1_2); I(d, in_bs); I(d, out_bs);
}
static void print(const FftDesc &d) {
    printf("\n    fft:"); I(d, L); I(d, M); I(d, logM); I(d, hop); I(d, frames); I(d, nout); I(d, tpb); I(d, F); I(d, npass); IA(d, pass_n); IA(d, pass_r); IA(d, pass_tw);
    I(d, tw_count); I(d, a_bs); I(d, a_vec4); I(d, dbg); I(d, npre); IA(d, pre_bin); IA(d, pre_act); XA(d, pre_p0); XA(d, pre_p1); IA(d, pre_bb); I(d, ldc);
    I(d, c_bs); I(d, has_bias); I(d, nmel); I(d, mel_nnz); I(d, mel_has_bias); I(d, mel_act); X(d, mel_p0); X(d, mel_p1); I(d, npost); IA(d, post_act);
    XA(d, post_p0); XA(d, post_p1); I(d, out_rs); I(d, out_cs); I(d, power); I(d, otab_stride); I(d, mel_mode); I(d, mel_groups); I(d, spec_stride);
    I(d, otab_planar); I(d, pad_l); I(d, in_len);
}

static void print(const PlanOp &op, size_t k) {
    static const char *kinds[] = {"ELT", "REDUCE", "GEMM", "CONV", "DWCONV", "GAP", "SEFC", "MBCONV", "POOL", "FFT"};
    printf("op %zu %s '%s'\n   ", k, kinds[(int)op.kind], op.name.c_str());
    // The operands print in the nine generic slots, the chain ("eb") and the four extras ("x") the plan had before its fields were named, so
    // that digests compare across that change: per kind, the named field that lived in each slot; a slot the kind left empty prints NONE.
    const PlanOp::Operands &r = op.r;
    const Ref none;
    refs_printed = 0;
    const bool gemm = op.kind == OpKind::GEMM, fft = op.kind == OpKind::FFT, two = op.kind == OpKind::MBCONV || op.kind == OpKind::SEFC;
    const bool tail = op.se_fused && (op.kind == OpKind::DWCONV || op.kind == OpKind::MBCONV), inl = op.se_fused && gemm;
    ref("out", r.out); ref("a", r.a);
    ref("b", op.kind == OpKind::REDUCE ? r.pair_out : op.kind == OpKind::SEFC ? r.hidden : gemm ? r.se.partial : r.gap_out);
    ref("w", fft ? r.fft.window : r.w); ref("bias", r.bias);
    ref("res", tail ? r.se.gate : r.residual); ref("scale", tail ? r.se.counter : r.gate);
    ref("w2", two ? r.w2 : fft ? r.fft.twiddles : gemm ? r.fold2.tables : none);
    ref("bias2", two ? r.bias2 : fft ? r.fft.otab : gemm ? r.fold2.colmap : none);
    for (const Ref &e : r.chain) ref("eb", e);
    const Ref *x[4] = {&none, &none, &none, &none};
    if (tail || inl) { x[0] = &r.se.w1; x[1] = &r.se.b1; x[2] = &r.se.w2t; x[3] = &r.se.b2; }
    if (fft) { x[0] = &r.mel.start; x[1] = &r.mel.entries; x[3] = &r.mel.bias; }
    for (const Ref *e : x) ref("x", *e);
    int set = 0;  // a field set where its kind has no slot for it must not go unseen
    for_each_ref(r, [&](const Ref &e) { set += e.space != Space::NONE; });
    if (set != refs_printed) printf(" UNPRINTED=%d", set - refs_printed);
    switch (op.kind) {
        case OpKind::ELT: print(op.elt); break;
        case OpKind::REDUCE: print(op.red); break;
        case OpKind::GEMM: print("gemm", op.gemm); print(op.pre); print(op.se); break;
        case OpKind::CONV: print(op.conv); break;
        case OpKind::DWCONV: print(op.dw); print(op.se); break;
        case OpKind::GAP: print(op.gap); break;
        case OpKind::SEFC: print(op.se); break;
        case OpKind::MBCONV: print(op.mb); print(op.se); break;
        case OpKind::POOL: print(op.pool); break;
        case OpKind::FFT: print(op.fft); break;
    }
    printf("\n   "); I(op, se_fused); I(op, mfma); X(op, flops_fft); X(op, macs); X(op, macs_mfma_extra); X(op, macs_recompute); X(op, macs_valu_extra); X(op, bytes);
    X(op, weight_bytes);
    printf("\n");
}

static void digest(const Plan &p) {
    printf("plan:"); I(p, sample_count); I(p, consts_elems); I(p, arena_elems); X(p, macs_mfma); X(p, macs_valu); X(p, act_bytes); X(p, weight_bytes);
    X(p, dft_gemm_macs); X(p, fft_flops); X(p, dft_performed_macs); X(p, dft_fft_equiv_flops); X(p, recompute_macs);
    printf("\nio: '%s'", p.io.input_name.c_str()); IA(p.io, input_shape);
    for (size_t k = 0; k < p.io.output_names.size(); k++) { printf(" | '%s'", p.io.output_names[k].c_str()); for (auto v : p.io.output_shapes[k]) printf(" %lld", (long long)v); }
    printf("\n");
    for (size_t k = 0; k < p.ops.size(); k++) print(p.ops[k], k);
    for (size_t k = 0; k < p.storages.size(); k++) {
        const Storage &s = p.storages[k];
        printf("storage %zu:", k); I(s, elems); I(s, first); I(s, last); I(s, pinned); I(s, persistent); I(s, arena_off); printf("\n");
    }
    for (size_t k = 0; k < p.outputs.size(); k++) {
        const OutputInfo &o = p.outputs[k];
        printf("output %zu '%s':", k, o.name.c_str()); IA(o, dims); I(o, row_elems); ref("ref", o.ref); I(o, computed); printf("\n");
    }
    for (size_t k = 0; k < p.consts.size(); k++) {
        uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a-64 over the constant's bytes
        const unsigned char *b = reinterpret_cast<const unsigned char *>(p.consts[k].data());
        for (size_t q = 0; q < p.consts[k].size() * sizeof(float); q++) h = (h ^ b[q]) * 0x100000001b3ull;
        printf("const %zu: len=%zu off=%lld fnv=%016llx\n", k, p.consts[k].size(), k < p.const_off.size() ? (long long)p.const_off[k] : -1ll, (unsigned long long)h);
    }
}

int main(int argc, char **argv) {
    for (int a = 1; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const char *base = strrchr(argv[a], '/');
        printf("== %s (%zu bytes)\n", base ? base + 1 : argv[a], bytes.size());
        try {
            OnnxModel m = parse_onnx(bytes.data(), bytes.size());
            std::vector<int> all;
            for (size_t k = 0; k < m.outputs.size(); k++) all.push_back((int)k);
            digest(*build_plan(m, all));
        } catch (const std::exception &e) {
            printf("refused: %s\n", e.what());
        }
    }
    return 0;
}
