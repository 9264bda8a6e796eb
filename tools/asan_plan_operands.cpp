// Host-side check of the launch operands of a finished plan (no device needed), under ASan / UBSan: built like tools/asan_plan.cpp
// (`make tools/asan_plan_operands`), run over model files with the BN_* switches from the environment:
//   tools/asan_plan_operands model.onnx [more.onnx ...]
// for_each_ref (engine.h) is the one list of a launch's operands.  For every plan:
//   * the first / last launch of every storage, recomputed from for_each_ref alone, are the ones the planner stored -- the memory plan
//     recycles a storage after `last`, so an operand the list missed would be read after its storage was given away;
//   * every ARENA ref names a storage and every CONSTS ref a constant of the plan;
//   * the operands the launcher takes as weights, biases and tables are never ARENA.
// Between them the files must plan an MBCONV that finishes a squeeze-excite, a GEMM with one in its prologue and an FFT that absorbed
// its mel bank (BN_SEFUSE=mb BN_MBROW=0 BN_SEGEMM=1 BN_STFT=1 BN_STFT_MEL=force on the small synthetic models): otherwise the run fails
// as having checked too little.
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "engine.h"

using namespace bn;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; printf("  FAIL: " __VA_ARGS__); printf("\n"); } } while (0)

int main(int argc, char **argv) {
    long refs = 0;
    int plans = 0, tails = 0, inlines = 0, mels = 0;
    for (int a = 1; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<uint8_t> bytes((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        printf("%s (%zu bytes)\n", argv[a], bytes.size());
        OnnxModel m = parse_onnx(bytes.data(), bytes.size());
        std::vector<int> all;
        for (size_t k = 0; k < m.outputs.size(); k++) all.push_back((int)k);
        const std::unique_ptr<Plan> p = build_plan(m, all);
        plans++;
        const int ns = (int)p->storages.size(), nc = (int)p->consts.size();
        std::vector<int> first((size_t)ns, -1), last((size_t)ns, -1);
        for (size_t k = 0; k < p->ops.size(); k++) {
            const PlanOp &op = p->ops[k];
            const char *name = op.name.c_str();
            for_each_ref(op.r, [&](const Ref &r) {
                refs += r.space != Space::NONE;
                if (r.space == Space::CONSTS) CHECK(r.id >= 0 && r.id < nc, "op %zu '%s': constant %d of %d", k, name, (int)r.id, nc);
                if (r.space != Space::ARENA) return;
                CHECK(r.id >= 0 && r.id < ns, "op %zu '%s': storage %d of %d", k, name, (int)r.id, ns);
                if (r.id < 0 || r.id >= ns) return;
                if (first[(size_t)r.id] < 0) first[(size_t)r.id] = (int)k;
                last[(size_t)r.id] = (int)k;
            });
            const PlanOp::Operands &r = op.r;
            for (const Ref *c : {&r.w, &r.bias, &r.w2, &r.bias2, &r.se.w1, &r.se.b1, &r.se.w2t, &r.se.b2, &r.fft.window, &r.fft.twiddles, &r.fft.otab,
                                 &r.mel.start, &r.mel.entries, &r.mel.bias, &r.fold2.tables, &r.fold2.colmap})
                CHECK(c->space == Space::CONSTS || c->space == Space::NONE, "op %zu '%s': a weight, bias or table in space %d", k, name, (int)c->space);
            CHECK(r.out.space == Space::ARENA, "op %zu '%s': result in space %d", k, name, (int)r.out.space);
            tails += op.kind == OpKind::MBCONV && op.se_fused && r.se.gate.space == Space::ARENA && r.se.counter.space == Space::ARENA;
            inlines += op.kind == OpKind::GEMM && op.se_fused && r.se.partial.space == Space::ARENA;
            mels += op.kind == OpKind::FFT && op.fft.nmel > 0 && r.mel.start.space == Space::CONSTS && r.mel.entries.space == Space::CONSTS;
        }
        for (int s = 0; s < ns; s++) {
            const Storage &st = p->storages[(size_t)s];
            CHECK(st.first == first[(size_t)s] && st.last == last[(size_t)s], "storage %d: planned over launches %d..%d, its operands span %d..%d", s, st.first, st.last,
                  first[(size_t)s], last[(size_t)s]);
        }
        printf("  %zu launches, %d storages, %d constants\n", p->ops.size(), ns, nc);
    }
    CHECK(tails > 0 && inlines > 0 && mels > 0, "checked too little: %d MBCONV with a squeeze-excite tail, %d GEMM with an inline one, %d FFT with a mel bank", tails, inlines, mels);
    printf("%d plans, %ld operands, %d tails, %d inline, %d mel banks, %d failures\n", plans, refs, tails, inlines, mels, failures);
    return failures ? 1 : 0;
}
