// What the pieces of the planner share (private to csrc/; engine.h is the public face).  The planner is five programs:
//   engine.cpp        Builder: one run over the graph, the lowering of every node to launches
//   onnx_rewrite.cpp  rewrites of the ONNX graph before lowering      -- nodes and constants, never the plan
//   dft_bank.cpp      a filter bank recognised as a windowed DFT, and the FFT / quarter-fold launches it becomes
//   mbconv_fuse.cpp   a depthwise conv and the launch before it as one fused MBConv launch, where a rule allows it
//   plan_passes.cpp   passes over the finished launch list            -- the plan, never the graph
// Here: the value a graph tensor has while planning (Val), the plan's three primitives (touch, add_const, push_op) and the entry points
// of the other four files.  None of these symbols leaves the library.
#pragma once
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "engine.h"

namespace bn {
#pragma GCC visibility push(hidden)

constexpr int64_t BATCH_SENTINEL = -1000000007;  // "the batch size" inside folded shape tensors

using Dims = std::vector<int64_t>;

inline int64_t prod(const Dims &d) {
    int64_t n = 1;
    for (auto v : d) n *= v;
    return n;
}
inline Dims row_major(const Dims &d) {
    Dims s(d.size());
    int64_t acc = 1;
    for (int i = (int)d.size() - 1; i >= 0; i--) {
        s[i] = acc;
        acc *= d[i];
    }
    return s;
}
inline std::string dims_str(const Dims &d) {
    std::string s = "[";
    for (size_t i = 0; i < d.size(); i++) s += (i ? "," : "") + std::to_string(d[i]);
    return s + "]";
}

struct Val {
    bool is_const = false;
    bool is_int = false;
    Dims dims;     // const: full dims; activation: per-sample dims
    Dims strides;  // activation only (elements)
    Space space = Space::NONE;
    int32_t storage = -1;
    int64_t offset = 0;
    std::vector<float> f;
    std::vector<int64_t> i;
    // squeeze-excite: `is_gate` marks the per-channel gate vector produced by the fused SE kernel;
    // `gate_storage >= 0` marks "x * gate" not yet applied (the consuming 1x1 conv applies it on load)
    bool is_gate = false;
    int32_t gate_storage = -1;
    // (round 5) frames * window not yet applied: the constant `win_name` (vals_ key) multiplies along the `win_nu`-th NON-UNIT
    // dimension; the DFT node that consumes the value folds it into its basis, any other consumer gets apply_window() in get()
    std::string win_name;
    int32_t win_nu = -1;
    int64_t numel() const { return prod(dims); }
    bool contiguous() const { return !is_const && strides_equal(row_major(dims)); }
    bool strides_equal(const Dims &s) const {
        for (size_t k = 0; k < dims.size(); k++)
            if (dims[k] != 1 && strides[k] != s[k]) return false;
        return true;
    }
};

[[noreturn]] inline void unsupported(const OnnxNode &n, const std::string &why) {
    throw UnsupportedModel("node '" + n.name + "' (" + n.op_type + "): " + why);
}

inline Val make_const_f(const Dims &d, std::vector<float> f) {
    Val v; v.is_const = true; v.dims = d; v.f = std::move(f); return v;
}
inline Val make_const_i(const Dims &d, std::vector<int64_t> i) {
    Val v; v.is_const = true; v.is_int = true; v.dims = d; v.i = std::move(i); return v;
}
// A node the planner writes itself (rewrites, operators lowered as sequences of the operators it maps)
inline OnnxNode synth_node(const std::string &op, const std::string &name, std::vector<std::string> ins, const std::string &out) {
    OnnxNode s_;
    s_.name = name;
    s_.op_type = op;
    s_.inputs = std::move(ins);
    s_.outputs = {out};
    return s_;
}
inline void set_ints(OnnxNode &nd, const std::string &key, std::vector<int64_t> v) {
    OnnxAttr a;
    a.name = key;
    a.type = 7;
    a.ints = std::move(v);
    nd.attrs[key] = a;
}

// ------------------------------------------------------------------ the plan's primitives
// storage liveness: launch `op_index` reads or writes the storage behind `r`
inline void touch(Plan &plan, const Ref &r, int op_index) {
    if (r.space != Space::ARENA) return;
    auto &s = plan.storages[r.id];
    if (s.first < 0) s.first = op_index;
    s.last = std::max(s.last, op_index);
}
inline int32_t add_const(Plan &plan, const std::vector<float> &data) {
    plan.consts.push_back(data);
    return (int32_t)plan.consts.size() - 1;
}
inline void push_op(Plan &plan, PlanOp &&op) {
    int idx = (int)plan.ops.size();
    for_each_ref(op.r, [&](const Ref &r) { touch(plan, r, idx); });
    plan.ops.push_back(std::move(op));
}

// ------------------------------------------------------------------ onnx_rewrite.cpp
// The graph as the rewrites that run after the liveness walk see it: the node list and the constant table (both edited in place), which
// nodes the wanted outputs keep alive, the live readers of every tensor and the names of the wanted outputs.
struct LiveGraph {
    std::vector<OnnxNode> &nodes;
    std::map<std::string, Val> &vals;
    const std::vector<bool> &live;
    const std::map<std::string, std::vector<int>> &consumers;
    const std::set<std::string> &wanted;
};
void canonicalize_spectrogram_dialects(const OnnxModel &m, std::vector<OnnxNode> &nodes, std::map<std::string, Val> &vals);  // before liveness
void prune_zero_rows(const LiveGraph &g);
void merge_framing_products(const LiveGraph &g);

// ------------------------------------------------------------------ mbconv_fuse.cpp
// The depthwise launch `dw` (not yet pushed) and the launch before it as ONE MBCONV launch, where a rule allows it: replaces
// plan.ops.back() and returns true, or leaves the plan untouched.  `only_reader`: the producer's output feeds this node alone.
bool fuse_mbconv(Plan &plan, const PlanOp &dw, const std::string &node_name, bool only_reader);

// ------------------------------------------------------------------ plan_passes.cpp
// Every pass over the lowered plan, in their one fixed order, down to the memory plan.
void run_plan_passes(Plan &plan);

#pragma GCC visibility pop
}  // namespace bn
