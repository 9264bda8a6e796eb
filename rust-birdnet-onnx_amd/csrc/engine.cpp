// ONNX graph -> launch plan.  See engine.h.
//
// Conventions
//  * Every activation has the batch as its outermost dimension; `dims` /
//    `strides` below describe ONE sample (batch stripped).  Ops that would mix
//    the batch with other dimensions are refused.
//  * Activations are strided views over per-sample storages, so Transpose,
//    Reshape, Squeeze, Unsqueeze, Slice (incl. negative steps) and Identity
//    cost nothing.  Convolutions produce channels-last (NHWC / NWC) storage,
//    which is what the MFMA GEMM and the depthwise kernel want; an ONNX NCHW
//    tensor is simply the view dims=[C,H,W], strides=[1,W*C,C] over it.
//  * Conv+BatchNorm+activation(+residual Add) and MatMul/Gemm+bias+activation
//    chains are folded into one launch at import time.
//
// The planner's other four pieces -- graph rewrites before lowering, DFT-bank recognition, MBConv fusion, passes over the finished plan -- are free
// functions in files of their own (plan_build.h lists them); this file is Builder: one run over the graph and the lowering of every node.
#include "engine.h"
#include "dft_bank.h"
#include "plan_build.h"
#include "plan_rules.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>
#include <set>

namespace bn {
namespace {

struct ActSpec {
    int32_t act = ACT_NONE;
    float p0 = 0, p1 = 0;
};

// Outputs along one axis of a window of extent `ke` (dilation included) at stride `s`, floor mode (Conv and the pools): the pads as the
// attributes gave them, or as auto_pad decides
int64_t window_out_dim(const std::string &auto_pad, int64_t in, int64_t ke, int64_t s, int64_t &p0, int64_t &p1) {
    if (auto_pad == "SAME_UPPER" || auto_pad == "SAME_LOWER") {
        const int64_t o = (in + s - 1) / s;
        const int64_t tot = std::max<int64_t>((o - 1) * s + ke - in, 0);
        p0 = auto_pad == "SAME_UPPER" ? tot / 2 : tot - tot / 2;
        p1 = tot - p0;
        return o;
    }
    if (auto_pad == "VALID") p0 = p1 = 0;
    return (in + p0 + p1 - ke) / s + 1;
}

class Builder {
   public:
    Builder(const OnnxModel &m, Plan &p) : m_(m), plan_(p) {}

    void run(const std::vector<int> &wanted) {
        plan_.io = read_io_meta(m_);
        if (m_.inputs.size() != 1)
            throw UnsupportedModel("expected exactly one graph input, found " + std::to_string(m_.inputs.size()));
        nodes_ = m_.nodes;  // mutable copy (pruning edits attributes / initializers)
        for (auto &t : m_.initializers) {
            Val v;
            v.is_const = true;
            v.dims = t.dims;
            if (t.is_float()) v.f = t.f;
            else { v.is_int = true; v.i = t.i; }
            vals_[t.name] = std::move(v);
        }
        canonicalize_spectrogram_dialects(m_, nodes_, vals_);
        // graph input
        const auto &in = m_.inputs[0];
        if (!in.has_shape || in.shape.size() < 2)
            throw UnsupportedModel("graph input must have a [batch, samples] or [batch, 1, samples] shape");
        {
            Val v;
            v.dims.assign(in.shape.begin() + 1, in.shape.end());
            for (auto d : v.dims)
                if (d <= 0) throw UnsupportedModel("graph input has a dynamic non-batch dimension");
            v.strides = row_major(v.dims);
            v.space = Space::INPUT;
            vals_[in.name] = v;
            plan_.sample_count = v.numel();
        }
        // liveness from wanted outputs
        std::set<std::string> want;
        for (int w : wanted) {
            if (w < 0 || w >= (int)m_.outputs.size()) throw UnsupportedModel("wanted output index out of range");
            want.insert(m_.outputs[w].name);
        }
        for (auto &o : m_.outputs) graph_outputs_.insert(o.name);
        live_.assign(nodes_.size(), false);
        {
            std::map<std::string, int> producer;
            for (size_t k = 0; k < nodes_.size(); k++)
                for (auto &o : nodes_[k].outputs) producer[o] = (int)k;
            std::vector<std::string> stack(want.begin(), want.end());
            while (!stack.empty()) {
                std::string t = stack.back();
                stack.pop_back();
                auto it = producer.find(t);
                if (it == producer.end() || live_[it->second]) continue;
                live_[it->second] = true;
                for (auto &i : nodes_[it->second].inputs)
                    if (!i.empty()) stack.push_back(i);
            }
        }
        for (size_t k = 0; k < nodes_.size(); k++)
            if (live_[k])
                for (auto &i : nodes_[k].inputs)
                    if (!i.empty()) consumers_[i].push_back((int)k);
        wanted_names_ = want;
        absorbed_.assign(nodes_.size(), false);

        // Arity of every node up front: the lowering (and its look-ahead fusion) indexes inputs / outputs directly,
        // so a malformed file must be refused here, not found by an out-of-range read later.
        for (const auto &nd : nodes_) {
            static const std::map<std::string, size_t> min_inputs = {
                {"Add", 2}, {"Sub", 2}, {"Mul", 2}, {"Div", 2}, {"Pow", 2}, {"Max", 2}, {"Min", 2}, {"Conv", 2}, {"MatMul", 2}, {"Gemm", 2},
                {"BatchNormalization", 5}, {"Reshape", 2}, {"Gather", 2}, {"Concat", 1}};
            if (nd.outputs.empty() || nd.outputs[0].empty()) throw UnsupportedModel("node '" + nd.name + "' (" + nd.op_type + ") has no output");
            auto it = min_inputs.find(nd.op_type);
            const size_t need = it != min_inputs.end() ? it->second : (nd.op_type == "Constant" || nd.op_type == "ConstantOfShape" || nd.op_type == "Range" ? 0 : 1);
            if (nd.inputs.size() < need) throw UnsupportedModel("node '" + nd.name + "' (" + nd.op_type + ") has " + std::to_string(nd.inputs.size()) + " inputs, needs " + std::to_string(need));
            for (size_t k = 0; k < need; k++)
                if (nd.inputs[k].empty()) throw UnsupportedModel("node '" + nd.name + "' (" + nd.op_type + "): required input " + std::to_string(k) + " is missing");
        }

        const LiveGraph graph{nodes_, vals_, live_, consumers_, wanted_names_};
        prune_zero_rows(graph);
        merge_framing_products(graph);

        for (size_t k = 0; k < nodes_.size(); k++) {
            if (!live_[k] || absorbed_[k]) continue;
            cur_ = (int)k;
            lower(nodes_[k]);
        }
        // outputs
        plan_.outputs.resize(m_.outputs.size());
        for (size_t k = 0; k < m_.outputs.size(); k++) {
            auto &oi = plan_.outputs[k];
            oi.name = m_.outputs[k].name;
            if (!want.count(oi.name)) continue;
            auto it = vals_.find(oi.name);
            if (it == vals_.end()) throw UnsupportedModel("graph output '" + oi.name + "' was never produced");
            Val v = it->second;
            if (v.is_const) v = upload_as_activation(v);
            if (v.space == Space::INPUT || !v.contiguous()) v = materialize(v, row_major(v.dims), "output:" + oi.name);
            oi.dims = v.dims;
            oi.row_elems = v.numel();
            oi.ref = Ref{v.space, v.storage, v.offset};
            oi.computed = true;
            plan_.storages[v.storage].pinned = true;
        }
        run_plan_passes(plan_);
        for (auto &op : plan_.ops) {
            (op.mfma ? plan_.macs_mfma : plan_.macs_valu) += op.macs;
            plan_.macs_mfma += op.macs_mfma_extra;
            plan_.recompute_macs += op.macs_recompute;
            plan_.macs_valu += op.macs_valu_extra;
            plan_.act_bytes += op.bytes;
            plan_.weight_bytes += op.weight_bytes;
            plan_.fft_flops += op.flops_fft;
        }
    }

   private:
    const OnnxModel &m_;
    Plan &plan_;
    std::vector<OnnxNode> nodes_;
    std::map<std::string, Val> vals_;
    std::map<std::string, std::vector<int>> consumers_;
    std::set<std::string> graph_outputs_, wanted_names_;
    std::vector<bool> live_, absorbed_;
    int cur_ = 0;

    // ------------------------------------------------------------------ utils
    const Val &get(const OnnxNode &n, size_t idx) {
        if (idx >= n.inputs.size() || n.inputs[idx].empty()) unsupported(n, "missing input " + std::to_string(idx));
        auto it = vals_.find(n.inputs[idx]);
        if (it == vals_.end()) unsupported(n, "input '" + n.inputs[idx] + "' is not defined (graph not topologically sorted?)");
        if (it->second.gate_storage >= 0 && !(n.op_type == "Conv" && idx == 0)) it->second = apply_gate(it->second, n.inputs[idx]);
        if (!it->second.win_name.empty() && !(idx == 0 && (n.op_type == "DFT" || n.op_type == "Unsqueeze" || n.op_type == "Squeeze" || n.op_type == "Reshape" ||
                                                          n.op_type == "Identity")))
            it->second = apply_window(it->second, n.inputs[idx]);
        return it->second;
    }
    // frames * window as an explicit elementwise launch (fallback when the consumer is not a DFT after all)
    Val apply_window(const Val &x, const std::string &why) {
        Val plain = x;
        plain.win_name.clear();
        plain.win_nu = -1;
        const Val &w = vals_.at(x.win_name);
        int ax = -1, nu = 0;
        for (size_t k = 0; k < x.dims.size(); k++)
            if (x.dims[k] != 1 && nu++ == x.win_nu) ax = (int)k;
        if (ax < 0 || w.numel() != x.dims[ax]) throw UnsupportedModel("internal: pending window of '" + why + "' lost its axis");
        Val out = new_act(x.dims, strides_for_order(x.dims, phys_order(x)));
        Dims ws(x.dims.size(), 0);
        ws[ax] = 1;
        emit_elt("window.mul:" + why, out, ref_of(plain), plain.strides, batch_stride(plain), Ref{Space::CONSTS, add_const(w.f), 0}, ws, 0, BIN_MUL, ActSpec{});
        return out;
    }
    // x * gate as an explicit elementwise launch (fallback when the consumer cannot fold the gate)
    Val apply_gate(const Val &x, const std::string &why) {
        Val plain = x;
        plain.gate_storage = -1;
        Val out = new_act(x.dims, x.strides_equal(row_major(x.dims)) ? row_major(x.dims) : strides_for_order(x.dims, phys_order(x)));
        Dims gs(x.dims.size(), 0);
        gs[0] = 1;  // gate is [C] along logical dim 0
        emit_elt("se.mul:" + why, out, ref_of(plain), plain.strides, batch_stride(plain), Ref{Space::ARENA, x.gate_storage, 0}, gs,
                 plan_.storages[x.gate_storage].elems, BIN_MUL, ActSpec{});
        return out;
    }
    bool has_input(const OnnxNode &n, size_t idx) const { return idx < n.inputs.size() && !n.inputs[idx].empty(); }
    const Val *opt(const OnnxNode &n, size_t idx) {
        if (!has_input(n, idx)) return nullptr;
        return &get(n, idx);
    }
    // Sole live consumer of tensor `t` (and t is not itself a wanted graph output), else -1.
    int sole_consumer(const std::string &t) {
        if (wanted_names_.count(t)) return -1;
        auto it = consumers_.find(t);
        if (it == consumers_.end()) return -1;
        int found = -1, cnt = 0;
        for (int k : it->second)
            if (!absorbed_[k]) { found = k; cnt++; }
        return cnt == 1 ? found : -1;
    }
    std::vector<int> live_consumers(const std::string &t) {
        std::vector<int> r;
        auto it = consumers_.find(t);
        if (it != consumers_.end())
            for (int k : it->second)
                if (!absorbed_[k]) r.push_back(k);
        return r;
    }
    bool const_scalar(const Val &v, float &out) {
        if (!v.is_const || v.numel() != 1) return false;
        out = v.is_int ? (float)v.i[0] : v.f[0];
        return true;
    }
    std::vector<int64_t> const_ints(const OnnxNode &n, const Val &v) {
        if (!v.is_const) unsupported(n, "expected a constant integer tensor");
        if (v.is_int) return v.i;
        std::vector<int64_t> r(v.f.size());
        for (size_t k = 0; k < r.size(); k++) r[k] = (int64_t)v.f[k];
        return r;
    }

    int32_t new_storage(int64_t elems) {
        Storage s;
        s.elems = elems;
        plan_.storages.push_back(s);
        return (int32_t)plan_.storages.size() - 1;
    }
    Val new_act(const Dims &dims, const Dims &strides) {
        Val v;
        v.dims = dims;
        v.strides = strides;
        v.space = Space::ARENA;
        // storage extent: max offset + 1
        int64_t ext = 1;
        for (size_t k = 0; k < dims.size(); k++) ext += (dims[k] - 1) * std::abs(strides[k]);
        v.storage = new_storage(ext);
        return v;
    }
    int32_t add_const(const std::vector<float> &data) { return bn::add_const(plan_, data); }
    Ref ref_of(const Val &v) const { return Ref{v.space, v.storage, v.offset}; }
    void touch(const Ref &r, int op_index) { bn::touch(plan_, r, op_index); }
    void push_op(PlanOp &&op) { bn::push_op(plan_, std::move(op)); }

    // Physical order of logical dims (outermost first) for an activation.
    static std::vector<int> phys_order(const Val &v) {
        std::vector<int> ord(v.dims.size());
        std::iota(ord.begin(), ord.end(), 0);
        // size-1 dims carry no layout information: treat them as outermost
        auto key = [&](int a) { return v.dims[a] == 1 ? INT64_MAX : std::abs(v.strides[a]); };
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return key(a) > key(b); });
        return ord;
    }
    // Contiguous strides for `dims` laid out in the given physical order.
    static Dims strides_for_order(const Dims &dims, const std::vector<int> &ord) {
        Dims s(dims.size(), 0);
        int64_t acc = 1;
        for (int k = (int)ord.size() - 1; k >= 0; k--) {
            s[ord[k]] = acc;
            acc *= dims[ord[k]];
        }
        return s;
    }

    // Broadcast strides of `v` against out dims (right aligned); const operands are row-major.
    Dims bcast_strides(const OnnxNode *n, const Dims &vdims, const Dims &vstrides, const Dims &out) {
        Dims s(out.size(), 0);
        int off = (int)out.size() - (int)vdims.size();
        if (off < 0) {
            if (n) unsupported(*n, "operand rank exceeds result rank");
            throw UnsupportedModel("broadcast rank mismatch");
        }
        for (size_t k = 0; k < vdims.size(); k++) {
            if (vdims[k] == out[k + off]) s[k + off] = vdims[k] == 1 ? 0 : vstrides[k];
            else if (vdims[k] == 1) s[k + off] = 0;
            else {
                if (n) unsupported(*n, "shapes " + dims_str(vdims) + " and " + dims_str(out) + " do not broadcast");
                throw UnsupportedModel("broadcast mismatch");
            }
        }
        return s;
    }

    // Emit an elementwise op.  sb/b may be empty for unary ops.
    void emit_elt(const std::string &name, const Val &out, const Ref &a, const Dims &sa, int64_t a_bs,
                  const Ref &b, const Dims &sb, int64_t b_bs, int bin, ActSpec act) {
        // iterate in out's physical order
        std::vector<int> ord = phys_order(out);
        struct L { int64_t n, so, sa, sb; };
        std::vector<L> loops;
        for (int d : ord) {
            if (out.dims[d] == 1) continue;
            L l{out.dims[d], out.strides[d], sa[d], sb.empty() ? 0 : sb[d]};
            if (!loops.empty()) {
                L &p = loops.back();
                if (p.so == l.so * l.n && p.sa == l.sa * l.n && p.sb == l.sb * l.n) {
                    p.n *= l.n; p.so = l.so; p.sa = l.sa; p.sb = l.sb;
                    continue;
                }
            }
            loops.push_back(l);
        }
        if (loops.empty()) loops.push_back(L{1, 1, 0, 0});
        if ((int)loops.size() > ELT_MAX_DIMS) throw UnsupportedModel("elementwise op '" + name + "' needs more than 5 loop dims");
        PlanOp op;
        op.kind = OpKind::ELT;
        op.name = name;
        op.r.out = ref_of(out);
        op.r.a = a;
        op.r.chain[0] = b;
        EltDesc &d = op.elt;
        d.nd = (int)loops.size();
        d.per_sample = 1;
        d.nstages = 1;
        EltStage &st = d.st[0];
        for (int k = 0; k < d.nd; k++) {
            d.size[k] = loops[k].n; d.so[k] = loops[k].so; d.sa[k] = loops[k].sa; st.sb[k] = loops[k].sb;
            d.per_sample *= loops[k].n;
        }
        int64_t out_ext = plan_.storages[out.storage].elems;
        d.bo = out_ext; d.ba = a_bs; st.bb = b_bs;
        st.bin = bin; st.act = act.act; st.p0 = act.p0; st.p1 = act.p1;
        op.bytes = 4.0 * (double)d.per_sample * (bin == BIN_NONE ? 2 : 3);
        push_op(std::move(op));
    }
    int64_t batch_stride(const Val &v) const {
        if (v.space == Space::INPUT) return plan_.sample_count;
        if (v.space == Space::ARENA) return plan_.storages[v.storage].elems;
        return 0;
    }

    // Copy `v` into fresh storage with the requested strides.
    Val materialize(const Val &v, const Dims &strides, const std::string &why) {
        Val out = new_act(v.dims, strides);
        emit_elt("copy(" + why + ")", out, ref_of(v), v.strides, batch_stride(v), Ref{}, {}, 0, BIN_NONE, ActSpec{});
        return out;
    }
    Val upload_as_activation(const Val &c) {
        // a constant graph output / concat input: broadcast over the batch via stride 0
        std::vector<float> data = c.is_int ? std::vector<float>(c.i.begin(), c.i.end()) : c.f;
        Dims d = c.dims;
        if (!d.empty() && d[0] == 1) d.erase(d.begin());
        Val out = new_act(d, row_major(d));
        Ref src{Space::CONSTS, add_const(data), 0};
        emit_elt("copy(const)", out, src, row_major(d), 0, Ref{}, {}, 0, BIN_NONE, ActSpec{});
        return out;
    }
    void define(const std::string &name, Val v) { vals_[name] = std::move(v); }

    // --------------------------------------------------------- constant folding
    static bool all_const(const std::vector<const Val *> &vs) {
        for (auto v : vs)
            if (v && !v->is_const) return false;
        return true;
    }
    static Dims bcast_dims(const Dims &a, const Dims &b) {
        size_t r = std::max(a.size(), b.size());
        Dims o(r);
        for (size_t k = 0; k < r; k++) {
            int64_t da = k + a.size() >= r ? a[k + a.size() - r] : 1;
            int64_t db = k + b.size() >= r ? b[k + b.size() - r] : 1;
            if (da != db && da != 1 && db != 1) throw UnsupportedModel("constant broadcast mismatch");
            o[k] = std::max(da, db);
        }
        return o;
    }
    template <class T, class F>
    static std::vector<T> bcast_apply(const Dims &ad, const std::vector<T> &a, const Dims &bd, const std::vector<T> &b,
                                      const Dims &od, F fn) {
        int64_t n = prod(od);
        std::vector<T> o((size_t)n);
        Dims as = row_major(ad), bs = row_major(bd), os = row_major(od);
        for (int64_t lin = 0; lin < n; lin++) {
            int64_t ia = 0, ib = 0, rem = lin;
            for (size_t k = 0; k < od.size(); k++) {
                int64_t idx = rem / os[k];
                rem %= os[k];
                int ka = (int)k - (int)(od.size() - ad.size()), kb = (int)k - (int)(od.size() - bd.size());
                if (ka >= 0 && ad[ka] != 1) ia += idx * as[ka];
                if (kb >= 0 && bd[kb] != 1) ib += idx * bs[kb];
            }
            o[lin] = fn(a[ia], b[ib]);
        }
        return o;
    }
    // (round 5) comparison / boolean operators: 0 / 1 integers on the constant side, f32 0.0 / 1.0 on the device side
    static int compare_code(const std::string &t) {
        return t == "Greater" ? BIN_GT : t == "Less" ? BIN_LT : t == "GreaterOrEqual" ? BIN_GE : t == "LessOrEqual" ? BIN_LE : t == "Equal" ? BIN_EQ
             : t == "Xor" ? BIN_NE : t == "bn.SelA" ? BIN_SELA : t == "bn.SelB" ? BIN_SELB : BIN_NONE;
    }
    bool fold_compare(const OnnxNode &n, const Val &a, const Val &b) {
        const std::string &t = n.op_type;
        const int code = t == "And" ? BIN_MUL : t == "Or" ? BIN_MAX : compare_code(t);
        if (code == BIN_NONE) return false;
        Dims od = bcast_dims(a.dims, b.dims);
        const bool ints = a.is_int && b.is_int;
        auto pick = [code](auto x, auto y) -> decltype(x) {
            using T = decltype(x);
            switch (code) {
                case BIN_GT: return (T)(x > y);
                case BIN_LT: return (T)(x < y);
                case BIN_GE: return (T)(x >= y);
                case BIN_LE: return (T)(x <= y);
                case BIN_EQ: return (T)(x == y);
                case BIN_NE: return (T)(x != y);
                case BIN_MUL: return (T)((x != 0) && (y != 0));
                case BIN_MAX: return (T)((x != 0) || (y != 0));
                case BIN_SELA: return y != 0 ? x : (T)0;
                default: return y != 0 ? (T)0 : x;  // BIN_SELB
            }
        };
        const bool keeps_type = code == BIN_SELA || code == BIN_SELB;  // a select keeps its data operand's type, a comparison yields 0 / 1
        if (ints) {
            define(n.outputs[0], make_const_i(od, bcast_apply<int64_t>(a.dims, a.i, b.dims, b.i, od, [&](int64_t x, int64_t y) { return pick(x, y); })));
            return true;
        }
        std::vector<float> af = a.is_int ? std::vector<float>(a.i.begin(), a.i.end()) : a.f;
        std::vector<float> bf = b.is_int ? std::vector<float>(b.i.begin(), b.i.end()) : b.f;
        std::vector<float> of = bcast_apply<float>(a.dims, af, b.dims, bf, od, [&](float x, float y) { return pick(x, y); });
        if (keeps_type && !a.is_int) define(n.outputs[0], make_const_f(od, of));
        else define(n.outputs[0], make_const_i(od, std::vector<int64_t>(of.begin(), of.end())));
        return true;
    }
    bool fold_binary(const OnnxNode &n, const Val &a, const Val &b) {
        const std::string &t = n.op_type;
        if (fold_compare(n, a, b)) return true;
        Dims od = bcast_dims(a.dims, b.dims);
        if (a.is_int && b.is_int) {
            std::function<int64_t(int64_t, int64_t)> fn;
            if (t == "Add") fn = [](int64_t x, int64_t y) { return x + y; };
            else if (t == "Sub") fn = [](int64_t x, int64_t y) { return x - y; };
            else if (t == "Mul") fn = [](int64_t x, int64_t y) { return (x == BATCH_SENTINEL || y == BATCH_SENTINEL) ? (x == 1 ? y : (y == 1 ? x : BATCH_SENTINEL)) : x * y; };
            else if (t == "Div") fn = [](int64_t x, int64_t y) { return y ? x / y : 0; };
            else if (t == "Max") fn = [](int64_t x, int64_t y) { return std::max(x, y); };
            else if (t == "Min") fn = [](int64_t x, int64_t y) { return std::min(x, y); };
            else return false;
            define(n.outputs[0], make_const_i(od, bcast_apply<int64_t>(a.dims, a.i, b.dims, b.i, od, fn)));
            return true;
        }
        std::vector<float> af = a.is_int ? std::vector<float>(a.i.begin(), a.i.end()) : a.f;
        std::vector<float> bf = b.is_int ? std::vector<float>(b.i.begin(), b.i.end()) : b.f;
        std::function<float(float, float)> fn;
        if (t == "Add") fn = [](float x, float y) { return x + y; };
        else if (t == "Sub") fn = [](float x, float y) { return x - y; };
        else if (t == "Mul") fn = [](float x, float y) { return x * y; };
        else if (t == "Div") fn = [](float x, float y) { return x / y; };
        else if (t == "Pow") fn = [](float x, float y) { return std::pow(x, y); };
        else if (t == "Max") fn = [](float x, float y) { return std::max(x, y); };
        else if (t == "Min") fn = [](float x, float y) { return std::min(x, y); };
        else return false;
        define(n.outputs[0], make_const_f(od, bcast_apply<float>(a.dims, af, b.dims, bf, od, fn)));
        return true;
    }
    bool fold_unary(const OnnxNode &n, const Val &a) {
        const std::string &t = n.op_type;
        std::function<float(float)> fn;
        if (t == "Sqrt") fn = [](float x) { return std::sqrt(x); };
        else if (t == "Exp") fn = [](float x) { return std::exp(x); };
        else if (t == "Log") fn = [](float x) { return std::log(x); };
        else if (t == "Neg") fn = [](float x) { return -x; };
        else if (t == "Abs") fn = [](float x) { return std::fabs(x); };
        else if (t == "Reciprocal") fn = [](float x) { return 1.0f / x; };
        else if (t == "Floor") fn = [](float x) { return std::floor(x); };
        else if (t == "Ceil") fn = [](float x) { return std::ceil(x); };
        else if (t == "Sigmoid") fn = [](float x) { return 1.0f / (1.0f + std::exp(-x)); };
        else if (t == "Relu") fn = [](float x) { return x > 0 ? x : 0.0f; };
        else if (t == "Tanh") fn = [](float x) { return std::tanh(x); };
        else return false;
        if (a.is_int) {
            if (t == "Neg") { std::vector<int64_t> o = a.i; for (auto &x : o) x = -x; define(n.outputs[0], make_const_i(a.dims, o)); return true; }
            if (t == "Abs") { std::vector<int64_t> o = a.i; for (auto &x : o) x = std::llabs(x); define(n.outputs[0], make_const_i(a.dims, o)); return true; }
        }
        std::vector<float> af = a.is_int ? std::vector<float>(a.i.begin(), a.i.end()) : a.f;
        for (auto &x : af) x = fn(x);
        define(n.outputs[0], make_const_f(a.dims, af));
        return true;
    }
    // generic strided gather of a constant: out[idx] = src[offset + sum idx*stride]
    Val const_view(const Val &c, const Dims &dims, const Dims &strides, int64_t offset) {
        Val o; o.is_const = true; o.is_int = c.is_int; o.dims = dims;
        int64_t n = prod(dims);
        Dims os = row_major(dims);
        if (c.is_int) o.i.resize(n); else o.f.resize(n);
        for (int64_t lin = 0; lin < n; lin++) {
            int64_t src = offset, rem = lin;
            for (size_t k = 0; k < dims.size(); k++) { src += (rem / os[k]) * strides[k]; rem %= os[k]; }
            if (c.is_int) o.i[lin] = c.i[src]; else o.f[lin] = c.f[src];
        }
        return o;
    }

    // ------------------------------------------------------------- folded framing convolutions
    // A long single-channel 1-D filter bank whose rows are symmetric (w[n] == w[L-n], windowed cosine bases) or
    // antisymmetric (w[n] == -w[L-n], windowed sine bases) about the frame centre, with w[0] == 0 (Hann-type
    // windows), needs only half the multiplications:
    //     sum_n w[n] x[n] = sum_{n=1}^{L/2-1} w[n] (x[n] +- x[L-n]) + w[L/2] x[L/2]
    // The GEMM stages the folded frame rows (kernels.h, GemmDesc::fold) and K drops from L to L/2.  Rows count as
    // (anti)symmetric when the two halves agree within BN_CONVFOLD_TOL x max|w| (default 2^-23: one unit in the
    // last place of the largest tap -- f32-rounded DFT bases differ from their mirror image by that much in
    // ~1 % of the taps); the first-half taps are the ones kept.  Maximal runs of equal symmetry become one launch
    // each (cos block, sin block), writing column slices of the same output.  BN_CONVFOLD=0 disables.
    bool fold_framing_conv(const OnnxNode &n, const PlanOp &base, const std::vector<float> &wf, int64_t Cout, int64_t L, int64_t OW,
                           bool has_bias) {
        if (sw_is(sw::BN_CONVFOLD, "0")) return false;
        if (L < 128 || L % 64 != 0) return false;  // K = L/2 must be a whole number of 32-wide K steps
        const double tol = sw_double(sw::BN_CONVFOLD_TOL);
        float maxabs = 0.0f;
        for (float v : wf) maxabs = std::max(maxabs, std::fabs(v));
        if (!(maxabs > 0.0f) || !std::isfinite(maxabs)) return false;
        const float eps = (float)(tol * maxabs);
        std::vector<int> cls((size_t)Cout);
        for (int64_t o = 0; o < Cout; o++) {
            const float *w = &wf[(size_t)(o * L)];
            if (!(std::fabs(w[0]) <= eps)) return false;
            bool sym = true, anti = std::fabs(w[L / 2]) <= eps;
            for (int64_t k = 1; k < L / 2 && (sym || anti); k++) {
                if (!(std::fabs(w[k] - w[L - k]) <= eps)) sym = false;
                if (!(std::fabs(w[k] + w[L - k]) <= eps)) anti = false;
            }
            if (!sym && !anti) return false;
            cls[(size_t)o] = (sym && anti) ? 0 : (sym ? 1 : -1);  // 0: an all-zero row joins either neighbour
        }
        {
            DftBank bank;
            if (detect_dft_bank(wf, Cout, L, cls, bank)) {
                if (emit_stft(plan_, n.name, base, bank, Cout, OW, has_bias)) return true;
                if (emit_quarter_fold(plan_, n.name, base, bank, cls, Cout, OW, has_bias)) return true;
            }
        }
        struct Run { int64_t n0, n1; int sign; };
        std::vector<Run> runs;
        for (int64_t o = 0; o < Cout; o++) {
            const int c = cls[(size_t)o];
            if (!runs.empty() && (c == 0 || runs.back().sign == 0 || c == runs.back().sign)) {
                runs.back().n1 = o + 1;
                if (runs.back().sign == 0) runs.back().sign = c;
            } else runs.push_back(Run{o, o + 1, c});
        }
        if (runs.size() > 4) return false;
        plan_.dft_gemm_macs += (double)OW * Cout * L;
        plan_.dft_performed_macs += (double)OW * Cout * (L / 2);  // folded: half the taps
        plan_.dft_fft_equiv_flops += (double)OW * 2.5 * (double)L * std::log2((double)L);  // the same frames as real FFTs (SURVEY 8(d) pricing, any L)
        const int64_t K = L / 2;
        for (const Run &r : runs) {
            const int sign = r.sign == 0 ? 1 : r.sign;
            const int64_t nn = r.n1 - r.n0;
            std::vector<float> wk((size_t)(nn * K));
            for (int64_t o = 0; o < nn; o++) {
                const float *w = &wf[(size_t)((r.n0 + o) * L)];
                for (int64_t c = 0; c + 1 < K; c++) wk[(size_t)(o * K + c)] = w[c + 1];
                wk[(size_t)(o * K + K - 1)] = sign > 0 ? 0.5f * w[K] : 0.0f;  // centre tap: its "pair" is itself
            }
            PlanOp f = base;
            f.name = "Conv:" + n.name + (sign > 0 ? "~sym" : "~anti");
            f.r.out.offset += r.n0;
            if (has_bias) f.r.bias.offset += r.n0;
            f.r.w = Ref{Space::CONSTS, add_const(wk), 0};
            f.gemm.N = (int32_t)nn;
            f.gemm.K = (int32_t)K;
            f.gemm.fold = sign;
            f.gemm.fold_n = (int32_t)L;
            f.macs = (double)OW * nn * K;  // multiplications actually performed
            f.weight_bytes = 4.0 * (wk.size() + (has_bias ? nn : 0));
            f.bytes = base.bytes * (double)nn / (double)Cout;
            push_op(std::move(f));
        }
        return true;
    }

    // ------------------------------------------------------------- lowering
    void lower(const OnnxNode &n) {
        const std::string &t = n.op_type;
        // constant folding first
        std::vector<const Val *> ins;
        for (size_t k = 0; k < n.inputs.size(); k++) ins.push_back(n.inputs[k].empty() ? nullptr : &get(n, k));
        if (t == "Constant") { lower_constant(n); return; }
        if (t == "Shape") { lower_shape(n); return; }
        if (t == "Size") {
            const Val &v = get(n, 0);
            if (!v.is_const) unsupported(n, "Size of an activation depends on the batch size, which a plan does not fix");
            define(n.outputs[0], make_const_i({}, {v.numel()}));
            return;
        }
        bool allc = !ins.empty() && all_const(ins);
        if (allc && try_fold(n, ins)) return;

        if (t == "Identity" || t == "Dropout") { define(n.outputs[0], get(n, 0)); return; }
        if (t == "Cast" && !get(n, 0).is_const) {
            // activations are f32 whatever the graph calls them: a cast between float types is the value itself, a cast to bool is
            // x != 0 -> 1, a cast to an integer type truncates toward zero (ONNX Cast) -- both stay f32 numbers
            const int64_t to = n.attr_i("to", 1);
            if (to == 1 || to == 10 || to == 11 || to == 16) { define(n.outputs[0], get(n, 0)); return; }
            if (to == 9) return lower_unary(n, ActSpec{ACT_NEZ, 0, 0});
            if (to == 2 || to == 3 || to == 4 || to == 5 || to == 6 || to == 7 || to == 12 || to == 13) return lower_unary(n, ActSpec{ACT_TRUNC, 0, 0});
            unsupported(n, "Cast to element type " + std::to_string(to) + " (strings / complex) is outside the native subset");
        }
        if (t == "Not") return lower_unary(n, ActSpec{ACT_AFFINE, -1.0f, 1.0f});  // on a 0 / 1 tensor
        if (t == "And" || t == "Or" || compare_code(t) != BIN_NONE) return lower_binary(n);
        if (t == "Where") return lower_where(n);
        if (t == "Gather" && !get(n, 0).is_const) return lower_gather(n);
        if (t == "DFT") return lower_dft(n);
        if (t == "Transpose") return lower_transpose(n);
        if (t == "Reshape" || t == "Flatten" || t == "Squeeze" || t == "Unsqueeze") return lower_reshape_like(n);
        if (t == "Slice") return lower_slice(n);
        if (t == "Concat") return lower_concat(n);
        if (t == "Pad") return lower_pad(n);
        if (t == "Softmax" || t == "LogSoftmax") return lower_softmax(n);
        if (t == "Split") return lower_split(n);
        if (t == "MaxPool" || t == "AveragePool") return lower_pool(n);
        if (t == "Conv") return lower_conv(n);
        if (t == "MatMul" || t == "Gemm") return lower_matmul(n);
        if (t == "BatchNormalization") return lower_batchnorm(n);
        if (t == "Add" || t == "Sub" || t == "Mul" || t == "Div" || t == "Pow" || t == "Max" || t == "Min") return lower_binary(n);
        if (lower_composite(n)) return;
        if (t == "GlobalAveragePool" || t == "GlobalMaxPool" || t.rfind("Reduce", 0) == 0) return lower_reduce(n);
        if (t == "STFT") return lower_stft(n);
        if (t == "Expand") return lower_expand(n);
        if (t == "Tile") return lower_tile(n);
        if (t == "PRelu") return lower_prelu(n);
        if (t == "InstanceNormalization") return lower_instance_norm(n);
        ActSpec a;
        if (unary_spec(n, a)) return lower_unary(n, a);
        // exporter dialects this path has met but does not map: say what the node is and what to export instead
        if (t == "Resize" || t == "Upsample") unsupported(n, "resampling of feature maps is outside the native subset (no BirdNET / Perch graph needs it)");
        if (t == "Gather" || t == "GatherND" || t == "GatherElements") unsupported(n, "gathers of activations are mapped only where the constant indices are an affine pattern (a strided view: tf.signal.frame's selector)");
        unsupported(n, "operator is outside the native subset");
    }

    // ------------------------------------------------------------- STFT (opset 17)
    // output[b, f, k, 0/1] = Re / Im of sum_n signal[b, f*step + n] * window[n] * exp(-2 pi i k n / N), no padding,
    // k = 0 .. N/2 (onesided, the default) or 0 .. N-1.  That is a 1-D framing convolution with 2*bins filters of N
    // taps and stride `step`: the filters are built here (double-precision cos / sin, rounded once) in the order
    // [all real rows | all imaginary rows], so that the mirror-symmetry fold and the FFT recognition of the framing
    // conv see one cos block and one sin block; the node's [frames, bins, 2] result is a strided VIEW of the conv's
    // channels-last output (no copy).
    void lower_stft(const OnnxNode &n) {
        const Val x = get(n, 0);
        if (x.is_const) unsupported(n, "STFT of a constant signal");
        const Val *stepv = opt(n, 1), *win = opt(n, 2), *flen = opt(n, 3);
        if (!stepv || !stepv->is_const) unsupported(n, "frame_step must be a constant");
        const int64_t step = const_ints(n, *stepv).at(0);
        if (win && !win->is_const) unsupported(n, "window must be a constant");
        if (flen && !flen->is_const) unsupported(n, "frame_length must be a constant");
        int64_t N = flen ? const_ints(n, *flen).at(0) : (win ? win->numel() : 0);
        if (N <= 0 || step <= 0) unsupported(n, "needs a window or a frame_length, and a positive frame_step");
        if (win && (win->is_int || win->numel() != N)) unsupported(n, "window length " + std::to_string(win ? win->numel() : 0) + " differs from frame_length " + std::to_string(N));
        // signal: [L], [L, 1] (real); [L, 2] would be complex
        int64_t L = 0, sL = 0;
        if (x.dims.size() == 1) { L = x.dims[0]; sL = x.strides[0]; }
        else if (x.dims.size() == 2 && x.dims[1] == 1) { L = x.dims[0]; sL = x.strides[0]; }
        else unsupported(n, "signal must be real: [batch, length] or [batch, length, 1], got per-sample dims " + dims_str(x.dims));
        if (L < N) unsupported(n, "signal shorter than one frame");
        const bool onesided = n.attr_i("onesided", 1) != 0;
        const int64_t bins = onesided ? N / 2 + 1 : N;
        if (N * 2 * bins > ((int64_t)1 << 28)) unsupported(n, "DFT basis too large");
        Val w;
        w.is_const = true;
        w.dims = {2 * bins, 1, N};
        w.f.resize((size_t)(2 * bins * N));
        for (int64_t k = 0; k < bins; k++)
            for (int64_t t = 0; t < N; t++) {
                const double wv = win ? (double)win->f[(size_t)t] : 1.0;
                const double th = 2.0 * M_PI * (double)((k * t) % N) / (double)N;
                w.f[(size_t)(k * N + t)] = (float)(wv * std::cos(th));
                w.f[(size_t)((bins + k) * N + t)] = (float)(-wv * std::sin(th));
            }
        const std::string base = "stft:" + (n.name.empty() ? n.outputs[0] : n.name);
        Val xv = x;
        xv.dims = {1, L};
        xv.strides = {L * sL, sL};
        vals_[base + "/signal"] = xv;
        vals_[base + "/basis"] = std::move(w);
        OnnxNode conv;
        conv.name = base;
        conv.op_type = "Conv";
        conv.inputs = {base + "/signal", base + "/basis"};
        conv.outputs = {base + "/frames"};
        OnnxAttr st;
        st.name = "strides";
        st.type = 7;
        st.ints = {step};
        conv.attrs["strides"] = st;
        lower_conv(conv);
        auto yit = vals_.find(base + "/frames");
        if (yit == vals_.end()) unsupported(n, "internal: the framing conv defined no output");
        const Val y = yit->second;
        if (y.is_const || y.dims.size() != 2 || y.dims[0] != 2 * bins) unsupported(n, "internal: framing conv produced " + dims_str(y.dims));
        Val out = y;
        out.dims = {y.dims[1], bins, 2};
        out.strides = {y.strides[1], y.strides[0], bins * y.strides[0]};
        define(n.outputs[0], out);
    }

    // ---- operators lowered as short sequences of operators the planner already has (each step is an ordinary node to
    // the lowering: constants fold, elementwise steps fuse into chains)
    std::string synth_const(const std::string &name, Dims dims, std::vector<float> f) {
        Val c;
        c.is_const = true;
        c.dims = std::move(dims);
        c.f = std::move(f);
        vals_[name] = std::move(c);
        return name;
    }
    static void set_int(OnnxNode &nd, const std::string &key, int64_t v) {
        OnnxAttr a;
        a.name = key;
        a.type = 2;
        a.i = v;
        nd.attrs[key] = a;
    }

    // Operators written out as the operators above (round 5): the pieces go through the elementwise / reduction lowering, so they fuse into
    // their neighbours like hand-written graphs of the same arithmetic.  ONNX defines each of these by exactly this formula.
    bool lower_composite(const OnnxNode &n) {
        const std::string &t = n.op_type;
        if (n.outputs.empty() || n.inputs.empty()) return false;
        const std::string base = "cmp:" + n.outputs[0];
        const std::string &x = n.inputs[0];
        int seq = 0;
        auto step = [&](const char *op, std::vector<std::string> ins, bool last = false) {
            const std::string out = last ? n.outputs[0] : base + "/" + std::to_string(seq);
            lower(synth_node(op, last ? n.name : n.name + "/" + std::to_string(seq), std::move(ins), out));
            seq++;
            return out;
        };
        auto k = [&](float v) { return synth_const(base + "/c" + std::to_string(seq++), {1}, {v}); };
        auto reduce = [&](const char *op, const std::string &in, bool last) {
            const std::string out = last ? n.outputs[0] : base + "/" + std::to_string(seq);
            OnnxNode r = synth_node(op, last ? n.name : n.name + "/" + std::to_string(seq), {in}, out);
            seq++;
            if (n.has("axes")) set_ints(r, "axes", n.attr_ints("axes"));
            else if (has_input(n, 1)) r.inputs.push_back(n.inputs[1]);
            set_int(r, "keepdims", n.attr_i("keepdims", 1));
            if (n.has("noop_with_empty_axes")) set_int(r, "noop_with_empty_axes", n.attr_i("noop_with_empty_axes", 0));
            lower(r);
            return out;
        };
        if (t == "Elu" || t == "Selu" || t == "Celu") {
            // max(x, 0) + alpha (exp(min(x, 0) / a) - 1), a = alpha for Celu and 1 otherwise; Selu scales the sum by gamma
            const float alpha = n.attr_f("alpha", t == "Selu" ? 1.67326319217681884765625f : 1.0f);
            const float gamma = t == "Selu" ? n.attr_f("gamma", 1.05070102214813232421875f) : 1.0f;
            std::string neg = step("Min", {x, k(0.0f)});
            if (t == "Celu") neg = step("Div", {neg, k(alpha)});
            neg = step("Exp", {neg});
            neg = step("Mul", {neg, k(alpha * gamma)});
            neg = step("Sub", {neg, k(alpha * gamma)});
            std::string pos = step("Relu", {x});
            if (gamma != 1.0f) pos = step("Mul", {pos, k(gamma)});
            step("Add", {pos, neg}, true);
            return true;
        }
        if (t == "ThresholdedRelu") {
            const std::string m = step("Greater", {x, k(n.attr_f("alpha", 1.0f))});
            step("Where", {m, x, k(0.0f)}, true);
            return true;
        }
        if (t == "Softsign") {
            std::string d = step("Abs", {x});
            d = step("Add", {d, k(1.0f)});
            step("Div", {x, d}, true);
            return true;
        }
        if (t == "Mish") {
            std::string d = step("Softplus", {x});
            d = step("Tanh", {d});
            step("Mul", {x, d}, true);
            return true;
        }
        if (t == "Gelu") {
            std::string g;
            if (n.attr_s("approximate", "none") == "tanh") {
                g = step("Mul", {x, x});
                g = step("Mul", {g, x});
                g = step("Mul", {g, k(0.044715f)});
                g = step("Add", {g, x});
                g = step("Mul", {g, k(0.797884583473205566406250f)});
                g = step("Tanh", {g});
            } else {
                g = step("Mul", {x, k(0.707106769084930419921875f)});
                g = step("Erf", {g});
            }
            g = step("Mul", {g, k(0.5f)});
            g = step("Add", {g, k(0.5f)});
            step("Mul", {x, g}, true);
            return true;
        }
        if (t == "Sign") {
            const std::string p = step("Greater", {x, k(0.0f)}), m = step("Less", {x, k(0.0f)});
            step("Sub", {p, m}, true);
            return true;
        }
        if (t == "Sum" || t == "Mean") {
            std::string acc = x;
            const size_t cnt = n.inputs.size();
            if (cnt == 1) { lower(synth_node("Identity", n.name, {x}, n.outputs[0])); return true; }
            for (size_t j = 1; j < cnt; j++) acc = step("Add", {acc, n.inputs[j]}, t == "Sum" && j + 1 == cnt);
            if (t == "Mean") step("Div", {acc, k((float)cnt)}, true);
            return true;
        }
        if (t == "ReduceL1") {
            reduce("ReduceSum", step("Abs", {x}), true);
            return true;
        }
        if (t == "ReduceLogSum") {
            step("Log", {reduce("ReduceSum", x, false)}, true);
            return true;
        }
        if (t == "ReduceLogSumExp") {
            // log(sum(exp(x - m))) + m with m the maximum over the same axes: the form that cannot overflow (what ORT computes)
            OnnxNode mx = synth_node("ReduceMax", n.name + "/max", {x}, base + "/max");
            if (n.has("axes")) set_ints(mx, "axes", n.attr_ints("axes"));
            else if (has_input(n, 1)) mx.inputs.push_back(n.inputs[1]);
            set_int(mx, "keepdims", 1);
            lower(mx);
            std::string e = step("Sub", {x, base + "/max"});
            e = step("Exp", {e});
            e = reduce("ReduceSum", e, false);
            e = step("Log", {e});
            std::string m = base + "/max";
            if (n.attr_i("keepdims", 1) == 0) {
                OnnxNode m2 = synth_node("ReduceMax", n.name + "/max0", {x}, base + "/max0");
                if (n.has("axes")) set_ints(m2, "axes", n.attr_ints("axes"));
                else if (has_input(n, 1)) m2.inputs.push_back(n.inputs[1]);
                set_int(m2, "keepdims", 0);
                lower(m2);
                m = base + "/max0";
            }
            step("Add", {e, m}, true);
            return true;
        }
        if (t == "LayerNormalization") {
            // over the dimensions from `axis` to the last: (x - mean) / sqrt(var + eps) * Scale + B; the optional Mean / InvStdDev outputs
            // are training-side and not produced here
            if (n.outputs.size() > 1 && (!n.outputs[1].empty() || (n.outputs.size() > 2 && !n.outputs[2].empty())))
                unsupported(n, "the Mean / InvStdDev outputs of LayerNormalization are not produced");
            const Val &xv = get(n, 0);
            if (xv.is_const) return false;
            const int64_t r = (int64_t)xv.dims.size() + 1;
            int64_t axis = n.attr_i("axis", -1);
            if (axis < 0) axis += r;
            if (axis <= 0 || axis >= r) unsupported(n, "LayerNormalization over the batch dimension");
            std::vector<int64_t> axes;
            for (int64_t a = axis; a < r; a++) axes.push_back(a);
            auto mean_of = [&](const std::string &in) {
                const std::string out = base + "/" + std::to_string(seq);
                OnnxNode m = synth_node("ReduceMean", n.name + "/" + std::to_string(seq), {in}, out);
                seq++;
                set_ints(m, "axes", axes);
                set_int(m, "keepdims", 1);
                lower(m);
                return out;
            };
            const std::string d = step("Sub", {x, mean_of(x)});
            std::string v = mean_of(step("Mul", {d, d}));
            v = step("Add", {v, k(n.attr_f("epsilon", 1e-5f))});
            v = step("Sqrt", {v});
            v = step("Div", {d, v});
            const bool has_b = has_input(n, 2);
            v = step("Mul", {v, n.inputs[1]}, !has_b);
            if (has_b) step("Add", {v, n.inputs[2]}, true);
            return true;
        }
        return false;
    }

    // PRelu(x, slope) = max(x, 0) + slope * min(x, 0); one slope for everything is LeakyRelu
    void lower_prelu(const OnnxNode &n) {
        const Val *sl = opt(n, 1);
        if (!sl || !sl->is_const || sl->is_int) unsupported(n, "PRelu needs a constant slope");
        const std::string base = "prelu:" + n.outputs[0];
        if (sl->numel() == 1) {
            OnnxNode lr = synth_node("LeakyRelu", n.name, {n.inputs[0]}, n.outputs[0]);
            OnnxAttr a;
            a.name = "alpha";
            a.type = 1;
            a.f = sl->f[0];
            lr.attrs["alpha"] = a;
            lower(lr);
            return;
        }
        lower(synth_node("Relu", n.name + "/pos", {n.inputs[0]}, base + "/pos"));
        lower(synth_node("Min", n.name + "/neg", {n.inputs[0], synth_const(base + "/zero", {1}, {0.0f})}, base + "/neg"));
        lower(synth_node("Mul", n.name + "/scaled", {base + "/neg", n.inputs[1]}, base + "/scaled"));
        lower(synth_node("Add", n.name, {base + "/pos", base + "/scaled"}, n.outputs[0]));
    }

    // Tile: only repeats of dimensions of size 1 (= Expand); anything else would need a gather
    void lower_tile(const OnnxNode &n) {
        const Val &x = get(n, 0);
        const Val *rp = opt(n, 1);
        if (!rp || !rp->is_const) unsupported(n, "Tile needs constant repeats");
        std::vector<int64_t> rep = const_ints(n, *rp);
        Dims full = x.dims;
        if (!x.is_const) full.insert(full.begin(), 1);  // the batch dimension: repeats[0] must be 1
        if (rep.size() != full.size()) unsupported(n, "repeats must have one entry per dimension");
        std::vector<int64_t> target(full.size());
        for (size_t k = 0; k < full.size(); k++) {
            if (rep[k] != 1 && full[k] != 1) unsupported(n, "Tile repeats a dimension of size " + std::to_string(full[k]) + " (only size-1 dimensions, i.e. broadcasts, are mapped)");
            if (k == 0 && !x.is_const && rep[k] != 1) unsupported(n, "Tile along the batch dimension");
            target[k] = full[k] * rep[k];
        }
        const std::string sname = "tile:" + n.outputs[0] + "/shape";
        Val sh = make_const_i({(int64_t)target.size()}, target);
        vals_[sname] = sh;
        lower_expand(synth_node("Expand", n.name, {n.inputs[0], sname}, n.outputs[0]));
    }

    // InstanceNormalization: per (sample, channel) over the spatial dimensions, (x - mean) / sqrt(var + eps) * scale + B
    void lower_instance_norm(const OnnxNode &n) {
        const Val &x = get(n, 0);
        const Val *sc = opt(n, 1), *bi = opt(n, 2);
        if (x.is_const || !sc || !bi || !sc->is_const || !bi->is_const) unsupported(n, "InstanceNormalization needs an activation input and constant scale / B");
        const size_t r = x.dims.size();  // per-sample rank: [C, spatial...]
        if (r < 2 || sc->numel() != x.dims[0] || bi->numel() != x.dims[0]) unsupported(n, "scale / B must have one entry per channel");
        const std::string base = "inorm:" + n.outputs[0];
        std::vector<int64_t> axes;
        for (size_t k = 2; k <= r; k++) axes.push_back((int64_t)k);
        Dims cdims(r, 1);
        cdims[0] = x.dims[0];
        auto mean_of = [&](const std::string &in, const std::string &out, const std::string &nm) {
            OnnxNode m = synth_node("ReduceMean", nm, {in}, out);
            set_ints(m, "axes", axes);
            set_int(m, "keepdims", 1);
            lower(m);
        };
        mean_of(n.inputs[0], base + "/mean", n.name + "/mean");
        lower(synth_node("Sub", n.name + "/centred", {n.inputs[0], base + "/mean"}, base + "/d"));
        lower(synth_node("Mul", n.name + "/sq", {base + "/d", base + "/d"}, base + "/sq"));
        mean_of(base + "/sq", base + "/var", n.name + "/var");
        lower(synth_node("Add", n.name + "/eps", {base + "/var", synth_const(base + "/epsc", {1}, {n.attr_f("epsilon", 1e-5f)})}, base + "/ve"));
        lower(synth_node("Sqrt", n.name + "/std", {base + "/ve"}, base + "/std"));
        lower(synth_node("Div", n.name + "/norm", {base + "/d", base + "/std"}, base + "/norm"));
        lower(synth_node("Mul", n.name + "/scale", {base + "/norm", synth_const(base + "/scalec", cdims, sc->f)}, base + "/scaled"));
        lower(synth_node("Add", n.name, {base + "/scaled", synth_const(base + "/biasc", cdims, bi->f)}, n.outputs[0]));
    }

    // Expand(x, shape): x * ones(broadcast shape) -- exact for every float including -0, infinities and NaN payloads
    // that survive a multiplication by 1; goes through the elementwise lowering, so it fuses into its neighbours.
    void lower_expand(const OnnxNode &n) {
        const Val &x = get(n, 0);
        const Val *shp = opt(n, 1);
        if (!shp || !shp->is_const) unsupported(n, "Expand needs a constant shape");
        std::vector<int64_t> target = const_ints(n, *shp);
        Dims full = x.dims;
        if (!x.is_const) full.insert(full.begin(), BATCH_SENTINEL);
        while (full.size() < target.size()) full.insert(full.begin(), 1);
        while (target.size() < full.size()) target.insert(target.begin(), 1);
        Dims ones_dims;
        for (size_t k = 0; k < full.size(); k++) {
            int64_t tdim = target[k], xdim = full[k];
            if (xdim == BATCH_SENTINEL || tdim == BATCH_SENTINEL) {
                if (k != 0 || (xdim != BATCH_SENTINEL && xdim != 1) || (tdim != BATCH_SENTINEL && tdim != 1))
                    unsupported(n, "Expand may only keep the batch dimension as it is");
                continue;  // the batch dimension is not part of the ones operand
            }
            if (tdim != 1 && xdim != 1 && tdim != xdim) unsupported(n, "shape " + dims_str(target) + " does not broadcast with " + dims_str(full));
            ones_dims.push_back(std::max(tdim, xdim));
        }
        if (!x.is_const && full.size() != x.dims.size() + 1) unsupported(n, "Expand would add dimensions in front of the batch");
        if (prod(ones_dims) > ((int64_t)1 << 28)) unsupported(n, "Expand target too large");
        Val ones;
        ones.is_const = true;
        ones.dims = ones_dims;
        ones.f.assign((size_t)prod(ones_dims), 1.0f);
        if (x.is_const && x.is_int) unsupported(n, "Expand of an integer constant");
        const std::string oname = "expand:" + n.outputs[0] + "/ones";
        vals_[oname] = std::move(ones);
        OnnxNode mul;
        mul.name = n.name.empty() ? "expand:" + n.outputs[0] : n.name;
        mul.op_type = "Mul";
        mul.inputs = {n.inputs[0], oname};
        mul.outputs = {n.outputs[0]};
        lower(mul);
    }

    void lower_constant(const OnnxNode &n) {
        auto it = n.attrs.find("value");
        if (it != n.attrs.end()) {
            const OnnxTensor &t = it->second.t;
            define(n.outputs[0], t.is_float() ? make_const_f(t.dims, t.f) : make_const_i(t.dims, t.i));
        } else if (n.has("value_float")) define(n.outputs[0], make_const_f({}, {n.attr_f("value_float", 0)}));
        else if (n.has("value_int")) define(n.outputs[0], make_const_i({}, {n.attr_i("value_int", 0)}));
        else if (n.has("value_ints")) { auto v = n.attr_ints("value_ints"); define(n.outputs[0], make_const_i({(int64_t)v.size()}, v)); }
        else if (n.has("value_floats")) { auto v = n.attrs.at("value_floats").floats; define(n.outputs[0], make_const_f({(int64_t)v.size()}, v)); }
        else unsupported(n, "Constant without a supported value attribute");
    }
    void lower_shape(const OnnxNode &n) {
        const Val &v = get(n, 0);
        std::vector<int64_t> s;
        if (v.is_const) s = v.dims;
        else { s.push_back(BATCH_SENTINEL); s.insert(s.end(), v.dims.begin(), v.dims.end()); }
        define(n.outputs[0], make_const_i({(int64_t)s.size()}, s));
    }

    bool try_fold(const OnnxNode &n, const std::vector<const Val *> &ins) {
        const std::string &t = n.op_type;
        const Val &a = *ins[0];
        if (ins.size() >= 2 && ins[1] && (t == "Add" || t == "Sub" || t == "Mul" || t == "Div" || t == "Pow" || t == "Max" || t == "Min" ||
                                          t == "And" || t == "Or" || compare_code(t) != BIN_NONE))
            return fold_binary(n, a, *ins[1]);
        if (t == "Not") {
            std::vector<int64_t> o(a.is_int ? a.i.size() : a.f.size());
            for (size_t k = 0; k < o.size(); k++) o[k] = a.is_int ? a.i[k] == 0 : a.f[k] == 0.0f;
            define(n.outputs[0], make_const_i(a.dims, o));
            return true;
        }
        if (t == "Where" && ins.size() == 3 && ins[1] && ins[2]) {
            // Where(cond, x, y) on constants (the exporters' shape arithmetic: Where(Equal(shape, -1), ...)): SelA(x, cond) + SelB(y, cond)
            const std::string base = "where:" + n.outputs[0];
            lower(synth_node("bn.SelA", n.name + "/x", {n.inputs[1], n.inputs[0]}, base + "/x"));
            lower(synth_node("bn.SelB", n.name + "/y", {n.inputs[2], n.inputs[0]}, base + "/y"));
            lower(synth_node("Add", n.name, {base + "/x", base + "/y"}, n.outputs[0]));
            return true;
        }
        if (t == "Identity") { define(n.outputs[0], a); return true; }
        if (t == "Cast") {
            int64_t to = n.attr_i("to", 1);
            Val o = a;
            if (to == 1 || to == 11 || to == 10) { if (a.is_int) { o.is_int = false; o.f.assign(a.i.begin(), a.i.end()); o.i.clear(); } }
            else { if (!a.is_int) { o.is_int = true; o.i.resize(a.f.size()); for (size_t k = 0; k < a.f.size(); k++) o.i[k] = (int64_t)a.f[k]; o.f.clear(); } }
            define(n.outputs[0], o);
            return true;
        }
        if (t == "Unsqueeze" || t == "Squeeze" || t == "Reshape" || t == "Flatten") {
            Dims nd = reshape_target(n, a.dims, /*is_const=*/true);
            Val o = a; o.dims = nd;
            define(n.outputs[0], o);
            return true;
        }
        if (t == "Transpose") {
            auto perm = n.attr_ints("perm");
            size_t r = a.dims.size();
            if (perm.empty()) for (size_t k = 0; k < r; k++) perm.push_back((int64_t)(r - 1 - k));
            Dims rs = row_major(a.dims), nd(r), ns(r);
            for (size_t k = 0; k < r; k++) { nd[k] = a.dims[perm[k]]; ns[k] = rs[perm[k]]; }
            define(n.outputs[0], const_view(a, nd, ns, 0));
            return true;
        }
        if (t == "Concat") {
            int64_t axis = n.attr_i("axis", 0);
            size_t r = a.dims.size();
            if (axis < 0) axis += (int64_t)r;
            Dims od = a.dims;
            od[axis] = 0;
            for (auto v : ins) od[axis] += v->dims[axis];
            int64_t outer = 1, inner = 1;
            for (int64_t k = 0; k < axis; k++) outer *= od[k];
            for (size_t k = axis + 1; k < r; k++) inner *= od[k];
            Val o; o.is_const = true; o.is_int = a.is_int; o.dims = od;
            for (int64_t ou = 0; ou < outer; ou++)
                for (auto v : ins) {
                    int64_t chunk = v->dims[axis] * inner;
                    for (int64_t e = 0; e < chunk; e++) {
                        if (o.is_int) o.i.push_back(v->is_int ? v->i[ou * chunk + e] : (int64_t)v->f[ou * chunk + e]);
                        else o.f.push_back(v->is_int ? (float)v->i[ou * chunk + e] : v->f[ou * chunk + e]);
                    }
                }
            define(n.outputs[0], o);
            return true;
        }
        if (t == "Gather") {
            int64_t axis = n.attr_i("axis", 0);
            const Val &idx = *ins[1];
            if (axis < 0) axis += (int64_t)a.dims.size();
            if (axis != 0 || a.dims.size() != 1) return false;
            auto ids = const_ints(n, idx);
            Val o; o.is_const = true; o.is_int = a.is_int; o.dims = idx.dims;
            for (auto id : ids) {
                if (id < 0) id += a.dims[0];
                if (a.is_int) o.i.push_back(a.i[id]); else o.f.push_back(a.f[id]);
            }
            define(n.outputs[0], o);
            return true;
        }
        if (t == "Slice") {
            Dims nd, ns; int64_t off;
            slice_params(n, a.dims, row_major(a.dims), nd, ns, off, /*batched=*/false);
            define(n.outputs[0], const_view(a, nd, ns, off));
            return true;
        }
        if (t == "ConstantOfShape") {
            auto shape = const_ints(n, a);
            float fv = 0; bool isint = false; int64_t iv = 0;
            auto it = n.attrs.find("value");
            if (it != n.attrs.end()) { if (it->second.t.is_float()) fv = it->second.t.f[0]; else { isint = true; iv = it->second.t.i[0]; } }
            for (auto d : shape) if (d < 0) return false;
            if (isint) define(n.outputs[0], make_const_i(shape, std::vector<int64_t>(prod(shape), iv)));
            else define(n.outputs[0], make_const_f(shape, std::vector<float>(prod(shape), fv)));
            return true;
        }
        if (t == "Range") {
            if (!a.is_int) return false;
            int64_t s = a.i[0], e = ins[1]->i[0], d = ins[2]->i[0];
            std::vector<int64_t> r;
            for (int64_t x = s; d > 0 ? x < e : x > e; x += d) r.push_back(x);
            define(n.outputs[0], make_const_i({(int64_t)r.size()}, r));
            return true;
        }
        return fold_unary(n, a);
    }

    // Target dims for Reshape/Flatten/Squeeze/Unsqueeze.  For activations `dims`
    // is per-sample and ONNX axes/shapes include the batch at position 0.
    Dims reshape_target(const OnnxNode &n, const Dims &dims, bool is_const) {
        const std::string &t = n.op_type;
        Dims full = dims;
        if (!is_const) full.insert(full.begin(), BATCH_SENTINEL);
        Dims out;
        auto axes_of = [&](size_t input_idx) {
            std::vector<int64_t> ax = n.attr_ints("axes");
            if (ax.empty() && has_input(n, input_idx)) ax = const_ints(n, get(n, input_idx));
            return ax;
        };
        if (t == "Flatten") {
            int64_t axis = n.attr_i("axis", 1);
            int64_t r = (int64_t)full.size();
            if (axis < 0) axis += r;
            if (!is_const && axis != 1) unsupported(n, "Flatten must keep the batch as the leading dimension (axis=1)");
            int64_t a = 1, b = 1;
            for (int64_t k = 0; k < axis; k++) a *= full[k];
            for (int64_t k = axis; k < r; k++) b *= full[k];
            out = is_const ? Dims{a, b} : Dims{BATCH_SENTINEL, b};
        } else if (t == "Squeeze") {
            auto ax = axes_of(1);
            int64_t r = (int64_t)full.size();
            std::set<int64_t> drop;
            if (ax.empty()) { for (int64_t k = 0; k < r; k++) if (full[k] == 1) drop.insert(k); }
            else for (auto a : ax) drop.insert(a < 0 ? a + r : a);
            for (int64_t k = 0; k < r; k++) {
                if (drop.count(k)) { if (full[k] != 1) unsupported(n, "cannot squeeze a dimension of size " + std::to_string(full[k])); }
                else out.push_back(full[k]);
            }
        } else if (t == "Unsqueeze") {
            auto ax = axes_of(1);
            int64_t r = (int64_t)full.size() + (int64_t)ax.size();
            std::set<int64_t> ins;
            for (auto a : ax) ins.insert(a < 0 ? a + r : a);
            size_t src = 0;
            for (int64_t k = 0; k < r; k++) {
                if (ins.count(k)) out.push_back(1);
                else out.push_back(full[src++]);
            }
        } else {  // Reshape
            auto shape = const_ints(n, get(n, 1));
            bool allowzero = n.attr_i("allowzero", 0) != 0;
            int64_t known = 1, total = 1;
            int infer = -1;
            bool batch_in_total = false;
            for (auto d : full) { if (d == BATCH_SENTINEL) batch_in_total = true; else total *= d; }
            bool batch_in_out = false;
            for (size_t k = 0; k < shape.size(); k++) {
                int64_t d = shape[k];
                if (d == 0 && !allowzero) d = k < full.size() ? full[k] : 0;
                if (d == -1) { infer = (int)k; out.push_back(-1); continue; }
                if (d == BATCH_SENTINEL) batch_in_out = true;
                else known *= d;
                out.push_back(d);
            }
            if (!is_const && batch_in_total && !batch_in_out) {
                // The exporter wrote the batch as a literal (1 for a batch-1 trace) or as -1.
                if (infer == 0) { out[0] = BATCH_SENTINEL; infer = -1; }
                else if (!out.empty() && out[0] == 1 && (infer >= 0 || known == total)) out[0] = BATCH_SENTINEL;
                else unsupported(n, "Reshape target " + dims_str(shape) + " does not keep the batch dimension leading");
            }
            if (infer >= 0) {
                if (known == 0 || total % known) unsupported(n, "Reshape cannot infer -1");
                out[infer] = total / known;
            }
        }
        if (!is_const) {
            if (out.empty() || out[0] != BATCH_SENTINEL) unsupported(n, "result does not keep the batch as the leading dimension");
            out.erase(out.begin());
            for (auto d : out) if (d == BATCH_SENTINEL || d < 0) unsupported(n, "batch dimension used in a non-leading position");
            if (prod(out) != prod(dims)) unsupported(n, "element count changes from " + dims_str(dims) + " to " + dims_str(out));
        }
        return out;
    }

    void lower_reshape_like(const OnnxNode &n) {
        const Val &v = get(n, 0);
        Dims nd = reshape_target(n, v.dims, false);
        // view if the non-unit dims are unchanged, else require row-major contiguity
        Dims a, as, b;
        for (size_t k = 0; k < v.dims.size(); k++) if (v.dims[k] != 1) { a.push_back(v.dims[k]); as.push_back(v.strides[k]); }
        for (auto d : nd) if (d != 1) b.push_back(d);
        Val o = v;
        o.dims = nd;
        Dims vs;
        if (a == b) {
            o.strides.assign(nd.size(), 0);
            size_t j = 0;
            for (size_t k = 0; k < nd.size(); k++) if (nd[k] != 1) o.strides[k] = as[j++];
        } else if (!v.win_name.empty()) {
            vals_[n.inputs[0]] = apply_window(v, n.inputs[0]);  // (the non-unit dims change: the window's axis would be lost)
            return lower_reshape_like(n);
        } else if (view_reshape(a, as, nd, vs)) {
            o.strides = vs;  // (round 5) dims that merge / split without moving an element: tf.signal.frame's [frames, L / sub, sub] -> [frames, L]
        } else {
            Val src = v.contiguous() ? v : materialize(v, row_major(v.dims), n.name);
            o = src;
            o.dims = nd;
            o.strides = row_major(nd);
        }
        define(n.outputs[0], o);
    }

    // Strides of `nd` over the same elements as the (non-unit) dims `a` with strides `as`, if one exists without a copy: the old dims are
    // cut into maximal runs that are contiguous among themselves (stride[k] == dims[k+1] * stride[k+1]); every new non-unit dim must
    // fall inside one run (row-major inside it).  The usual no-copy reshape rule.
    static bool view_reshape(const Dims &a, const Dims &as, const Dims &nd, Dims &out) {
        out.assign(nd.size(), 0);
        size_t i = 0, j = 0;
        while (j < nd.size() && nd[j] == 1) j++;
        while (i < a.size() && j < nd.size()) {
            // old run [i, e): contiguous among themselves
            size_t e = i + 1;
            int64_t run = a[i];
            // extend the new side until the products match, extending the old run when the new product overshoots
            size_t j0 = j;
            int64_t np = nd[j];
            size_t je = j + 1;
            while (np != run) {
                if (np < run) {
                    while (je < nd.size() && nd[je] == 1) je++;
                    if (je >= nd.size()) return false;
                    np *= nd[je++];
                } else {
                    if (e >= a.size() || as[e - 1] != a[e] * as[e]) return false;
                    run *= a[e++];
                }
            }
            // strides of the new dims inside the run: row-major, innermost = the run's last old stride
            int64_t st = as[e - 1];
            for (size_t k = je; k-- > j0;) {
                if (nd[k] == 1) continue;
                out[k] = st;
                st *= nd[k];
            }
            i = e;
            j = je;
            while (j < nd.size() && nd[j] == 1) j++;
        }
        return i == a.size() && j == nd.size();
    }

    // Gather of an activation with CONSTANT indices that form an affine pattern idx[i0, i1, ...] = base + sum_k i_k * step_k: a strided
    // view, no copy.  This is what framing looks like in a TensorFlow export (tf.signal.frame gathers sub-frames with the selector
    // frame * (hop / sub) + j); anything that is not affine is refused.
    void lower_gather(const OnnxNode &n) {
        const Val &x = get(n, 0);
        const Val &iv = get(n, 1);
        if (x.is_const || !iv.is_const) unsupported(n, "Gather is mapped for an activation with constant indices only");
        int64_t axis = n.attr_i("axis", 0);
        const int64_t r = (int64_t)x.dims.size() + 1;
        if (axis < 0) axis += r;
        if (axis <= 0 || axis >= r) unsupported(n, "Gather along the batch dimension");
        axis -= 1;
        const int64_t D = x.dims[axis];
        std::vector<int64_t> idx = const_ints(n, iv);
        for (auto &v : idx) { if (v < 0) v += D; if (v < 0 || v >= D) unsupported(n, "Gather index out of range"); }
        const Dims &id = iv.dims;
        Dims irs = row_major(id), step(id.size(), 0);
        const int64_t base = idx.empty() ? 0 : idx[0];
        for (size_t k = 0; k < id.size(); k++) step[k] = id[k] > 1 ? idx[(size_t)irs[k]] - base : 0;
        for (size_t lin = 0; lin < idx.size(); lin++) {
            int64_t want = base, rem = (int64_t)lin;
            for (size_t k = 0; k < id.size(); k++) { want += (rem / irs[k]) * step[k]; rem %= irs[k]; }
            if (idx[lin] != want) unsupported(n, "Gather indices are not an affine pattern (only strided views of an activation are mapped; tf.signal.frame's selector is one)");
        }
        Val o = x;
        o.dims.assign(x.dims.begin(), x.dims.begin() + axis);
        o.strides.assign(x.strides.begin(), x.strides.begin() + axis);
        for (size_t k = 0; k < id.size(); k++) { o.dims.push_back(id[k]); o.strides.push_back(step[k] * x.strides[axis]); }
        o.dims.insert(o.dims.end(), x.dims.begin() + axis + 1, x.dims.end());
        o.strides.insert(o.strides.end(), x.strides.begin() + axis + 1, x.strides.end());
        o.offset = x.offset + base * x.strides[axis];
        define(n.outputs[0], o);
    }

    // Mul(frames, window[L]) whose result reaches a DFT node through nothing but unit-dimension reshapes: leave the window pending on the
    // value -- lower_dft folds it into its basis, which is what lets the framing kernels (mirror / quarter fold, FFT) recognise the bank
    bool try_pending_window(const OnnxNode &n, const Val &a, const Val &b) {
        const Val &x = a.is_const ? b : a, &w = a.is_const ? a : b;
        if (x.is_const || !w.is_const || w.is_int || !x.win_name.empty() || x.gate_storage >= 0 || wanted_names_.count(n.outputs[0])) return false;
        const int64_t L = w.numel();
        if (L < 2) return false;
        // the window's one non-unit dim, aligned from the right against the full (batched) dims of x
        int wax = -1;
        for (size_t k = 0; k < w.dims.size(); k++)
            if (w.dims[k] != 1) { if (wax >= 0) return false; wax = (int)k; }
        const int ax = wax + (int)(x.dims.size() + 1) - (int)w.dims.size() - 1;  // per-sample axis of x
        if (ax < 0 || ax >= (int)x.dims.size() || x.dims[ax] != L) return false;
        std::string cur = n.outputs[0];
        for (int hop = 0; hop < 4; hop++) {
            int c = sole_consumer(cur);
            if (c < 0 || nodes_[c].inputs.empty() || nodes_[c].inputs[0] != cur) return false;
            const std::string &ct = nodes_[c].op_type;
            if (ct == "DFT") {
                Val o = x;
                o.win_name = n.inputs[a.is_const ? 0 : 1];
                o.win_nu = 0;
                for (int k = 0; k < ax; k++) o.win_nu += x.dims[k] != 1;
                define(n.outputs[0], o);
                return true;
            }
            if (ct != "Unsqueeze" && ct != "Squeeze" && ct != "Reshape" && ct != "Identity") return false;
            cur = nodes_[c].outputs[0];
        }
        return false;
    }

    // ONNX DFT (opset 17: attribute axis, default 1; opset 20: input axis, default -2): forward, real input [.., L, 1], optional constant
    // dft_length N (zero-padded or truncated signal), onesided -> N/2 + 1 bins, output [.., bins, 2].  The frames [F, L] along `axis` are
    // rows of a framing convolution over the flat view they come from (hop = frame stride / sample stride: overlapping views of a signal
    // -- tf.signal.frame through lower_gather -- or hop = L for a materialised tensor), exactly like lower_stft: one cos | -sin bank built in
    // double precision with a pending window folded in, so the mirror / quarter folds and the FFT kernel apply to it like to any bank.
    void lower_dft(const OnnxNode &n) {
        Val x = get(n, 0);
        if (x.is_const) unsupported(n, "DFT of a constant signal");
        if (n.attr_i("inverse", 0) != 0) unsupported(n, "inverse DFT is outside the native subset (no BirdNET / Perch front end needs it)");
        const int64_t r = (int64_t)x.dims.size() + 1;
        if (x.dims.empty() || x.dims.back() == 2) unsupported(n, "complex input (last dimension 2) is outside the native subset; the front ends transform a real signal");
        if (x.dims.back() != 1) unsupported(n, "input must end in a dimension of 1 (real) per the operator's definition, got per-sample dims " + dims_str(x.dims));
        int64_t axis = n.has("axis") ? n.attr_i("axis", 1) : (m_.opset >= 20 ? -2 : 1);
        if (!n.has("axis") && has_input(n, 2)) axis = const_ints(n, get(n, 2)).at(0);
        if (axis < 0) axis += r;
        if (axis <= 0 || axis >= r - 1) unsupported(n, "DFT axis must be a signal dimension (not the batch, not the trailing real / imaginary one)");
        axis -= 1;
        const int64_t L = x.dims[axis];
        int64_t N = L;
        if (has_input(n, 1)) { const Val &dl = get(n, 1); if (!dl.is_const) unsupported(n, "dft_length must be a constant"); N = const_ints(n, dl).at(0); }
        if (N <= 0) unsupported(n, "dft_length must be positive");
        const int64_t taps = std::min(L, N);  // a longer transform zero-pads the signal (= fewer taps per basis row), a shorter one truncates it
        const bool onesided = n.attr_i("onesided", 0) != 0;
        const int64_t bins = onesided ? N / 2 + 1 : N;
        if (taps * 2 * bins > ((int64_t)1 << 28)) unsupported(n, "DFT basis too large");
        // pending window: must lie along the transformed axis and have its length
        std::vector<float> win;
        if (!x.win_name.empty()) {
            int nu = 0;
            for (int64_t k = 0; k < axis; k++) nu += x.dims[k] != 1;
            const Val &w = vals_.at(x.win_name);
            if (nu == x.win_nu && w.numel() == L) win = w.f;
            else x = apply_window(x, n.inputs[0]);
            x.win_name.clear();
            x.win_nu = -1;
        }
        // frames: every non-unit dim except `axis` and the trailing 1, merged into one row index with ONE stride if the view allows it
        Dims lead, lead_s;
        for (int64_t k = 0; k + 1 < (int64_t)x.dims.size(); k++)
            if (k != axis && x.dims[k] != 1) { lead.push_back(x.dims[k]); lead_s.push_back(x.strides[k]); }
        int64_t F = 1;
        for (auto d : lead) F *= d;
        int64_t sL = x.strides[axis], sF = lead.empty() ? L * sL : lead_s.back();
        bool rows_ok = sL > 0 && sF > 0 && sF % sL == 0;
        for (size_t k = 0; k + 1 < lead.size() && rows_ok; k++) rows_ok = lead_s[k] == lead[k + 1] * lead_s[k + 1];
        if (!rows_ok) {  // arbitrary view: copy the frames into [lead..., L] row-major, then they are non-overlapping rows
            Dims keep = x.dims;
            Val c = materialize(x, row_major(keep), n.name + "/frames");
            x = c;
            lead_s.clear();
            for (int64_t k = 0; k + 1 < (int64_t)x.dims.size(); k++)
                if (k != axis && x.dims[k] != 1) lead_s.push_back(x.strides[k]);
            sL = x.strides[axis];
            sF = lead.empty() ? L * sL : lead_s.back();
            rows_ok = sL > 0 && sF % sL == 0;
            for (size_t k = 0; k + 1 < lead.size() && rows_ok; k++) rows_ok = lead_s[k] == lead[k + 1] * lead_s[k + 1];
            if (!rows_ok) unsupported(n, "DFT axis must be the innermost signal dimension of its frames (transpose the frames first)");
        }
        const int64_t hop = sF / sL;
        Val w;
        w.is_const = true;
        w.dims = {2 * bins, 1, taps};
        w.f.resize((size_t)(2 * bins * taps));
        for (int64_t k = 0; k < bins; k++)
            for (int64_t t = 0; t < taps; t++) {
                const double wv = win.empty() ? 1.0 : (double)win[(size_t)t];
                const double th = 2.0 * M_PI * (double)((k * t) % N) / (double)N;
                w.f[(size_t)(k * taps + t)] = (float)(wv * std::cos(th));
                w.f[(size_t)((bins + k) * taps + t)] = (float)(-wv * std::sin(th));
            }
        const std::string base = "dft:" + (n.name.empty() ? n.outputs[0] : n.name);
        const int64_t span = (F - 1) * hop + taps;
        Val xv = x;
        xv.dims = {1, span};
        xv.strides = {span * sL, sL};
        vals_[base + "/signal"] = xv;
        vals_[base + "/basis"] = std::move(w);
        OnnxNode conv;
        conv.name = base;
        conv.op_type = "Conv";
        conv.inputs = {base + "/signal", base + "/basis"};
        conv.outputs = {base + "/frames"};
        set_ints(conv, "strides", {hop});
        lower_conv(conv);
        auto yit = vals_.find(base + "/frames");
        if (yit == vals_.end()) unsupported(n, "internal: the framing conv defined no output");
        const Val y = yit->second;
        if (y.is_const || y.dims.size() != 2 || y.dims[0] != 2 * bins || y.dims[1] != F) unsupported(n, "internal: framing conv produced " + dims_str(y.dims));
        // the node's result: x's dims with `axis` -> bins and the trailing 1 -> 2, as a strided view of the conv's [2 bins, F] output
        Val out = y;
        out.dims = x.dims;
        out.strides.assign(x.dims.size(), 0);
        int64_t fs = y.strides[1];
        for (int64_t k = (int64_t)x.dims.size() - 2; k >= 0; k--) {
            if (k == axis || x.dims[k] == 1) continue;
            out.strides[k] = fs;
            fs *= x.dims[k];
        }
        out.dims[axis] = bins;
        out.strides[axis] = y.strides[0];
        out.dims.back() = 2;
        out.strides.back() = bins * y.strides[0];
        define(n.outputs[0], out);
    }

    void lower_transpose(const OnnxNode &n) {
        const Val &v = get(n, 0);
        auto perm = n.attr_ints("perm");
        size_t r = v.dims.size() + 1;
        if (perm.empty()) for (size_t k = 0; k < r; k++) perm.push_back((int64_t)(r - 1 - k));
        if (perm.size() != r || perm[0] != 0) unsupported(n, "Transpose must keep the batch as the leading dimension");
        Val o = v;
        for (size_t k = 1; k < r; k++) { o.dims[k - 1] = v.dims[perm[k] - 1]; o.strides[k - 1] = v.strides[perm[k] - 1]; }
        define(n.outputs[0], o);
    }

    void slice_params(const OnnxNode &n, const Dims &dims, const Dims &strides, Dims &nd, Dims &ns, int64_t &off, bool batched) {
        std::vector<int64_t> starts, ends, axes, steps;
        if (n.has("starts")) { starts = n.attr_ints("starts"); ends = n.attr_ints("ends"); axes = n.attr_ints("axes"); }
        else {
            starts = const_ints(n, get(n, 1));
            ends = const_ints(n, get(n, 2));
            if (has_input(n, 3)) axes = const_ints(n, get(n, 3));
            if (has_input(n, 4)) steps = const_ints(n, get(n, 4));
        }
        int64_t r = (int64_t)dims.size() + (batched ? 1 : 0);
        if (axes.empty()) for (size_t k = 0; k < starts.size(); k++) axes.push_back((int64_t)k);
        if (steps.empty()) steps.assign(starts.size(), 1);
        nd = dims; ns = strides; off = 0;
        for (size_t k = 0; k < starts.size(); k++) {
            int64_t ax = axes[k] < 0 ? axes[k] + r : axes[k];
            if (batched) { if (ax == 0) unsupported(n, "Slice along the batch dimension"); ax -= 1; }
            int64_t d = dims[ax], st = steps[k], s = starts[k], e = ends[k];
            if (st == 0) unsupported(n, "Slice step 0");
            if (s < 0) s += d;
            if (e < 0) e += d;
            int64_t cnt;
            if (st > 0) { s = std::clamp<int64_t>(s, 0, d); e = std::clamp<int64_t>(e, 0, d); cnt = e > s ? (e - s + st - 1) / st : 0; }
            else {
                // ONNX: clamp start to [0, d-1], end to [-1, d-1] for negative steps
                int64_t s0 = starts[k] < 0 ? starts[k] + d : starts[k];
                int64_t e0 = ends[k];
                if (e0 < -d - 1) e0 = -1; else if (e0 < 0) e0 += d;
                s = std::clamp<int64_t>(s0, 0, d - 1);
                e = std::clamp<int64_t>(e0, -1, d - 1);
                cnt = s > e ? (s - e + (-st) - 1) / (-st) : 0;
            }
            if (cnt <= 0) unsupported(n, "Slice produces an empty tensor");
            off += s * strides[ax];
            nd[ax] = cnt;
            ns[ax] = strides[ax] * st;
        }
    }
    void lower_slice(const OnnxNode &n) {
        const Val &v = get(n, 0);
        Val o = v;
        int64_t off;
        slice_params(n, v.dims, v.strides, o.dims, o.strides, off, true);
        o.offset = v.offset + off;
        define(n.outputs[0], o);
    }

    void lower_concat(const OnnxNode &n) {
        std::vector<Val> ins;
        for (size_t k = 0; k < n.inputs.size(); k++) {
            Val v = get(n, k);
            if (v.is_const) v = upload_as_activation(v);
            ins.push_back(v);
        }
        int64_t r = (int64_t)ins[0].dims.size() + 1;
        int64_t axis = n.attr_i("axis", 0);
        if (axis < 0) axis += r;
        if (axis == 0) unsupported(n, "Concat along the batch dimension");
        axis -= 1;
        Dims od = ins[0].dims;
        od[axis] = 0;
        for (auto &v : ins) {
            if (v.dims.size() != od.size()) unsupported(n, "rank mismatch");
            od[axis] += v.dims[axis];
        }
        // layout: channels-last when the result (through elementwise ops) feeds a convolution,
        // else follow the first input's physical order
        bool to_conv = false;
        {
            std::string cur = n.outputs[0];
            for (int hop = 0; hop < 6 && !to_conv; hop++) {
                int c = sole_consumer(cur);
                if (c < 0) break;
                const OnnxNode &cn = nodes_[c];
                if (cn.op_type == "Conv" && cn.inputs[0] == cur) to_conv = true;
                else if (cn.inputs[0] == cur && (cn.op_type == "BatchNormalization" || cn.op_type == "Relu" || cn.op_type == "Clip" ||
                                                 cn.op_type == "Mul" || cn.op_type == "Add" || cn.op_type == "Sub" || cn.op_type == "Div" ||
                                                 cn.op_type == "Sigmoid" || cn.op_type == "Pow" || cn.op_type == "Log" || cn.op_type == "Sqrt"))
                    cur = cn.outputs[0];
                else break;
            }
        }
        Dims ostr = strides_for_order(od, phys_order(ins[0]));
        if (to_conv && od.size() == 3) ostr = Dims{1, od[2] * od[0], od[0]};
        else if (to_conv && od.size() == 2) ostr = Dims{1, od[0]};
        Val out = new_act(od, ostr);
        // Concat of single-channel planes along the channel axis followed by BatchNormalization (the v2.4 spectrogram
        // image): every plane sees ONE scale and shift, so the normalisation rides on the copy of each plane (and, with
        // rule E, ends up in the epilogue of the GEMM that produced it) instead of one more pass over the image.
        std::vector<float> plane_s, plane_t;
        std::string result = n.outputs[0];
        if (axis == 0 && od[0] == (int64_t)ins.size()) {
            int c = sole_consumer(n.outputs[0]);
            if (c >= 0 && nodes_[c].op_type == "BatchNormalization" && nodes_[c].inputs.size() >= 5 && nodes_[c].inputs[0] == n.outputs[0]) {
                const OnnxNode &bn_ = nodes_[c];
                const Val &sc = get(bn_, 1), &bi = get(bn_, 2), &mu = get(bn_, 3), &var = get(bn_, 4);
                if (sc.is_const && bi.is_const && mu.is_const && var.is_const && sc.numel() == od[0] && bi.numel() == od[0] &&
                    mu.numel() == od[0] && var.numel() == od[0] && bn_.outputs.size() == 1) {
                    const float eps = bn_.attr_f("epsilon", 1e-5f);
                    for (int64_t k = 0; k < od[0]; k++) {
                        const float sk = sc.f[k] / std::sqrt(var.f[k] + eps);
                        plane_s.push_back(sk);
                        plane_t.push_back(bi.f[k] - mu.f[k] * sk);
                    }
                    absorbed_[c] = true;
                    result = bn_.outputs[0];
                }
            }
        }
        int64_t pos = 0;
        for (auto &v : ins) {
            Val slot = out;
            slot.dims = v.dims;
            slot.offset = out.offset + pos * out.strides[axis];
            ActSpec plane_act;
            std::string what = "concat:" + n.name;
            if (!plane_s.empty()) {
                plane_act.act = ACT_AFFINE; plane_act.p0 = plane_s[(size_t)pos]; plane_act.p1 = plane_t[(size_t)pos];
                what += "+bn";
            }
            emit_elt(what, slot, ref_of(v), v.strides, batch_stride(v), Ref{}, {}, 0, BIN_NONE, plane_act);
            pos += v.dims[axis];
        }
        define(result, out);
    }

    // Padded copy of an activation (per-sample dims): the whole result is filled with `value`, then
    // the interior is overwritten by the input.  Two strided elementwise launches, no new kernel.
    Val pad_copy(Val v, const Dims &lo, const Dims &hi, float value, const std::string &name) {
        if (v.is_const) v = upload_as_activation(v);
        if (v.gate_storage >= 0) v = apply_gate(v, name);
        Dims od = v.dims;
        for (size_t i = 0; i < od.size(); i++) od[i] += lo[i] + hi[i];
        Val out = new_act(od, strides_for_order(od, phys_order(v)));
        Ref fill{Space::CONSTS, add_const(std::vector<float>{value}), 0};
        emit_elt("pad.fill:" + name, out, fill, Dims(od.size(), 0), 0, Ref{}, {}, 0, BIN_NONE, ActSpec{});
        Val slot = out;
        slot.dims = v.dims;
        for (size_t i = 0; i < od.size(); i++) slot.offset += lo[i] * out.strides[i];
        emit_elt("pad.copy:" + name, slot, ref_of(v), v.strides, batch_stride(v), Ref{}, {}, 0, BIN_NONE, ActSpec{});
        return out;
    }

    // ONNX Pad, constant mode (pads as attribute for opset < 11, as input otherwise)
    void lower_pad(const OnnxNode &n) {
        Val x = get(n, 0);
        if (n.attr_s("mode", "constant") != "constant") unsupported(n, "only constant-mode Pad is supported");
        std::vector<int64_t> pads = n.attr_ints("pads");
        float value = n.attr_f("value", 0.0f);
        if (pads.empty()) {
            const Val *pv = opt(n, 1);
            if (!pv || !pv->is_const) unsupported(n, "Pad needs constant pads");
            pads = pv->i;
            const Val *cv = opt(n, 2);
            if (cv) { if (!const_scalar(*cv, value)) unsupported(n, "Pad needs a constant fill value"); }
        }
        const size_t r = x.dims.size() + 1;  // with the batch dimension
        std::vector<int64_t> axes;
        if (const Val *av = opt(n, 3)) {
            if (!av->is_const) unsupported(n, "Pad needs constant axes");
            axes = av->i;
        } else {
            for (size_t i = 0; i < r; i++) axes.push_back((int64_t)i);
        }
        if (pads.size() != 2 * axes.size()) unsupported(n, "pads/axes size mismatch");
        Dims lo(x.dims.size(), 0), hi(x.dims.size(), 0);
        for (size_t k = 0; k < axes.size(); k++) {
            int64_t ax = axes[k] < 0 ? axes[k] + (int64_t)r : axes[k];
            const int64_t p0 = pads[k], p1 = pads[axes.size() + k];
            if (p0 < 0 || p1 < 0) unsupported(n, "negative pads");
            if (ax == 0) { if (p0 || p1) unsupported(n, "Pad along the batch dimension"); continue; }
            lo[ax - 1] = p0; hi[ax - 1] = p1;
        }
        define(n.outputs[0], pad_copy(x, lo, hi, value, n.name));
    }

    // MaxPool / AveragePool (1-D or 2-D, no dilation, floor mode) on a channels-last tensor.
    void lower_pool(const OnnxNode &n) {
        Val x = get(n, 0);
        if (x.is_const) unsupported(n, "pooling of a constant");
        if (x.gate_storage >= 0) x = apply_gate(x, n.name);
        const size_t sp = x.dims.size() - 1;
        if (sp != 1 && sp != 2) unsupported(n, "only 1-D and 2-D pooling is supported");
        if (n.attr_i("ceil_mode", 0) != 0) unsupported(n, "ceil_mode pooling");
        for (auto dd : n.attr_ints("dilations")) if (dd != 1) unsupported(n, "dilated pooling");
        if (n.outputs.size() > 1 && !n.outputs[1].empty()) unsupported(n, "MaxPool indices output");
        auto ks = n.attr_ints("kernel_shape");
        if (ks.size() != sp) unsupported(n, "kernel_shape rank mismatch");
        auto st = n.attr_ints("strides");
        if (st.empty()) st.assign(sp, 1);
        auto pads = n.attr_ints("pads");
        if (pads.empty()) pads.assign(2 * sp, 0);
        if (st.size() != sp || pads.size() != 2 * sp) unsupported(n, "strides / pads do not match the spatial rank");
        for (auto e : ks) if (e <= 0) unsupported(n, "kernel_shape must be positive");
        for (auto e : st) if (e <= 0) unsupported(n, "strides must be positive");
        for (auto e : pads) if (e < 0) unsupported(n, "negative pads");
        const int64_t C = x.dims[0], H = sp == 2 ? x.dims[1] : 1, W = sp == 2 ? x.dims[2] : x.dims[1];
        const int64_t kh = sp == 2 ? ks[0] : 1, kw = sp == 2 ? ks[1] : ks[0];
        const int64_t sh = sp == 2 ? st[0] : 1, sw = sp == 2 ? st[1] : st[0];
        int64_t pt = sp == 2 ? pads[0] : 0, pl = sp == 2 ? pads[1] : pads[0], pb = sp == 2 ? pads[2] : 0, pr = sp == 2 ? pads[3] : pads[1];
        const std::string auto_pad = n.attr_s("auto_pad", "NOTSET");
        const int64_t OH = window_out_dim(auto_pad, H, kh, sh, pt, pb), OW = window_out_dim(auto_pad, W, kw, sw, pl, pr);
        if (OH <= 0 || OW <= 0) unsupported(n, "empty pooling output");
        x = to_channels_last(x, n.name);
        Dims od = sp == 2 ? Dims{C, OH, OW} : Dims{C, OW};
        Dims ostr = sp == 2 ? Dims{1, OW * C, C} : Dims{1, C};
        Val out = new_act(od, ostr);
        PlanOp op;
        op.kind = OpKind::POOL;
        op.name = n.op_type + ":" + n.name;
        op.r.out = ref_of(out);
        op.r.a = ref_of(x);
        PoolDesc &d = op.pool;
        d.H = (int32_t)H; d.W = (int32_t)W; d.C = (int32_t)C; d.OH = (int32_t)OH; d.OW = (int32_t)OW;
        d.kh = (int32_t)kh; d.kw = (int32_t)kw; d.sh = (int32_t)sh; d.sw = (int32_t)sw; d.pt = (int32_t)pt; d.pl = (int32_t)pl;
        d.is_max = n.op_type == "MaxPool" ? 1 : 0;
        d.count_include_pad = (int32_t)n.attr_i("count_include_pad", 0);
        d.in_bs = batch_stride(x); d.out_bs = plan_.storages[out.storage].elems;
        op.macs = 0;
        op.bytes = 4.0 * ((double)C * H * W + (double)C * OH * OW);
        push_op(std::move(op));
        define(n.outputs[0], out);
    }

    // Softmax / LogSoftmax over one non-batch axis, expanded into the launches the engine already has
    // (max -> x - max -> exp -> sum -> divide, or ... -> log(sum) -> subtract); the elementwise-chain pass fuses
    // the neighbours.  Opset < 13 semantics (flatten from `axis`) coincide with this when `axis` is the last one.
    void lower_softmax(const OnnxNode &n) {
        const Val &x = get(n, 0);
        if (x.is_const) unsupported(n, "Softmax of a constant");
        const int64_t r = (int64_t)x.dims.size() + 1;
        int64_t axis = n.attr_i("axis", -1);
        if (axis < 0) axis += r;
        if (axis <= 0 || axis >= r) unsupported(n, "Softmax over the batch dimension");
        auto mk = [&](const char *op, const std::string &suffix, std::vector<std::string> ins, const std::string &out) {
            OnnxNode q;
            q.op_type = op;
            q.name = n.name + "/" + suffix;
            q.inputs = std::move(ins);
            q.outputs = {out};
            return q;
        };
        auto with_axes = [&](OnnxNode q) {
            OnnxAttr a;
            a.name = "axes"; a.type = 7; a.ints = {axis};
            q.attrs["axes"] = a;
            OnnxAttr k;
            k.name = "keepdims"; k.type = 2; k.i = 1;
            q.attrs["keepdims"] = k;
            return q;
        };
        const std::string b = n.outputs[0] + "/sm.";
        lower_reduce(with_axes(mk("ReduceMax", "max", {n.inputs[0]}, b + "max")));
        lower_binary(mk("Sub", "shift", {n.inputs[0], b + "max"}, b + "shift"));
        ActSpec e; e.act = ACT_EXP;
        lower_unary(mk("Exp", "exp", {b + "shift"}, b + "exp"), e);
        lower_reduce(with_axes(mk("ReduceSum", "sum", {b + "exp"}, b + "sum")));
        if (n.op_type == "Softmax") {
            lower_binary(mk("Div", "div", {b + "exp", b + "sum"}, n.outputs[0]));
        } else {
            ActSpec l; l.act = ACT_LOG;
            lower_unary(mk("Log", "log", {b + "sum"}, b + "lse"), l);
            lower_binary(mk("Sub", "sub", {b + "shift", b + "lse"}, n.outputs[0]));
        }
    }

    // Split along a non-batch axis: every output is a view (no launch).
    void lower_split(const OnnxNode &n) {
        const Val &v = get(n, 0);
        const int64_t r = (int64_t)v.dims.size() + 1;
        int64_t axis = n.attr_i("axis", 0);
        if (axis < 0) axis += r;
        if (axis <= 0 || axis >= r) unsupported(n, "Split along the batch dimension");
        axis -= 1;
        std::vector<int64_t> sizes = n.attr_ints("split");
        if (sizes.empty() && has_input(n, 1)) sizes = const_ints(n, get(n, 1));
        const int64_t nout = (int64_t)n.outputs.size();
        if (sizes.empty()) {
            const int64_t each = (v.dims[axis] + nout - 1) / nout;
            for (int64_t k = 0; k < nout; k++) sizes.push_back(std::min(each, v.dims[axis] - k * each));
        }
        if ((int64_t)sizes.size() != nout) unsupported(n, "split sizes do not match the outputs");
        int64_t pos = 0;
        for (int64_t k = 0; k < nout; k++) {
            if (sizes[k] < 0 || pos + sizes[k] > v.dims[axis]) unsupported(n, "split sizes exceed the dimension");
            if (v.is_const) unsupported(n, "Split of a constant");
            Val o = v;
            o.dims[axis] = sizes[k];
            o.offset = v.offset + pos * v.strides[axis];
            if (!n.outputs[k].empty()) define(n.outputs[k], o);
            pos += sizes[k];
        }
    }

    bool unary_spec(const OnnxNode &n, ActSpec &a) {
        const std::string &t = n.op_type;
        if (t == "Relu") a.act = ACT_RELU;
        else if (t == "Sigmoid") a.act = ACT_SIGMOID;
        else if (t == "Tanh") a.act = ACT_TANH;
        else if (t == "Exp") a.act = ACT_EXP;
        else if (t == "Log") a.act = ACT_LOG;
        else if (t == "Sqrt") a.act = ACT_SQRT;
        else if (t == "Abs") a.act = ACT_ABS;
        else if (t == "Neg") a.act = ACT_NEG;
        else if (t == "Reciprocal") a.act = ACT_RECIP;
        else if (t == "Floor") a.act = ACT_FLOOR;
        else if (t == "Ceil") a.act = ACT_CEIL;
        else if (t == "Round") a.act = ACT_ROUND;
        else if (t == "Erf") a.act = ACT_ERF;
        else if (t == "Softplus") a.act = ACT_SOFTPLUS;
        else if (t == "HardSwish") a.act = ACT_HSWISH;
        else if (t == "HardSigmoid") { a.act = ACT_HSIGMOID; a.p0 = n.attr_f("alpha", 0.2f); a.p1 = n.attr_f("beta", 0.5f); }
        else if (t == "LeakyRelu") { a.act = ACT_LEAKY; a.p0 = n.attr_f("alpha", 0.01f); }
        else if (t == "Clip") {
            float lo = -INFINITY, hi = INFINITY;
            if (n.has("min")) lo = n.attr_f("min", lo);
            if (n.has("max")) hi = n.attr_f("max", hi);
            if (has_input(n, 1)) { if (!const_scalar(get(n, 1), lo)) return false; }
            if (has_input(n, 2)) { if (!const_scalar(get(n, 2), hi)) return false; }
            a.act = ACT_CLIP; a.p0 = lo; a.p1 = hi;
        } else return false;
        return true;
    }
    // activation pattern starting at tensor `cur`: returns true and the final tensor name if absorbed
    bool absorb_activation(std::string &cur, ActSpec &a) {
        auto cons = live_consumers(cur);
        if (wanted_names_.count(cur)) return false;
        if (cons.size() == 1) {
            const OnnxNode &c = nodes_[cons[0]];
            if (c.inputs.empty() || c.inputs[0] != cur) return false;
            ActSpec s;
            if (!unary_spec(c, s) || !act_in(ACT_SET_CONV, s.act)) return false;  // (a bare Sigmoid is fusable too)
            a = s;
            absorbed_[cons[0]] = true;
            cur = c.outputs[0];
            return true;
        }
        if (cons.size() == 2) {  // x * sigmoid(x)
            int si = -1, mi = -1;
            for (int k : cons) { if (nodes_[k].op_type == "Sigmoid") si = k; else if (nodes_[k].op_type == "Mul") mi = k; }
            if (si < 0 || mi < 0) return false;
            const OnnxNode &sg = nodes_[si], &ml = nodes_[mi];
            if (sole_consumer(sg.outputs[0]) != mi) return false;
            bool ok = (ml.inputs[0] == cur && ml.inputs[1] == sg.outputs[0]) || (ml.inputs[1] == cur && ml.inputs[0] == sg.outputs[0]);
            if (!ok) return false;
            a.act = ACT_SILU;
            absorbed_[si] = absorbed_[mi] = true;
            cur = ml.outputs[0];
            return true;
        }
        return false;
    }

    void lower_unary(const OnnxNode &n, ActSpec a) {
        const Val &v = get(n, 0);
        if (v.is_const) unsupported(n, "constant operand not foldable");
        Val out = new_act(v.dims, strides_for_order(v.dims, phys_order(v)));
        emit_elt(n.op_type + ":" + n.name, out, ref_of(v), v.strides, batch_stride(v), Ref{}, {}, 0, BIN_NONE, a);
        define(n.outputs[0], out);
    }

    void lower_binary(const OnnxNode &n) {
        const Val &a = get(n, 0), &b = get(n, 1);
        const std::string &t = n.op_type;
        if (t == "Mul" && (a.is_gate != b.is_gate)) {
            // x * se_gate: leave it pending on the value; the consuming 1x1 conv folds it into its
            // operand load, any other consumer triggers apply_gate() in get()
            const Val &x = a.is_gate ? b : a;
            const Val &g = a.is_gate ? a : b;
            if (!x.is_const && x.gate_storage < 0 && x.dims.size() == 3 && x.dims[0] == g.dims[0] && x.space == Space::ARENA) {
                Val o = x;
                o.gate_storage = g.storage;
                if (wanted_names_.count(n.outputs[0])) o = apply_gate(o, n.name);
                define(n.outputs[0], o);
                return;
            }
        }
        if (t == "Mul" && a.is_const != b.is_const && try_pending_window(n, a, b)) return;
        int bin = t == "Add" ? BIN_ADD : t == "Sub" ? BIN_SUB : t == "Mul" ? BIN_MUL : t == "Div" ? BIN_DIV : t == "Pow" ? BIN_POW : t == "Max" ? BIN_MAX
                : t == "And" ? BIN_MUL : t == "Or" ? BIN_MAX : compare_code(t) != BIN_NONE ? compare_code(t) : BIN_MIN;
        // scalar constants become parametrised unary ops
        float c;
        if (!a.is_const && const_scalar(b, c)) {
            ActSpec s;
            bool ok = true;
            switch (bin) {
                case BIN_ADD: s = {ACT_AFFINE, 1.0f, c}; break;
                case BIN_SUB: s = {ACT_AFFINE, 1.0f, -c}; break;
                case BIN_MUL: s = {ACT_AFFINE, c, 0.0f}; break;
                case BIN_MAX: s = {ACT_MAXC, c, 0}; break;
                case BIN_MIN: s = {ACT_MINC, c, 0}; break;
                case BIN_POW:
                    if (c == 2.0f) s = {ACT_SQUARE, 0, 0};
                    else if (c == 0.5f) s = {ACT_SQRT, 0, 0};
                    else if (c == 1.0f) s = {ACT_AFFINE, 1.0f, 0.0f};
                    else s = {ACT_POW, c, 0};
                    break;
                case BIN_GT: s = {ACT_GTC, c, 0}; break;
                case BIN_LT: s = {ACT_LTC, c, 0}; break;
                case BIN_GE: s = {ACT_GEC, c, 0}; break;
                case BIN_LE: s = {ACT_LEC, c, 0}; break;
                case BIN_EQ: s = {ACT_EQC, c, 0}; break;
                default: ok = false;
            }
            if (ok && (t == "And" || t == "Or")) ok = false;  // (logic on 0 / 1 tensors takes the general path)
            if (ok) return lower_unary(n, s);
        }
        if (!b.is_const && const_scalar(a, c)) {
            ActSpec s;
            bool ok = true;
            switch (bin) {
                case BIN_ADD: s = {ACT_AFFINE, 1.0f, c}; break;
                case BIN_MUL: s = {ACT_AFFINE, c, 0.0f}; break;
                case BIN_SUB: s = {ACT_RSUB, c, 0}; break;
                case BIN_DIV: s = {ACT_RDIV, c, 0}; break;
                case BIN_MAX: s = {ACT_MAXC, c, 0}; break;
                case BIN_MIN: s = {ACT_MINC, c, 0}; break;
                case BIN_GT: s = {ACT_LTC, c, 0}; break;  // c > x
                case BIN_LT: s = {ACT_GTC, c, 0}; break;
                case BIN_GE: s = {ACT_LEC, c, 0}; break;
                case BIN_LE: s = {ACT_GEC, c, 0}; break;
                case BIN_EQ: s = {ACT_EQC, c, 0}; break;
                default: ok = false;
            }
            if (ok && (t == "And" || t == "Or")) ok = false;
            if (ok) {
                OnnxNode sw = n;
                std::swap(sw.inputs[0], sw.inputs[1]);
                return lower_unary(sw, s);
            }
        }
        // general broadcast; result dims
        auto act_dims = [&](const Val &v) { Dims d = v.dims; if (v.is_const) { if (d.size() > 0 && (int64_t)d.size() > 0) {} } return d; };
        (void)act_dims;
        // Normalise both to per-sample dims: constants may carry a leading batch dim of 1.
        auto per_sample = [&](const Val &v, size_t rank_hint) {
            Dims d = v.dims;
            if (v.is_const && d.size() == rank_hint + 1) {
                if (d[0] != 1) unsupported(n, "constant operand has a non-unit batch dimension");
                d.erase(d.begin());
            }
            return d;
        };
        size_t ra = a.is_const ? 0 : a.dims.size(), rb = b.is_const ? 0 : b.dims.size();
        size_t rank = std::max(ra, rb);
        Dims da = per_sample(a, rank), db = per_sample(b, rank);
        if (da.size() > rank || db.size() > rank) {
            // constant with more dims than the activation (e.g. [1,C,1,1] against [B,C]) is not expected
            rank = std::max(da.size(), db.size());
        }
        Dims od = bcast_dims(da, db);
        // dominant operand decides layout
        const Val *dom = nullptr;
        if (!a.is_const && prod(da) == prod(od) && da.size() == od.size()) dom = &a;
        else if (!b.is_const && prod(db) == prod(od) && db.size() == od.size()) dom = &b;
        Val out = dom ? new_act(od, strides_for_order(od, phys_order(*dom))) : new_act(od, row_major(od));
        auto operand = [&](const Val &v, const Dims &d, Ref &r, Dims &s, int64_t &bs) {
            if (v.is_const) {
                std::vector<float> data = v.is_int ? std::vector<float>(v.i.begin(), v.i.end()) : v.f;
                r = Ref{Space::CONSTS, add_const(data), 0};
                s = bcast_strides(&n, d, row_major(d), od);
                bs = 0;
            } else {
                r = ref_of(v);
                s = bcast_strides(&n, d, v.strides, od);
                bs = batch_stride(v);
            }
        };
        Ref ra_, rb_; Dims sa, sb; int64_t ba, bb;
        operand(a, da, ra_, sa, ba);
        operand(b, db, rb_, sb, bb);
        emit_elt(t + ":" + n.name, out, ra_, sa, ba, rb_, sb, bb, bin, ActSpec{});
        define(n.outputs[0], out);
    }

    // Where(cond, x, y) with at least one activation among the three: SelA(x, cond) + SelB(y, cond) -- each half is exactly x or +0
    // (never x * 0: infinities and NaNs of the unselected branch do not leak), the sum adds a +0; a branch that is the constant 0
    // drops its half.  The one difference to a true select: a selected -0.0 comes out as +0.0.
    void lower_where(const OnnxNode &n) {
        if (n.inputs.size() != 3) unsupported(n, "Where takes three inputs");
        const Val &x = get(n, 1), &y = get(n, 2);
        float c;
        const bool x0 = const_scalar(x, c) && c == 0.0f, y0 = const_scalar(y, c) && c == 0.0f;
        const std::string base = "where:" + n.outputs[0];
        if (y0 && !x0) return lower(synth_node("bn.SelA", n.name, {n.inputs[1], n.inputs[0]}, n.outputs[0]));
        if (x0 && !y0) return lower(synth_node("bn.SelB", n.name, {n.inputs[2], n.inputs[0]}, n.outputs[0]));
        lower(synth_node("bn.SelA", n.name + "/x", {n.inputs[1], n.inputs[0]}, base + "/x"));
        lower(synth_node("bn.SelB", n.name + "/y", {n.inputs[2], n.inputs[0]}, base + "/y"));
        lower(synth_node("Add", n.name, {base + "/x", base + "/y"}, n.outputs[0]));
    }

    void lower_batchnorm(const OnnxNode &n) {
        const Val &x = get(n, 0);
        const Val &sc = get(n, 1), &bi = get(n, 2), &mu = get(n, 3), &var = get(n, 4);
        if (!sc.is_const || !bi.is_const || !mu.is_const || !var.is_const) unsupported(n, "BatchNormalization parameters must be constants");
        float eps = n.attr_f("epsilon", 1e-5f);
        int64_t C = sc.numel();
        if (x.dims.empty() || x.dims[0] != C) unsupported(n, "channel count mismatch");
        std::vector<float> s(C), t(C);
        for (int64_t c = 0; c < C; c++) { s[c] = sc.f[c] / std::sqrt(var.f[c] + eps); t[c] = bi.f[c] - mu.f[c] * s[c]; }
        Dims cd(x.dims.size(), 1);
        cd[0] = C;
        Val mid = new_act(x.dims, strides_for_order(x.dims, phys_order(x)));
        Ref rs{Space::CONSTS, add_const(s), 0}, rt{Space::CONSTS, add_const(t), 0};
        Dims cs = bcast_strides(&n, cd, row_major(cd), x.dims);
        emit_elt("bn.mul:" + n.name, mid, ref_of(x), x.strides, batch_stride(x), rs, cs, 0, BIN_MUL, ActSpec{});
        Val out = new_act(x.dims, mid.strides);
        emit_elt("bn.add:" + n.name, out, ref_of(mid), mid.strides, batch_stride(mid), rt, cs, 0, BIN_ADD, ActSpec{});
        define(n.outputs[0], out);
    }

    // GlobalAveragePool -> Conv1x1 -> act -> Conv1x1 -> Sigmoid/HardSigmoid -> Mul(x, .) : squeeze-excite.
    // Emits the two SE launches and defines the gate; returns false if the pattern does not match.
    bool try_squeeze_excite(const OnnxNode &n, const Val &x) {
        if (x.dims.size() != 3 || x.space != Space::ARENA || x.gate_storage >= 0) return false;
        const int64_t C = x.dims[0], H = x.dims[1], W = x.dims[2];
        if (C % 4 || C > 4096 || !x.strides_equal(Dims{1, W * C, C}) || x.offset != 0) return false;
        if (plan_.storages[x.storage].elems % 4) return false;
        // spatial mean?
        if (n.op_type == "ReduceMean") {
            auto axes = n.attr_ints("axes");
            if (axes.empty() && has_input(n, 1)) axes = const_ints(n, get(n, 1));
            std::set<int64_t> ax;
            for (auto a : axes) ax.insert(a < 0 ? a + 4 : a);
            if (ax != std::set<int64_t>{2, 3} || n.attr_i("keepdims", 1) == 0) return false;
        } else if (n.op_type != "GlobalAveragePool") return false;
        int c1 = sole_consumer(n.outputs[0]);
        if (c1 < 0 || nodes_[c1].op_type != "Conv") return false;
        auto conv_1x1 = [&](const OnnxNode &cv, int64_t cin, int64_t &cout, std::vector<float> &w, std::vector<float> &b) {
            auto wi = vals_.find(cv.inputs[1]);
            if (wi == vals_.end() || !wi->second.is_const || wi->second.dims.size() != 4) return false;
            const Val &wv = wi->second;
            if (wv.dims[1] != cin || wv.dims[2] != 1 || wv.dims[3] != 1 || cv.attr_i("group", 1) != 1) return false;
            for (auto p : cv.attr_ints("pads")) if (p) return false;
            for (auto p : cv.attr_ints("strides")) if (p != 1) return false;
            cout = wv.dims[0];
            w = wv.f;
            b.clear();
            if (cv.inputs.size() > 2 && !cv.inputs[2].empty()) {
                auto bi = vals_.find(cv.inputs[2]);
                if (bi == vals_.end() || !bi->second.is_const) return false;
                b = bi->second.f;
            }
            return true;
        };
        int64_t Cr = 0, C2 = 0;
        std::vector<float> w1, b1, w2, b2;
        if (nodes_[c1].inputs[0] != n.outputs[0] || !conv_1x1(nodes_[c1], C, Cr, w1, b1) || Cr > 1024) return false;
        // dry-run the chain before absorbing anything
        std::vector<bool> saved = absorbed_;
        auto bail = [&]() { absorbed_ = saved; return false; };
        absorbed_[c1] = true;
        std::string cur = nodes_[c1].outputs[0];
        ActSpec act1;
        absorb_activation(cur, act1);
        int c2 = sole_consumer(cur);
        if (c2 < 0 || nodes_[c2].op_type != "Conv" || nodes_[c2].inputs[0] != cur || !conv_1x1(nodes_[c2], Cr, C2, w2, b2) || C2 != C) return bail();
        absorbed_[c2] = true;
        cur = nodes_[c2].outputs[0];
        int sg = sole_consumer(cur);
        ActSpec act2;
        if (sg < 0 || nodes_[sg].inputs[0] != cur || (nodes_[sg].op_type != "Sigmoid" && nodes_[sg].op_type != "HardSigmoid") || !unary_spec(nodes_[sg], act2)) return bail();
        absorbed_[sg] = true;
        const std::string gate_name = nodes_[sg].outputs[0];
        if (wanted_names_.count(gate_name)) return bail();
        // the gate must only feed Mul(x, gate)
        for (int k : live_consumers(gate_name)) {
            const OnnxNode &m = nodes_[k];
            if (m.op_type != "Mul") return bail();
            const std::string &other = m.inputs[0] == gate_name ? m.inputs[1] : m.inputs[0];
            if (other != n.inputs[0]) return bail();
        }
        // ---- emit
        const int64_t HW = H * W;
        int32_t splits = (int32_t)std::min<int64_t>(64, std::max<int64_t>(1, (HW + 31) / 32));
        // produced by the tiled depthwise kernel just before? then it emits the channel sums itself
        PlanOp *dwp = nullptr;
        if (!plan_.ops.empty()) {
            PlanOp &last = plan_.ops.back();
            if (last.kind == OpKind::DWCONV && last.dw.tiled && last.r.out.space == Space::ARENA && last.r.out.id == x.storage && last.r.out.offset == 0)
                dwp = &last;
        }
        PlanOp *mbp = nullptr;
        if (!dwp && !plan_.ops.empty()) {
            PlanOp &last = plan_.ops.back();
            if (last.kind == OpKind::MBCONV && last.r.out.space == Space::ARENA && last.r.out.id == x.storage && last.r.out.offset == 0) mbp = &last;
        }
        if (dwp) splits = dwp->dw.nblk;
        if (mbp) splits = mbp->mb.tiles_x * mbp->mb.tiles_y;
        Val partial = new_act(Dims{(int64_t)splits, C}, Dims{C, 1});
        if (mbp) {
            mbp->mb.has_gap = 1;
            mbp->mb.gap_bs = plan_.storages[partial.storage].elems;
            mbp->r.gap_out = ref_of(partial);
            touch(mbp->r.gap_out, (int)plan_.ops.size() - 1);
        } else if (dwp) {
            dwp->dw.has_gap = 1;
            dwp->dw.gap_bs = plan_.storages[partial.storage].elems;
            dwp->r.gap_out = ref_of(partial);
            touch(dwp->r.gap_out, (int)plan_.ops.size() - 1);
        } else {
            PlanOp op;
            op.kind = OpKind::GAP;
            op.name = "se.squeeze:" + n.name;
            op.r.out = ref_of(partial);
            op.r.a = ref_of(x);
            op.gap.HW = HW; op.gap.C = (int32_t)C; op.gap.splits = splits;
            op.gap.in_bs = batch_stride(x); op.gap.out_bs = plan_.storages[partial.storage].elems;
            op.bytes = 4.0 * (double)(HW * C + splits * C);
            push_op(std::move(op));
        }
        Val gate = new_act(Dims{C, 1, 1}, Dims{1, 0, 0});
        plan_.storages[gate.storage].elems = (C + 3) / 4 * 4;
        std::vector<float> w2t(w2.size());  // [C][Cr] -> [Cr][C]: coalesced reads in the excite product
        for (int64_t c = 0; c < C; c++)
            for (int64_t j = 0; j < Cr; j++) w2t[j * C + c] = w2[c * Cr + j];
        SeFcDesc sd{};
        sd.C = (int32_t)C; sd.Cr = (int32_t)Cr; sd.splits = splits; sd.inv_hw = 1.0f / (float)HW;
        sd.act1 = act1.act; sd.p0_1 = act1.p0; sd.p1_1 = act1.p1;
        sd.act2 = act2.act; sd.p0_2 = act2.p0; sd.p1_2 = act2.p1;
        sd.in_bs = plan_.storages[partial.storage].elems; sd.out_bs = plan_.storages[gate.storage].elems;
        // Rule H: the launch that produced the squeeze sums finishes the squeeze-excite itself -- its last block per sample
        // (ticket counter, write-through partial sums: no fence, kernels.h SeTail) -- when that launch is a fused MBConv
        // or a whole-map depthwise conv.  One launch less per block (16 in the v2.4 plan).  BN_SEFUSE=0 disables.
        PlanOp *host = nullptr;
        {
            // Opt-in (BN_SEFUSE = dw | mb | 1): correct, but slower than the separate excite launch on every block of the
            // v2.4 plan -- the last block streams both excite matrices through ONE compute unit (442 KB at C = 1152:
            // +26 us per whole-map depthwise launch against 8-10 us for the multi-block excite kernel), and every block of
            // a fused MBConv launch pays a store drain + returning atomic (+13 us per launch); DESIGN.md section 4.12.
            const std::string mode = sw_text(sw::BN_SEFUSE);  // 0 | dw | mb | 1 (both)
            if (mbp && !mbp->mb.whole_map && !mbp->mb.row_mode && (mode == "1" || mode == "mb")) host = mbp;  // the row-streaming form has no block that could be "last"
            else if (dwp && dwp->dw.tiled == 2 && (mode == "1" || mode == "dw")) host = dwp;
        }
        if (host) {
            Val cnt = new_act(Dims{1}, Dims{1});
            plan_.storages[cnt.storage].pinned = true;      // never recycled ...
            plan_.storages[cnt.storage].persistent = true;  // ... and never shared with an earlier tensor either: the word must stay zero between launches
            const int hidx = (int)plan_.ops.size() - 1;
            host->se_fused = 1;
            host->se = sd;
            host->r.se.w1 = Ref{Space::CONSTS, add_const(w1), 0};
            if (!b1.empty()) host->r.se.b1 = Ref{Space::CONSTS, add_const(b1), 0};
            host->r.se.w2t = Ref{Space::CONSTS, add_const(w2t), 0};
            if (!b2.empty()) host->r.se.b2 = Ref{Space::CONSTS, add_const(b2), 0};
            host->r.se.gate = ref_of(gate);
            host->r.se.counter = ref_of(cnt);
            touch(host->r.se.gate, hidx);
            touch(host->r.se.counter, hidx);
            host->name += "+se";
            host->macs += 2.0 * (double)C * Cr;
            host->weight_bytes += 4.0 * (w1.size() + w2.size() + b1.size() + b2.size());
            host->bytes += 4.0 * (double)(splits * C + C);
        } else {
            PlanOp op;
            Val hidden = new_act(Dims{Cr}, Dims{1});
            op.kind = OpKind::SEFC;
            op.name = "se.excite:" + n.name;
            op.r.out = ref_of(gate);
            op.r.a = ref_of(partial);
            op.r.hidden = ref_of(hidden);  // scratch between the two excite launches
            op.r.w = Ref{Space::CONSTS, add_const(w1), 0};
            if (!b1.empty()) op.r.bias = Ref{Space::CONSTS, add_const(b1), 0};
            op.r.w2 = Ref{Space::CONSTS, add_const(w2t), 0};
            if (!b2.empty()) op.r.bias2 = Ref{Space::CONSTS, add_const(b2), 0};
            op.se = sd;
            op.macs = 2.0 * (double)C * Cr;
            op.weight_bytes = 4.0 * (w1.size() + w2.size() + b1.size() + b2.size());
            op.bytes = 4.0 * (double)(splits * C + C);
            push_op(std::move(op));
        }
        gate.is_gate = true;
        define(gate_name, gate);
        return true;
    }

    void lower_reduce(const OnnxNode &n) {
        const Val &v = get(n, 0);
        const std::string &t = n.op_type;
        if (v.is_const) unsupported(n, "reduction of a constant");
        if (try_squeeze_excite(n, v)) return;
        // max(x - s) == max(x) - s exactly when s is one number per reduced range (rounding is monotone), same for min:
        // the reduction reads x itself and the shifted signal is no longer needed for it -- in the min-max normalisation
        // of the v2.4 front end the Sub then has a single consumer left and fuses into the scaling chain (one pass less).
        if ((t == "ReduceMax" || t == "ReduceMin") && sw_on(sw::BN_REDUCE_SHIFT)) {
            int prod = -1;
            for (size_t k = 0; k < nodes_.size() && prod < 0; k++)
                if (live_[k] && !absorbed_[k] && nodes_[k].op_type == "Sub" && nodes_[k].outputs.size() == 1 && nodes_[k].outputs[0] == n.inputs[0]) prod = (int)k;
            if (prod >= 0 && nodes_[prod].inputs.size() == 2 && n.attr_i("keepdims", 1) != 0) {
                const OnnxNode &sub = nodes_[prod];
                auto xi = vals_.find(sub.inputs[0]), si = vals_.find(sub.inputs[1]);
                if (xi != vals_.end() && si != vals_.end() && !xi->second.is_const && xi->second.dims == v.dims && live_consumers(n.inputs[0]).size() > 1) {
                    // s must be constant along every reduced axis: here, one element per sample
                    if (si->second.numel() == 1) {
                        OnnxNode r2 = n;
                        r2.name = n.name + "/unshifted";
                        r2.inputs[0] = sub.inputs[0];
                        r2.outputs = {n.outputs[0] + "/unshifted"};
                        lower_reduce(r2);
                        OnnxNode s2;
                        s2.op_type = "Sub";
                        s2.name = n.name + "/shift";
                        s2.inputs = {r2.outputs[0], sub.inputs[1]};
                        s2.outputs = {n.outputs[0]};
                        lower_binary(s2);
                        return;
                    }
                }
            }
        }
        int op;
        std::vector<int64_t> axes;
        bool keep = n.attr_i("keepdims", 1) != 0;
        int64_t r = (int64_t)v.dims.size() + 1;
        if (t == "GlobalAveragePool" || t == "GlobalMaxPool") {
            op = t == "GlobalAveragePool" ? RED_MEAN : RED_MAX;
            for (int64_t k = 2; k < r; k++) axes.push_back(k);
            keep = true;
        } else {
            if (t == "ReduceMean") op = RED_MEAN; else if (t == "ReduceSum") op = RED_SUM; else if (t == "ReduceMax") op = RED_MAX;
            else if (t == "ReduceMin") op = RED_MIN; else if (t == "ReduceProd") op = RED_PROD; else if (t == "ReduceL2") op = RED_L2;
            else if (t == "ReduceSumSquare") op = RED_SUMSQ; else unsupported(n, "unsupported reduction");
            axes = n.attr_ints("axes");
            if (axes.empty() && has_input(n, 1)) axes = const_ints(n, get(n, 1));
            if (axes.empty()) {
                if (n.attr_i("noop_with_empty_axes", 0)) { define(n.outputs[0], v); return; }
                unsupported(n, "reduction over all axes would include the batch");
            }
        }
        std::set<int> red;
        for (auto a : axes) { if (a < 0) a += r; if (a == 0) unsupported(n, "reduction over the batch dimension"); red.insert((int)a - 1); }
        Dims od;
        for (size_t k = 0; k < v.dims.size(); k++) { if (red.count((int)k)) { if (keep) od.push_back(1); } else od.push_back(v.dims[k]); }
        // kept dims in input physical order
        std::vector<int> ord = phys_order(v);
        PlanOp op_;
        op_.kind = OpKind::REDUCE;
        op_.name = t + ":" + n.name;
        ReduceDesc &d = op_.red;
        d.op = op;
        Dims kept_dims_phys;
        std::vector<int> kept_axes_phys;
        d.kept = d.red = 1;
        d.inner_kept = 0;
        for (int ax : ord) {
            if (v.dims[ax] == 1) continue;
            if (red.count(ax)) {
                if (d.nr >= 3) unsupported(n, "more than 3 reduced dimensions");
                d.rsize[d.nr] = v.dims[ax]; d.rin[d.nr] = v.strides[ax]; d.nr++; d.red *= v.dims[ax];
            } else {
                if (d.nk >= 4) unsupported(n, "more than 4 kept dimensions");
                d.ksize[d.nk] = v.dims[ax]; d.kin[d.nk] = v.strides[ax]; d.nk++; d.kept *= v.dims[ax];
                kept_axes_phys.push_back(ax);
                if (std::abs(v.strides[ax]) == 1) d.inner_kept = 1;
            }
        }
        // output: contiguous over kept dims in input physical order
        Dims ostr_phys(kept_axes_phys.size());
        { int64_t acc = 1; for (int k = (int)kept_axes_phys.size() - 1; k >= 0; k--) { ostr_phys[k] = acc; acc *= v.dims[kept_axes_phys[k]]; } }
        for (int k = 0; k < d.nk; k++) d.kout[k] = ostr_phys[k];
        // logical output strides
        Dims ostr(od.size(), 0);
        {
            size_t oi = 0;
            for (size_t k = 0; k < v.dims.size(); k++) {
                bool is_red = red.count((int)k) != 0;
                if (is_red && !keep) continue;
                if (!is_red && v.dims[k] != 1) {
                    for (size_t q = 0; q < kept_axes_phys.size(); q++) if (kept_axes_phys[q] == (int)k) ostr[oi] = ostr_phys[q];
                }
                oi++;
            }
        }
        Val out = new_act(od, ostr);
        plan_.storages[out.storage].elems = std::max<int64_t>(d.kept, 1);
        d.bi = batch_stride(v);
        d.bo = plan_.storages[out.storage].elems;
        op_.r.out = ref_of(out);
        op_.r.a = ref_of(v);
        op_.bytes = 4.0 * (double)(d.kept * d.red + d.kept);
        // A whole-segment min / max (144 000 samples -> one number) as ONE block per sample leaves the chip idle
        // (32 blocks at batch 32, 26 us).  Min and max do not depend on the order of evaluation, so the range is cut
        // into c chunks reduced by c blocks per sample and a second tiny launch reduces the c partials: bit-identical
        // result, ~4x less time.  Sums keep their single fixed-order pass.  BN_REDUCE_SPLIT=0 disables.
        if ((op == RED_MAX || op == RED_MIN) && d.nk == 0 && d.nr == 1 && d.rin[0] == 1 && d.red >= 32768 &&
            sw_on(sw::BN_REDUCE_SPLIT)) {
            int64_t c = 0;
            for (int64_t q = 64; q >= 4 && !c; q--)
                if (d.red % q == 0 && (d.red / q) % 4 == 0 && d.red / q >= 8192) c = q;
            if (c) {
                Val part = new_act(Dims{c}, Dims{1});
                PlanOp s1 = op_, s2 = op_;
                s1.name += "/chunks";
                s1.r.out = ref_of(part);
                s1.red.nk = 1; s1.red.ksize[0] = c; s1.red.kin[0] = d.red / c; s1.red.kout[0] = 1; s1.red.kept = c;
                s1.red.rsize[0] = d.red / c; s1.red.red = d.red / c;
                s1.red.bo = plan_.storages[part.storage].elems;
                s1.bytes = 4.0 * (double)(d.red + c);
                s2.r.a = ref_of(part);
                s2.red.rsize[0] = c; s2.red.red = c;
                s2.red.bi = plan_.storages[part.storage].elems;
                s2.bytes = 4.0 * (double)(c + 1);
                push_op(std::move(s1));
                push_op(std::move(s2));
                define(n.outputs[0], out);
                return;
            }
        }
        push_op(std::move(op_));
        define(n.outputs[0], out);
    }

    // Ensure `v` ([C,H,W] or [C,L]) is channels-last contiguous; returns the (possibly copied) value.
    Val to_channels_last(const Val &v, const std::string &why) {
        Dims want(v.dims.size());
        if (v.dims.size() == 3) { want = {1, v.dims[2] * v.dims[0], v.dims[0]}; }
        else { want = {1, v.dims[0]}; }
        if (v.space != Space::INPUT && v.strides_equal(want)) return v;
        if (v.space == Space::INPUT && v.strides_equal(want)) return v;
        return materialize(v, want, why);
    }

    // What a Conv node's attributes and operand shapes fix.  A 1-D conv is the 2-D case with H = kh = 1: stride and dilation 1 and no pad along h.
    struct ConvGeom {
        size_t sp = 0;  // spatial rank
        int64_t H = 0, W = 0, kh = 0, kw = 0;
        std::vector<int64_t> strides, dil;       // {h, w}
        int64_t pt = 0, pl = 0, pb = 0, pr = 0;  // after auto_pad
        int64_t OH = 0, OW = 0;
    };
    ConvGeom conv_geom(const OnnxNode &n, const Val &x, const Val &w, int64_t groups) {
        ConvGeom g;
        const size_t sp = g.sp = x.dims.size() - 1;
        if (sp != 1 && sp != 2) unsupported(n, "only 1-D and 2-D convolutions are supported");
        if (w.dims.size() != sp + 2) unsupported(n, "weight rank mismatch");
        if (w.dims[1] * groups != x.dims[0] || w.dims[0] % groups) unsupported(n, "channel/group mismatch");
        auto get2 = [&](const char *key, int64_t dflt) {
            auto v = n.attr_ints(key);
            if (v.empty()) v.assign(sp, dflt);
            if (v.size() != sp) unsupported(n, std::string(key) + " does not match the spatial rank");
            for (auto e : v) if (e <= 0) unsupported(n, std::string(key) + " must be positive");
            if (sp == 1) v.insert(v.begin(), dflt == 0 ? 0 : 1);
            return v;
        };
        g.H = sp == 2 ? x.dims[1] : 1; g.W = sp == 2 ? x.dims[2] : x.dims[1];
        g.kh = sp == 2 ? w.dims[2] : 1; g.kw = sp == 2 ? w.dims[3] : w.dims[2];
        g.strides = get2("strides", 1); g.dil = get2("dilations", 1);
        std::vector<int64_t> pads = n.attr_ints("pads");
        if (pads.empty()) pads.assign(2 * sp, 0);
        if (pads.size() != 2 * sp) unsupported(n, "pads does not match the spatial rank");
        for (auto e : pads) if (e < 0) unsupported(n, "negative pads");
        if (sp == 2) { g.pt = pads[0]; g.pl = pads[1]; g.pb = pads[2]; g.pr = pads[3]; }
        else { g.pt = g.pb = 0; g.pl = pads[0]; g.pr = pads[1]; }
        const std::string auto_pad = n.attr_s("auto_pad", "NOTSET");
        g.OH = window_out_dim(auto_pad, g.H, (g.kh - 1) * g.dil[0] + 1, g.strides[0], g.pt, g.pb);
        g.OW = window_out_dim(auto_pad, g.W, (g.kw - 1) * g.dil[1] + 1, g.strides[1], g.pl, g.pr);
        if (g.OH <= 0 || g.OW <= 0) unsupported(n, "empty convolution output");
        return g;
    }
    // BatchNormalization with constant statistics as the only reader of `cur`: folded into the filters and the bias, `cur` moves past it
    void fold_batchnorm(std::string &cur, std::vector<float> &wf, std::vector<float> &bias, bool &has_bias) {
        const int64_t Cout = (int64_t)bias.size(), per_out = (int64_t)wf.size() / Cout;
        int c = sole_consumer(cur);
        if (c < 0 || nodes_[c].op_type != "BatchNormalization" || nodes_[c].inputs[0] != cur) return;
        const OnnxNode &bn_ = nodes_[c];
        const Val &sc = get(bn_, 1), &bi = get(bn_, 2), &mu = get(bn_, 3), &var = get(bn_, 4);
        if (!(sc.is_const && bi.is_const && mu.is_const && var.is_const && sc.numel() == Cout)) return;
        float eps = bn_.attr_f("epsilon", 1e-5f);
        for (int64_t o = 0; o < Cout; o++) {
            float s = sc.f[o] / std::sqrt(var.f[o] + eps);
            for (int64_t k = 0; k < per_out; k++) wf[o * per_out + k] *= s;
            bias[o] = (bias[o] - mu.f[o]) * s + bi.f[o];
        }
        has_bias = true;
        absorbed_[c] = true;
        cur = bn_.outputs[0];
    }
    // residual: Add(cur, other) as the only reader of `cur`, with `other` an available activation of identical shape and layout
    bool absorb_residual(std::string &cur, const Dims &out_dims, const Dims &out_strides, Val &res) {
        int c = sole_consumer(cur);
        if (c < 0 || nodes_[c].op_type != "Add") return false;
        const OnnxNode &ad = nodes_[c];
        const std::string &other = ad.inputs[0] == cur ? ad.inputs[1] : ad.inputs[0];
        auto it = vals_.find(other);
        if (it == vals_.end() || it->second.is_const || it->second.dims != out_dims || it->second.space != Space::ARENA || !it->second.strides_equal(out_strides))
            return false;
        res = it->second;
        absorbed_[c] = true;
        cur = ad.outputs[0];
        return true;
    }

    void lower_conv(const OnnxNode &n) {
        Val x = get(n, 0);
        int32_t gate_storage = x.gate_storage;
        x.gate_storage = -1;
        const Val &w = get(n, 1);
        const Val *bptr = opt(n, 2);
        if (x.is_const || !w.is_const || (bptr && !bptr->is_const)) unsupported(n, "Conv needs an activation input and constant weights");
        const int64_t groups = n.attr_i("group", 1);
        ConvGeom geo = conv_geom(n, x, w, groups);
        const size_t sp = geo.sp;
        const int64_t Cin = x.dims[0], Cout = w.dims[0], cpg = w.dims[1];
        const int64_t H = geo.H, kh = geo.kh, kw = geo.kw, OH = geo.OH, OW = geo.OW;
        const std::vector<int64_t> &strides = geo.strides, &dil = geo.dil;

        // ---- epilogue fusion: BatchNorm, activation, residual ----
        std::vector<float> wf = w.f;
        std::vector<float> bias(Cout, 0.0f);
        bool has_bias = bptr != nullptr;
        if (bptr) bias = bptr->f;
        std::string cur = n.outputs[0];
        fold_batchnorm(cur, wf, bias, has_bias);
        ActSpec act;
        absorb_activation(cur, act);
        Dims out_dims = sp == 2 ? Dims{Cout, OH, OW} : Dims{Cout, OW};
        Dims out_strides = sp == 2 ? Dims{1, OW * Cout, Cout} : Dims{1, Cout};
        Val res;
        const bool has_res = absorb_residual(cur, out_dims, out_strides, res);

        Val out = new_act(out_dims, out_strides);
        PlanOp op;
        op.name = "Conv:" + n.name;
        op.r.out = ref_of(out);
        op.macs = (double)OH * OW * Cout * kh * kw * cpg;
        op.weight_bytes = 4.0 * (wf.size() + (has_bias ? Cout : 0));
        op.bytes = 4.0 * ((double)Cin * H * geo.W + (double)Cout * OH * OW * (has_res ? 2 : 1));
        if (has_bias) op.r.bias = Ref{Space::CONSTS, add_const(bias), 0};
        if (has_res) op.r.residual = ref_of(res);

        // the SE gate still pending on x as a launch of its own, where this conv cannot fold it
        auto ungate = [&] {
            if (gate_storage < 0) return;
            Val gx = x;
            gx.gate_storage = gate_storage;
            x = apply_gate(gx, n.name);
            gate_storage = -1;
        };
        bool unit_dil = dil[0] == 1 && dil[1] == 1;
        // a padded 1-D convolution with a long filter (STFT / learned front ends) is worth a padded copy
        // of its input: it then runs as the overlapping-rows GEMM on the matrix cores instead of the
        // direct kernel (Perch-style front end: 14 ms -> GEMM time at batch 128)
        if (groups == 1 && kh == 1 && H == 1 && unit_dil && geo.pt == 0 && geo.pb == 0 && (geo.pl || geo.pr) && kw * Cin >= 64) {
            ungate();
            Dims lo(x.dims.size(), 0), hi(x.dims.size(), 0);
            lo.back() = geo.pl; hi.back() = geo.pr;
            x = pad_copy(x, lo, hi, 0.0f, n.name);
            geo.W += geo.pl + geo.pr;
            geo.pl = geo.pr = 0;
        }
        const int64_t W = geo.W, pt = geo.pt, pl = geo.pl;
        bool no_pad = pt == 0 && pl == 0 && geo.pb == 0 && geo.pr == 0;
        const bool gemm_path = groups == 1 && kh == 1 && unit_dil && no_pad && (H == 1 || (kw == 1 && strides[0] == 1 && strides[1] == 1));
        if (!(gemm_path && kw == 1)) ungate();  // only the 1x1 GEMM folds the SE gate
        if (gemm_path) {
            // GEMM: 1x1 conv (rows = H*W) or 1-D conv as overlapping rows (rows = OW, K = kw*Cin)
            x = to_channels_last(x, n.name);
            if (gate_storage >= 0) {
                op.r.gate = Ref{Space::ARENA, gate_storage, 0};
                op.gemm.has_scale = 1;
                op.gemm.s_bs = plan_.storages[gate_storage].elems;
            }
            op.kind = OpKind::GEMM;
            op.mfma = true;
            GemmDesc &g = op.gemm;
            g.K = (int32_t)(kw * Cin);
            g.N = (int32_t)Cout;
            if (H == 1) { g.rows = OW; g.lda = strides[1] * Cin; }
            else { g.rows = H * W; g.lda = Cin; }
            g.a_bs = batch_stride(x);
            g.ldc = Cout; g.c_bs = plan_.storages[out.storage].elems;
            g.act = act.act; g.p0 = act.p0; g.p1 = act.p1;
            g.has_bias = has_bias; g.has_res = has_res;
            if (has_res) { g.ldr = Cout; g.r_bs = batch_stride(res); }
            // weights [Cout][Cin][kw] -> [Cout][kw][Cin]  (K index = k*Cin + c)
            std::vector<float> wp(wf.size());
            for (int64_t o = 0; o < Cout; o++)
                for (int64_t c = 0; c < Cin; c++)
                    for (int64_t k = 0; k < kw; k++) wp[(o * kw + k) * Cin + c] = wf[(o * Cin + c) * kw + k];
            op.r.a = ref_of(x);
            if (H == 1 && Cin == 1 && !has_res && gate_storage < 0 && fold_framing_conv(n, op, wf, Cout, kw, OW, has_bias)) {
                define(cur, out);
                return;
            }
            op.r.w = Ref{Space::CONSTS, add_const(wp), 0};
        } else if (groups == Cin && cpg == 1 && Cout == Cin) {
            x = to_channels_last(x, n.name);
            if (has_res) {  // depthwise kernel has no residual input: undo that fusion
                unsupported(n, "depthwise convolution followed by a fused residual is not expected");
            }
            op.kind = OpKind::DWCONV;
            DwDesc &d = op.dw;
            d.H = (int32_t)H; d.W = (int32_t)W; d.C = (int32_t)Cin; d.OH = (int32_t)OH; d.OW = (int32_t)OW;
            d.kh = (int32_t)kh; d.kw = (int32_t)kw; d.sh = (int32_t)strides[0]; d.sw = (int32_t)strides[1];
            d.pt = (int32_t)pt; d.pl = (int32_t)pl; d.dh = (int32_t)dil[0]; d.dw = (int32_t)dil[1];
            d.act = act.act; d.p0 = act.p0; d.p1 = act.p1; d.has_bias = has_bias;
            d.in_bs = batch_stride(x); d.out_bs = plan_.storages[out.storage].elems;
            if (Cin % 4 == 0 && Cin / 4 <= 1024 && (kw == 3 || kw == 5) && (strides[1] == 1 || strides[1] == 2) && unit_dil && x.offset % 4 == 0 &&
                d.in_bs % 4 == 0 && d.out_bs % 4 == 0) {
                d.tiled = 1;
                d.tw = 4;
                // pixel tiles per block: up to 1024 lanes, but keep >= 8 blocks per sample; fewer, larger
                // blocks also mean fewer squeeze partials for the SE excite kernel to add up
                const int64_t tiles = OH * ((OW + d.tw - 1) / d.tw);
                d.rpb = (int32_t)std::max<int64_t>(1, std::min<int64_t>(1024 / (Cin / 4), (tiles + 7) / 8));
                d.nblk = (int32_t)((tiles + d.rpb - 1) / d.rpb);
                // small feature maps: one block stages the whole map of 32 channels in LDS (one round of
                // coalesced loads instead of a load-use chain per kernel row) and emits the complete
                // squeeze sums, so the excite kernel adds nothing up
                const bool map_off = !sw_on(sw::BN_DWMAP);
                if (!map_off && kh == kw && strides[0] == strides[1] && H * W <= 768) {
                    d.tiled = 2;
                    d.mapt = sw_int(sw::BN_DWMAPT) != 0 ? 1 : 0;
                    d.nblk = 1;
                }
            }
            std::vector<float> wp(wf.size());  // [C][1][kh][kw] -> [kh][kw][C]
            for (int64_t c = 0; c < Cin; c++)
                for (int64_t k = 0; k < kh * kw; k++) wp[k * Cin + c] = wf[c * kh * kw + k];
            op.r.w = Ref{Space::CONSTS, add_const(wp), 0};
            op.r.a = ref_of(x);
            // ... or, with the launch before it, one fused MBConv launch (mbconv_fuse.cpp)
            if (fuse_mbconv(plan_, op, n.name, sole_consumer(n.inputs[0]) == cur_)) {
                define(cur, out);
                return;
            }
        } else {
            x = to_channels_last(x, n.name);
            op.kind = OpKind::CONV;
            ConvDesc &d = op.conv;
            d.H = (int32_t)H; d.W = (int32_t)W; d.Cin = (int32_t)Cin; d.OH = (int32_t)OH; d.OW = (int32_t)OW; d.Cout = (int32_t)Cout;
            d.kh = (int32_t)kh; d.kw = (int32_t)kw; d.sh = (int32_t)strides[0]; d.sw = (int32_t)strides[1];
            d.pt = (int32_t)pt; d.pl = (int32_t)pl; d.dh = (int32_t)dil[0]; d.dw = (int32_t)dil[1]; d.groups = (int32_t)groups;
            d.act = act.act; d.p0 = act.p0; d.p1 = act.p1; d.has_bias = has_bias; d.has_res = has_res;
            d.in_bs = batch_stride(x); d.out_bs = plan_.storages[out.storage].elems;
            // [Cout][cpg][kh][kw] -> [kh][kw][cpg][Cout]
            std::vector<float> wp(wf.size());
            for (int64_t o = 0; o < Cout; o++)
                for (int64_t c = 0; c < cpg; c++)
                    for (int64_t k = 0; k < kh * kw; k++) wp[(k * cpg + c) * Cout + o] = wf[(o * cpg + c) * kh * kw + k];
            op.r.w = Ref{Space::CONSTS, add_const(wp), 0};
            op.r.a = ref_of(x);
        }
        push_op(std::move(op));
        define(cur, out);
    }

    void lower_matmul(const OnnxNode &n) {
        Val a = get(n, 0);
        const Val &b = get(n, 1);
        bool gemm = n.op_type == "Gemm";
        if (a.is_const || !b.is_const) unsupported(n, "needs an activation left operand and a constant right operand");
        if (b.dims.size() != 2) unsupported(n, "right operand must be a 2-D constant");
        bool transB = gemm && n.attr_i("transB", 0);
        if (gemm && n.attr_i("transA", 0)) unsupported(n, "transA is not supported");
        float alpha = gemm ? n.attr_f("alpha", 1.0f) : 1.0f, beta = gemm ? n.attr_f("beta", 1.0f) : 1.0f;
        int64_t K = transB ? b.dims[1] : b.dims[0], N = transB ? b.dims[0] : b.dims[1];
        if (a.dims.empty() || a.dims.back() != K) unsupported(n, "inner dimensions disagree: " + dims_str(a.dims) + " x " + dims_str(b.dims));
        // A must be row-major contiguous so rows collapse to (rows, K) with lda = K
        if (!a.contiguous()) a = materialize(a, row_major(a.dims), n.name);
        int64_t rows = a.numel() / K;
        std::vector<float> wp((size_t)(N * K));  // [N][K]
        for (int64_t nn = 0; nn < N; nn++)
            for (int64_t k = 0; k < K; k++) wp[nn * K + k] = alpha * (transB ? b.f[nn * K + k] : b.f[k * N + nn]);
        std::vector<float> bias;
        bool has_bias = false;
        if (gemm && has_input(n, 2)) {
            const Val &c = get(n, 2);
            if (!c.is_const) unsupported(n, "Gemm C must be constant");
            if (c.numel() == N) bias = c.f;
            else if (c.numel() == 1) bias.assign(N, c.f[0]);
            else unsupported(n, "Gemm C must broadcast along rows");
            for (auto &v : bias) v *= beta;
            has_bias = true;
        }
        std::string cur = n.outputs[0];
        if (!has_bias) {  // MatMul + Add(const [N])
            int c = sole_consumer(cur);
            if (c >= 0 && nodes_[c].op_type == "Add") {
                const OnnxNode &ad = nodes_[c];
                const std::string &other = ad.inputs[0] == cur ? ad.inputs[1] : ad.inputs[0];
                auto it = vals_.find(other);
                if (it != vals_.end() && it->second.is_const && !it->second.is_int && it->second.numel() == N &&
                    (it->second.dims.empty() || it->second.dims.back() == N)) {
                    bias = it->second.f;
                    has_bias = true;
                    absorbed_[c] = true;
                    cur = ad.outputs[0];
                }
            }
        }
        ActSpec act;
        absorb_activation(cur, act);
        Dims od = a.dims;
        od.back() = N;
        Val out = new_act(od, row_major(od));
        PlanOp op;
        op.kind = OpKind::GEMM;
        op.mfma = true;
        op.name = n.op_type + ":" + n.name;
        op.r.out = ref_of(out);
        op.r.a = ref_of(a);
        op.r.w = Ref{Space::CONSTS, add_const(wp), 0};
        if (has_bias) op.r.bias = Ref{Space::CONSTS, add_const(bias), 0};
        GemmDesc &g = op.gemm;
        g.rows = rows; g.K = (int32_t)K; g.N = (int32_t)N;
        g.lda = K; g.a_bs = batch_stride(a);
        g.ldc = N; g.c_bs = plan_.storages[out.storage].elems;
        g.act = act.act; g.p0 = act.p0; g.p1 = act.p1; g.has_bias = has_bias;
        op.macs = (double)rows * K * N;
        op.weight_bytes = 4.0 * (wp.size() + bias.size());
        op.bytes = 4.0 * ((double)rows * K + (double)rows * N);
        push_op(std::move(op));
        define(cur, out);
    }
};

}  // namespace

bool op_type_mapped(const std::string &t) {
    // the operator types Builder::lower / try_fold dispatch on (keep in step with them: tests/test_host_logic.py plans one node of every
    // type listed here and expects no "outside the native subset" refusal)
    static const std::set<std::string> known = {
        "Constant", "ConstantOfShape", "Range", "Shape", "Identity", "Dropout", "Cast", "Transpose", "Reshape", "Flatten", "Squeeze", "Unsqueeze",
        "Slice", "Concat", "Pad", "Softmax", "LogSoftmax", "Split", "MaxPool", "AveragePool", "Conv", "MatMul", "Gemm", "BatchNormalization",
        "Add", "Sub", "Mul", "Div", "Pow", "Max", "Min", "GlobalAveragePool", "GlobalMaxPool", "ReduceMean", "ReduceSum", "ReduceMax", "ReduceMin",
        "ReduceProd", "ReduceL2", "ReduceSumSquare", "STFT", "DFT", "Expand", "Tile", "PRelu", "InstanceNormalization", "Relu", "Sigmoid", "Tanh",
        "Exp", "Log", "Sqrt", "Abs", "Neg", "Reciprocal", "Floor", "Ceil", "Erf", "Softplus", "HardSwish", "HardSigmoid", "LeakyRelu", "Clip",
        "Greater", "Less", "GreaterOrEqual", "LessOrEqual", "Equal", "Not", "And", "Or", "Xor", "Where", "Gather", "Elu", "Selu", "Celu",
        "ThresholdedRelu", "Softsign", "Mish", "Gelu", "Sign", "Round", "Sum", "Mean", "Size", "ReduceL1", "ReduceLogSum", "ReduceLogSumExp",
        "LayerNormalization"};
    return known.count(t) != 0;
}

IoMeta read_io_meta(const OnnxModel &m) {
    IoMeta io;
    if (!m.inputs.empty()) {
        io.input_name = m.inputs[0].name;
        io.input_shape = m.inputs[0].shape;
        if (!io.input_shape.empty() && io.input_shape[0] <= 0) io.input_shape[0] = -1;
    }
    for (auto &o : m.outputs) {
        io.output_names.push_back(o.name);
        io.output_shapes.push_back(o.shape);
    }
    return io;
}

std::unique_ptr<Plan> build_plan(const OnnxModel &m, const std::vector<int> &wanted_outputs) {
    auto p = std::make_unique<Plan>();
    Builder b(m, *p);
    b.run(wanted_outputs);
    return p;
}

}  // namespace bn
