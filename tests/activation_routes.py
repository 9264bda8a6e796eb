"""Graphs of the per-route activation tests: the eight activations a conv / GEMM epilogue absorbs, in the ONNX forms the planner
absorbs, behind the graph shapes test_gpu_ops.py uses.  No GPU needed to build or plan them."""
import numpy as np

from gpu_helpers import op_graph

# name -> the plan's code (Act, kernels.h)
ACTS = {"relu": 1, "clip": 2, "silu": 4, "hswish": 6, "sigmoid": 3, "hsigmoid": 5, "leaky": 7, "tanh": 8}
MBCONV_SET = ["relu", "clip", "silu", "hswish"]
GEMM_DMA_SET = MBCONV_SET + ["sigmoid", "hsigmoid"]
CONV_SET = GEMM_DMA_SET + ["leaky", "tanh"]
KEEPS_ZERO = [a for a in CONV_SET if a not in ("sigmoid", "hsigmoid")]  # act(0) == 0: what the tiled MBConv kernels need


def act_node(g, y, act):
    if act is None:
        return y
    if act == "silu":
        return g.node("Mul", [y, g.node("Sigmoid", [y])])
    if act == "clip":
        return g.node("Clip", [y, g.const(np.float32(0)), g.const(np.float32(6))])
    op, attrs = {"relu": ("Relu", {}), "hswish": ("HardSwish", {}), "sigmoid": ("Sigmoid", {}), "tanh": ("Tanh", {}),
                 "hsigmoid": ("HardSigmoid", {"alpha": 0.25, "beta": 0.4}), "leaky": ("LeakyRelu", {"alpha": 0.1})}[act]
    return g.node(op, [y], **attrs)


def _map(g, x, cin, h, w):
    i64 = lambda *v: g.const(np.array(v, dtype=np.int64))
    return g.node("Reshape", [g.node("Slice", [x, i64(0), i64(cin * h * w), i64(1), i64(1)]), i64(-1, cin, h, w)])


def _w(rng, *shape):
    return (rng.standard_normal(shape) / np.sqrt(np.prod(shape[1:]))).astype(np.float32)


def _b(rng, n):
    return rng.standard_normal(n).astype(np.float32)


def pointwise(cin, h, w, cout, act):
    """1x1 (brings the map into the channels-last layout) -> the 1x1 conv under test, dense in and out -> 1x1 down to 8 channels"""
    rng = np.random.default_rng(cin + cout)

    def build(g, x):
        y = g.node("Conv", [_map(g, x, cin, h, w), g.const(_w(rng, cin, cin, 1, 1))], kernel_shape=[1, 1])
        y = g.node("Conv", [y, g.const(_w(rng, cout, cin, 1, 1)), g.const(_b(rng, cout))], kernel_shape=[1, 1])
        return g.node("Conv", [act_node(g, y, act), g.const(_w(rng, 8, cout, 1, 1))], kernel_shape=[1, 1])
    return op_graph(build, [8, h, w])


def conv(cin, h, w, cout, k, stride, pad, groups, act):
    rng = np.random.default_rng(cin + cout)
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    def build(g, x):
        y = g.node("Conv", [_map(g, x, cin, h, w), g.const(_w(rng, cout, cin // groups, k, k)), g.const(_b(rng, cout))],
                   kernel_shape=[k, k], strides=[stride] * 2, pads=[pad] * 4, group=groups)
        return act_node(g, y, act)
    return op_graph(build, [cout, oh, ow])


def mbconv(cin, h, w, cmid, k, stride, act, se=False):
    """expand 1x1 + act -> depthwise k x k + act [-> squeeze-excite -> project 1x1, as the small-map kernels' blocks have them]"""
    rng = np.random.default_rng(cin + cmid)
    pad = k // 2
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1

    def build(g, x):
        x = g.node("Conv", [_map(g, x, cin, h, w), g.const(_w(rng, cin, cin, 1, 1))], kernel_shape=[1, 1])
        y = act_node(g, g.node("Conv", [x, g.const(_w(rng, cmid, cin, 1, 1)), g.const(_b(rng, cmid))], kernel_shape=[1, 1]), act)
        z = act_node(g, g.node("Conv", [y, g.const(_w(rng, cmid, 1, k, k)), g.const(_b(rng, cmid))], kernel_shape=[k, k],
                               strides=[stride] * 2, pads=[pad] * 4, group=cmid), act)
        if not se:
            return z
        cr = max(4, cmid // 24)
        e = g.node("GlobalAveragePool", [z])
        e = g.node("Relu", [g.node("Conv", [e, g.const(_w(rng, cr, cmid, 1, 1)), g.const(_b(rng, cr))], kernel_shape=[1, 1])])
        e = g.node("Sigmoid", [g.node("Conv", [e, g.const(_w(rng, cmid, cr, 1, 1)), g.const(_b(rng, cmid))], kernel_shape=[1, 1])])
        return g.node("Conv", [g.node("Mul", [z, e]), g.const(_w(rng, 24, cmid, 1, 1))], kernel_shape=[1, 1])
    return op_graph(build, [24 if se else cmid, oh, ow])
