"""Every kernel route applies every activation of its set (kernels.h, ACT_SET_*): one launch-carried activation per case, against the
oracle, with proof that the case could not pass had the kernel dropped the activation.

Per case: (1) plan_describe names the intended route and the activation rides in THAT launch -- `act=<code>` on its GEMM / CONV / DWCONV
line; the MBCONV line prints no activation field, so there every other launch of the plan must carry none (an ELT, GEMM or DWCONV
beside it would show its code); (2) the result agrees with the oracle under the suite's tolerance (the bf16x3 GEMMs: 2e-5 max|ref|, as
test_gemm_bf16x3_forms_...); (3) the oracle's output of the same graph WITHOUT the activation node differs from the reference by more
than 100 tolerances in at least 10 % of the elements -- a property of the inputs, checked on the CPU.

The tiled MBConv kernels need act(0) == 0 of their activation (pixels outside the image expand to zeros): the planner keeps Sigmoid and
HardSigmoid out of them, and out of the row-streaming form everything outside its set -- those cases pin that refusal (no MBCONV launch
with the route's marks) and still check the result."""
import re

import numpy as np
import pytest

from oracle import onnx_ref
from gpu_helpers import ATOL, RTOL, assert_close, write_model
import activation_routes as R

pytestmark = pytest.mark.gpu

_MB = (16, 7, 9, 40, 3, 1)     # test_fused_expand_depthwise's smallest block, with its switches
_SMALL = (80, 6, 32, 40, 3, 2)  # test_fused_expand_depthwise_small_maps: the smallest block the wave-specialised kernel takes


def _mb_env(variant):
    return {"BN_MBFUSE": "force", "BN_MBMAP": "1" if variant == "map" else "0", "BN_MBMAP_MAXHW": "1024", "BN_MBPIPE": "1" if variant == "pipe" else "0",
            "BN_MBROW": "force" if variant == "row" else "0", "BN_MBROW_TOH": "5", "BN_MBROW_TR": "0"}


# route -> (graph(act), switches, the launch's line: kind and the marks it must show, activations, fused for, bf16x3 bound)
ROUTES = {
    "gemm-tiled-8x7": (lambda a: R.pointwise(8, 3, 5, 7, a), {}, ("GEMM", [" K=8 N=7 ", "kernel=tiled"]), R.CONV_SET, R.CONV_SET, False),
    "gemm-tiled-13x130": (lambda a: R.pointwise(13, 4, 6, 130, a), {}, ("GEMM", [" K=13 N=130 ", "kernel=tiled"]), R.CONV_SET, R.CONV_SET, False),
    # (K = 320, 48 rows per sample; BN_GEMM3=0 as well: by default the register-staged bf16x3 GEMM takes this shape for the codes of its set)
    "gemm-splitk": (lambda a: R.pointwise(320, 3, 16, 128, a), {"BN_GEMMDMA": "0", "BN_GEMM3": "0"}, ("GEMM", [" K=320 N=128 ", "kernel=splitk"]),
                    R.CONV_SET, R.CONV_SET, False),
    "gemm-dma": (lambda a: R.pointwise(144, 8, 16, 40, a), {"BN_GEMM3": "0"}, ("GEMM", [" K=144 N=40 ", "kernel=dma "]), R.GEMM_DMA_SET, R.GEMM_DMA_SET, False),
    "gemm-dma3": (lambda a: R.pointwise(144, 8, 16, 40, a), {}, ("GEMM", [" K=144 N=40 ", "kernel=dma3"]), R.GEMM_DMA_SET, R.GEMM_DMA_SET, True),
    "gemm-b3": (lambda a: R.pointwise(80, 5, 16, 100, a), {}, ("GEMM", [" K=80 N=100 ", "kernel=b3"]), R.GEMM_DMA_SET, R.GEMM_DMA_SET, True),
    "conv-direct": (lambda a: R.conv(2, 20, 31, 32, 3, 2, 1, 1, a), {}, ("CONV", ["20x31x2->10x16x32"]), R.CONV_SET, R.CONV_SET, False),
    "conv-small": (lambda a: R.conv(3, 20, 31, 8, 3, 1, 1, 1, a), {}, ("CONV", ["20x31x3->20x31x8"]), R.CONV_SET, R.CONV_SET, False),
    "dwconv-plain": (lambda a: R.conv(8, 5, 5, 8, 7, 1, 3, 8, a), {}, ("DWCONV", ["k=7x7", "tiled=0"]), R.CONV_SET, R.CONV_SET, False),
    "dwconv-tiled": (lambda a: R.conv(32, 24, 30, 32, 3, 1, 1, 32, a), {}, ("DWCONV", ["k=3x3", "tiled=2"]), R.CONV_SET, R.CONV_SET, False),
    "mbconv-tiled": (lambda a: R.mbconv(*_MB, a), _mb_env("tiled"), ("MBCONV", ["rows=0"]), R.CONV_SET, R.KEEPS_ZERO, False),
    "mbconv-pipe": (lambda a: R.mbconv(*_MB, a), _mb_env("pipe"), ("MBCONV", ["rows=0"]), R.CONV_SET, R.KEEPS_ZERO, False),
    "mbconv-map": (lambda a: R.mbconv(*_MB, a), _mb_env("map"), ("MBCONV", ["tiles=1x1", "rows=0"]), R.CONV_SET, R.CONV_SET, False),
    "mbconv-row": (lambda a: R.mbconv(*_MB, a), _mb_env("row"), ("MBCONV", ["rows=5"]), R.MBCONV_SET, R.MBCONV_SET, False),
    "mbmap": (lambda a: R.mbconv(*_SMALL, a, se=True), {"BN_MBMAP_WS": "0"}, ("MBCONV", ["map=cfg1,b3 "]), R.MBCONV_SET, R.MBCONV_SET, False),
    "mbmap-ws": (lambda a: R.mbconv(*_SMALL, a, se=True), {}, ("MBCONV", ["map=cfg1,ws "]), R.MBCONV_SET, R.MBCONV_SET, False),
}
CASES = [(route, act) for route, spec in ROUTES.items() for act in spec[3]]


def _act_fields(line):
    return [int(v) for v in re.findall(r"\bact\d?=(\d+)", line)]


@pytest.mark.parametrize("route,act", CASES, ids=[f"{r}-{a}" for r, a in CASES])
def test_route_applies_activation(bn, route, act, monkeypatch):
    graph, env, (kind, marks), _, fused_for, b3 = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    data, code = graph(act), R.ACTS[act]
    path = write_model(data)
    text = bn.plan_describe(path)
    launches = [l + " " for l in text.splitlines() if re.match(r"\s*\d+ [A-Z]+ ", l)]
    mine = [l for l in launches if f" {kind} " in l and all(m in l for m in marks)]
    if act not in fused_for:
        assert not any(" MBCONV " in l for l in launches), text
    else:
        assert len(mine) == 1, text
        if kind == "MBCONV":
            assert all(v == 0 for l in launches if l is not mine[0] and " SEFC " not in l for v in _act_fields(l)), text
        else:
            assert _act_fields(mine[0]) == [code], text
            assert all(v == 0 for l in launches if l is not mine[0] for v in _act_fields(l)), text
    x = np.random.default_rng(0).standard_normal((3, 144000)).astype(np.float32)
    ref = onnx_ref.run_model(data, x)["output"]
    bare = onnx_ref.run_model(graph(None), x)["output"]
    got = bn.Context(bn.Model(path), 4).infer(x)[0].reshape(ref.shape)
    scale = float(np.abs(ref).max())
    lim = 2e-5 * scale if b3 else ATOL + RTOL * np.abs(ref.astype(np.float64))
    dropped = np.abs(bare.astype(np.float64) - ref.astype(np.float64)) > 100 * lim
    print(f"{route} {act}: max err {np.abs(got - ref).max():.3e}, scale {scale:.3e}, {dropped.mean():.1%} of the elements tell a dropped activation")
    assert dropped.mean() >= 0.10, f"the inputs do not tell {act} from the identity: {dropped.mean():.1%}"
    if b3:
        assert np.abs(got - ref).max() <= lim, (np.abs(got - ref).max(), scale)
    else:
        assert_close(got, ref, f"{route} {act}")
