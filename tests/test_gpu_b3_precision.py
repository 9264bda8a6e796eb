"""The bf16x3 kernels against float64, at the precision they claim (error 2^-24 rms of sum |x||w|, "equal to the exact-f32 kernel's").

Every kernel under test is observed through a path that is exact in any arithmetic that keeps 24 bits -- identity / scaled-permutation
1x1 convs around a GEMM, a centre-tap power-of-two depthwise window behind an MBConv expand (no activation between the two) -- so the graph input IS the activation matrix and the graph output IS the kernel's output, value for value.  Per case:

  * the path is proved first: with a scaled selection matrix in place of the weights the output equals the expected values bit for bit;
  * plan_describe names the kernel meant;
  * e = (got - ref64) / (sum_k |x_k||w_k| + |b|) is summarised as rms over all outputs and as the worst aligned 16 x 16 output tile
    (b3_model.statistic), on dense batches (standard normal; input channels spread over 2^+-20) and on a batch whose samples each carry
    one 8-channel window of the k range (a fault in one k step, half step, padded step or K slice is not averaged away);
  * both numbers must stay below sqrt(faithful model x weakest mutant) -- computed at run time from the same operands by the numpy model
    of the scheme (tests/b3_model.py; test_b3_model_cpu.py shows that bound is >= 4 x above the model and >= 4 x below every mutant) --
    for the bf16x3 form AND for the exact-f32 form the same layer takes under its switch.

The quarter-folded filter bank needs no such path (the signal is the graph input, its output the graph output); its reference and D run
over the original filter taps, its model restates the fold in f32 (b3_model.fold_operands).

Measured statistics are printed (pytest -s) as "B3STAT ..." lines: model, weakest mutant, bound, bf16x3 kernel(s), exact-f32 kernel."""
import os

import numpy as np
import pytest

import b3_model as b3
from gpu_helpers import op_graph, write_model

pytestmark = pytest.mark.gpu

P_OUT, P_SEL = 2.0 ** -2, 2.0 ** 3   # the scales of the observing permutation / window and of the path proof's selection matrix


class Env:
    """Planner switches for the duration of a block (they are read at model load), restored afterwards."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _i64(g, *v):
    return g.const(np.array(v, dtype=np.int64))


def _head(g, xin, cin, h, w):
    """Graph input -> [B, cin, h, w] -> identity 1x1 conv (brings the map into the channels-last layout the kernels read)."""
    y = g.node("Reshape", [g.node("Slice", [xin, _i64(g, 0), _i64(g, cin * h * w), _i64(g, 1), _i64(g, 1)]), _i64(g, -1, cin, h, w)])
    return g.node("Conv", [y, g.const(np.eye(cin, dtype=np.float32).reshape(cin, cin, 1, 1))], kernel_shape=[1, 1])


def _perm(n):
    return np.random.default_rng(n).permutation(n)


def gemm_graph(cin, h, w, cout, W, bias):
    """Slice/Reshape -> Conv(eye) -> the conv under test -> Conv(P), out[o] = 2^-2 y[perm[o]]."""
    perm = _perm(cout)
    P = np.zeros((cout, cout), np.float32)
    P[np.arange(cout), perm] = P_OUT

    def build(g, xin):
        y = _head(g, xin, cin, h, w)
        y = g.node("Conv", [y, g.const(W.reshape(cout, cin, 1, 1)), g.const(bias)], kernel_shape=[1, 1])
        return g.node("Conv", [y, g.const(P.reshape(cout, cout, 1, 1))], kernel_shape=[1, 1])
    return op_graph(build, [cout, h, w]), perm


def mb_graph(cin, h, w, cmid, k, W, bias):
    """Slice/Reshape -> Conv(eye) -> the expand under test, no activation -> depthwise k x k: centre tap 2^-2, zero bias, stride 1.  The
    planner fuses the pair without an activation between them (and without a squeeze-excite behind them) for the row kernel and for
    every whole-map configuration alike, so the fused launch's output is the expand's output times 2^-2."""
    wd = np.zeros((cmid, 1, k, k), np.float32)
    wd[:, 0, k // 2, k // 2] = P_OUT

    def build(g, xin):
        y = _head(g, xin, cin, h, w)
        y = g.node("Conv", [y, g.const(W.reshape(cmid, cin, 1, 1)), g.const(bias)], kernel_shape=[1, 1])
        return g.node("Conv", [y, g.const(wd), g.const(np.zeros(cmid, np.float32))], kernel_shape=[k, k], strides=[1, 1], pads=[k // 2] * 4, group=cmid)
    return op_graph(build, [cmid, h, w])


def selection(N, K):
    """The path proof's stand-in for the weights: output channel n = 2^3 x input channel (7 n + 3) mod K; zero bias."""
    sel = (7 * np.arange(N) + 3) % K
    W = np.zeros((N, K), np.float32)
    W[np.arange(N), sel] = P_SEL
    return W, np.zeros(N, np.float32), sel


def to_input(X, batch, rows, K):
    """The activation matrix [batch rows, K] as graph input: sample b = its [K, rows] map, flattened, zeros behind."""
    x = np.zeros((batch, 144000), np.float32)
    x[:, :K * rows] = X.reshape(batch, rows, K).transpose(0, 2, 1).reshape(batch, -1)
    return x


def run_matrix(bn, path, X, rows, K, N, perm, scale):
    """The kernel's output matrix [batch rows, N] for the activation matrix X, the observing scale / permutation undone (exactly)."""
    batch = X.shape[0] // rows
    out = bn.Context(bn.Model(path), batch).infer(to_input(X, batch, rows, K))[0].reshape(batch, N, rows).transpose(0, 2, 1).reshape(-1, N)
    out = out.astype(np.float32) / np.float32(scale)
    if perm is None:
        return out
    Y = np.empty_like(out)
    Y[:, perm] = out
    return Y


class Report:
    """Collects 'statistic <= bound' checks so that every figure of a case is printed before the first failure is raised."""

    def __init__(self, case):
        self.case, self.failures = case, []

    def bounds(self, batch_name, r):
        assert r["mutant"][0] >= 16.0 * r["model"][0] and r["mutant"][1] >= 16.0 * r["model"][1], (self.case, batch_name, r["model"], r["mutant"], r["names"])
        print(f"B3STAT {self.case} [{batch_name}] model rms {r['model'][0]:.3f} tile {r['model'][1]:.3f} | weakest mutant rms {r['mutant'][0]:.2f} ({r['names'][0]}) "
              f"tile {r['mutant'][1]:.2f} ({r['names'][1]}) | bound rms {r['bound'][0]:.3f} tile {r['bound'][1]:.3f}   (units 2^-24 D)")

    def check(self, batch_name, form, Y, r, bias):
        dead = r["dead"]
        assert np.array_equal(Y[dead], np.broadcast_to(bias[None, :], Y.shape)[dead]), f"{form}: a dead output is not the bias"
        rms, tile = b3.statistic(Y, r["ref"], r["D"], dead)
        ok = rms <= r["bound"][0] and tile <= r["bound"][1]
        print(f"B3STAT {self.case} [{batch_name}] {form}: rms {rms:.3f} tile {tile:.3f}  {'ok' if ok else 'EXCEEDS the bound'}")
        if not ok:
            tm = b3.tile_rms_map(Y, r["ref"], r["D"], dead)[0]
            worst = np.argwhere(np.nan_to_num(tm) > r["bound"][1])[:12]
            self.failures.append(f"[{batch_name}] {form}: rms {rms:.3f} (bound {r['bound'][0]:.3f}) worst tile {tile:.3f} (bound {r['bound'][1]:.3f}); "
                                 f"tiles over the bound (row tile, channel tile): {worst.tolist()} of {tm.shape}")

    def finish(self):
        assert not self.failures, f"{self.case}:\n" + "\n".join(self.failures)


def prove_path(run, K, N, rows):
    """`run(X)` on the graph whose weights are `selection(N, K)`: the output is 2^3 x the selected input channel, bit for bit -- on values
    with full 24-bit significands and exponents spread over 2^+-20."""
    rng = np.random.default_rng(3)
    X = b3.dense_inputs(rng, 3 * rows, K, spread=True)
    got = run(X)
    want = X[:, selection(N, K)[2]] * np.float32(P_SEL)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), "the observing path is not exact"


def plan_line(text, needle):
    lines = [l for l in text.splitlines() if needle in l]
    assert len(lines) == 1, (needle, text)
    return lines[0]


def matrix_case(bn, case, forms, base, check_plan, path, proof, K, N, rows, sizes, perm=None):
    """What the three matrix families share.  forms: [(name, planner switches)], the exact-f32 form last; check_plan(form, plan text).  For
    every form: the plan names the kernel (on the graph under test and on the path proof's), the path is exact; then, per batch of
    b3_model.batches: model, weakest mutant (>= 16 x the model), and rms / worst tile of every form against the bound.  Dead outputs
    (filter row 5) are the bias exactly."""
    W, bias = b3.case_weights(K, N)
    run = lambda p, X: run_matrix(bn, p, X, rows, K, N, perm, P_OUT)
    for form, env in forms:
        with Env(**base), Env(**env):
            for p in (path, proof):
                check_plan(form, bn.plan_describe(p))
            prove_path(lambda X: run(proof, X), K, N, rows)
    rep = Report(case)
    for name, (X, row_step) in b3.batches(K, rows, sizes).items():
        r = b3.bounds_of(X, row_step, W, bias)
        assert r["dead"].sum() == r["dead"][:, 5].sum() == X.shape[0]   # the dead filter row: one row, nothing else
        rep.bounds(name, r)
        for form, env in forms:
            with Env(**base), Env(**env):
                rep.check(name, form, run(path, X), r, bias)
    rep.finish()


# ---------------------------------------------------------------------------------------------------------------- 1x1-conv GEMMs
@pytest.mark.parametrize("K,N,h,w,kernel", b3.GEMM_CASES)
def test_gemm_b3_and_dma3_against_float64(bn, K, N, h, w, kernel):
    """gemm_b3_kernel (every row-tile height: BN_GEMMB3_MT 2 / 3 / 4) and gemm_dma3_kernel (one and two K slices: BN_GEMM3_KS), batches of
    1, 5 and 33 samples (row tiles that span samples, a ragged last tile), and the exact-f32 kernel of the same layer (BN_GEMM3=0)."""
    W, bias = b3.case_weights(K, N)
    data, perm = gemm_graph(K, h, w, N, W, bias)
    Ws, bs, _ = selection(N, K)
    forms = [(f"b3 MT={mt}", dict(BN_GEMMB3_MT=mt)) for mt in (2, 3, 4)] if kernel == "b3" else [(f"dma3 KS={ks}", dict(BN_GEMM3_KS=ks)) for ks in (1, 2)]
    forms.append(("exact f32", dict(BN_GEMM3=0)))

    def check_plan(form, text):
        line = plan_line(text, f" K={K} N={N} ")
        assert (f"kernel={kernel}" in line) == (form != "exact f32") and ("kernel=b3" in line or "kernel=dma3" in line) == (form != "exact f32"), line
    matrix_case(bn, f"{kernel} K={K} N={N} rows={h * w}", forms, {}, check_plan, write_model(data), write_model(gemm_graph(K, h, w, N, Ws, bs)[0]),
                K, N, h * w, b3.GEMM_BATCHES, perm)


# ---------------------------------------------------------------------------------------------------------------- row-streaming MBConv expand
@pytest.mark.parametrize("cin,h,w,cmid,k", b3.MBROW_CASES)
def test_mbrow_expand_against_float64(bn, cin, h, w, cmid, k):
    """mbrow.hip's expand on the bf16 pipe (one to five 8-channel K groups, 3 x 3 and 5 x 5 windows, bands of 5 rows with a ragged last
    one, the transposed walk for 3 x 3), no activation between expand and window; its exact-f32 form under BN_MBROW_B3=0."""
    assert h % 5, "the last band is meant to be ragged"
    W, bias = b3.case_weights(cin, cmid)
    Ws, bs, _ = selection(cmid, cin)
    base = dict(BN_MBFUSE="force", BN_MBMAP=0, BN_MBPIPE=0, BN_MBROW="force", BN_MBROW_TOH=5, BN_MBROW_TR=0)
    forms = [("row_b3", {})] + ([("row_b3 transposed", dict(BN_MBROW_TR=1))] if k == 3 else []) + [("exact f32", dict(BN_MBROW_B3=0))]

    def check_plan(form, text):
        line = plan_line(text, " MBCONV ")
        assert (" row_b3 " in line) == (form != "exact f32") and "rows=5" in line and ("(columns)" in line) == ("transposed" in form), line
    matrix_case(bn, f"mbrow Cin={cin} Cmid={cmid} {h}x{w} k={k}", forms, base, check_plan, write_model(mb_graph(cin, h, w, cmid, k, W, bias)),
                write_model(mb_graph(cin, h, w, cmid, k, Ws, bs)), cin, cmid, h * w, (5,))


# ---------------------------------------------------------------------------------------------------------------- whole-map MBConv expand
@pytest.mark.parametrize("cin,h,w,cmid,k,expect", b3.MBMAP_CASES)
def test_mbmap_expand_against_float64(bn, cin, h, w, cmid, k, expect):
    """mbmap_ws.hip (wave-specialised) and mbmap.hip's bf16x3 form (BN_MBMAP_WS=0 where the configuration has one), one shape per
    configuration: cfg1 - cfg6, bands, transposed maps, K padded to 240 / 144 in LDS, K in two slices (both kernels), ragged channel
    counts; no activation between expand and window.  The exact-f32 form: BN_MBMAP_B3=0 (mbmap.hip's f32 expand, or -- bands, cfg6 -- the
    unfused layer, then with BN_GEMM3=0 so that its GEMM is the f32 one too)."""
    W, bias = b3.case_weights(cin, cmid)
    path = write_model(mb_graph(cin, h, w, cmid, k, W, bias))
    Ws, bs, _ = selection(cmid, cin)
    first = expect.split()[0]
    forms = [(first, {})]
    with Env(BN_MBMAP_WS=0):
        if ",ws" in first and "map=" + first.replace(",ws", ",b3") + " " in bn.plan_describe(path):
            forms.append((first.replace(",ws", ",b3"), dict(BN_MBMAP_WS=0)))
    assert len(forms) == 2 or ",b3" in first or "bands" in first or "cfg6" in first, forms   # cfg1 - cfg4: both bf16x3 kernels
    with Env(BN_MBMAP_B3=0):
        fused_f32 = "MBCONV" in bn.plan_describe(path)
    assert fused_f32 == (len(forms) == 2 or ",b3" in first)
    forms.append(("exact f32", dict(BN_MBMAP_B3=0) if fused_f32 else dict(BN_MBMAP_B3=0, BN_GEMM3=0)))

    def check_plan(form, text):
        if form == "exact f32":
            line = plan_line(text, " MBCONV " if fused_f32 else f" K={cin} N={cmid} ")
            assert ",ws" not in line and ",b3" not in line and "kernel=b3" not in line and "kernel=dma3" not in line and " row_b3 " not in line, text
        else:
            assert ("map=" + (expect if form == first else form + " ")) in plan_line(text, " MBCONV ") + " ", text
    matrix_case(bn, f"mbmap {first} Cin={cin} Cmid={cmid} {h}x{w} k={k}", forms, {}, check_plan, path, write_model(mb_graph(cin, h, w, cmid, k, Ws, bs)),
                cin, cmid, h * w, (5,))


# ---------------------------------------------------------------------------------------------------------------- quarter-folded filter bank
def bank_graph(start, taps, bias, hop):
    """Graph input -> the view [start, start + BANK_SAMPLES) -> Conv1d: the signal is the graph input, the bank's output the graph output."""
    frames = (b3.BANK_SAMPLES - taps.shape[1]) // hop + 1

    def build(g, x):
        x = g.node("Slice", [x, _i64(g, start), _i64(g, start + b3.BANK_SAMPLES), _i64(g, 1), _i64(g, 1)])
        u = g.node("Unsqueeze", [x, _i64(g, 1)])
        return g.node("Conv", [u, g.const(np.ascontiguousarray(taps[:, None, :])), g.const(bias)], kernel_shape=[taps.shape[1]], strides=[hop])
    return op_graph(build, [taps.shape[0], frames])


@pytest.mark.parametrize("which", b3.BANK_CASES)
def test_quarter_folded_filter_bank_against_float64(bn, which, monkeypatch):
    """frame_fold2q_kernel (the quarter fold on the bf16 pipe) on the `low` and `wide` banks, the signal view aligned and 1 - 3 samples
    into the segment (the scalar span load), two samples (a ragged last row tile); reference and D over the ORIGINAL 2048 taps in float64.
    The exact-f32 forms under BN_FRAME2_B3=0: both block heights (frame_fold2p, and frame_fold2 with BN_FRAME2_WPK=0).  The dead filter
    row's outputs are the bias, exactly, and the only dead outputs."""
    monkeypatch.setenv("BN_STFT", "0")   # (the default would decide FFT / matrix product per bank by estimated cost)
    bank, bias, hop = b3.bank_case(which)
    N, L = bank.taps.shape
    forms = [("frame_fold2q", {}, "kernel=frame_fold2q"), ("exact f32, half height", dict(BN_FRAME2_B3=0), "kernel=frame_fold2p"),
             ("exact f32, 64 rows", dict(BN_FRAME2_B3=0, BN_FRAME2_WPK=0), "kernel=frame_fold2 ")]
    rep = Report(f"frame_fold2 {which} 2048/{hop}")
    for start in b3.BANK_STARTS:
        path = write_model(bank_graph(start, bank.taps, bias, hop))
        x = b3.bank_signal(which, start)
        F, nf = b3.frames_of(x[:, start:start + b3.BANK_SAMPLES], L, hop)
        run = lambda p: bn.Context(bn.Model(p), 2).infer(x)[0].reshape(2, -1, nf).transpose(0, 2, 1).reshape(2 * nf, -1).astype(np.float32)
        # the path: delta filters (tap 13 c mod L of channel c, times 2^3) in place of the bank pick samples of the view, bit for bit
        sel = (13 * np.arange(N)) % L
        delta = np.zeros((N, L), np.float32)
        delta[np.arange(N), sel] = P_SEL
        got = run(write_model(bank_graph(start, delta, np.zeros(N, np.float32), hop)))
        assert np.array_equal(got.view(np.uint32), (F[:, sel] * np.float32(P_SEL)).view(np.uint32)), "the observing path is not exact"
        r = b3.fold_bounds(F, bank, bias)
        assert r["dead"].sum() == r["dead"][:, 3].sum() == F.shape[0]
        rep.bounds(f"start {start}", r)
        for form, env, needle in forms:
            with Env(**env):
                text = bn.plan_describe(path)
                assert "~quarter" in text and any(needle in l + " " for l in text.splitlines()) and f"fold=2/{L}" in text, text
                rep.check(f"start {start}", form, run(path), r, bias)
    rep.finish()
