"""The bf16x3 arithmetic of the matrix kernels, restated in numpy, with its mutants and the statistic the precision tests bound.

The scheme (csrc/bf16x3.h): an f32 operand is the exact sum of three bf16 numbers hi + mid + lo; per 32-deep k step six of the nine
partial products are added to an f32 accumulator in mm6's order (smallest first).  This module is the yardstick of
test_gpu_b3_precision.py: the bound of a case is the geometric mean of what the faithful model and what the weakest broken model
("mutant": one of the three small partial products lost somewhere, or two planes exchanged) give on the SAME operands, so neither factor
of a bound is the code under test.  No GPU, nothing of the product package: plain numpy.
"""
import numpy as np

U24 = 2.0 ** -24

# (weight plane, activation plane) of the six products in mm6's order; planes: 0 = hi, 1 = mid, 2 = lo
TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
TERM_NAMES = ("wl.xh", "wh.xl", "wm.xm", "wm.xh", "wh.xm", "wh.xh")
SMALL_TERMS = (0, 1, 2)   # the products of order 2^-16 |x w|: the ones a loose tolerance does not see
STEP = 32


def top(v):
    """v with the low 16 bits of every f32 cleared: its leading bf16 term."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    return (v.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)


def split(x):
    """x == hi + mid + lo, the expressions of split_bf16x3 (plan_rules.h) / split3 (bf16x3.h)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = top(x)
    r1 = x - hi
    mid = top(r1)
    lo = r1 - mid
    return hi, mid, lo


def n_steps(K):
    return (K + STEP - 1) // STEP


def emulate(X, W, bias=None, drop=None, step=None, swap=None, depth=STEP):
    """X [M, K] times W [N, K] transposed, plus bias, the kernels' way: k steps of 32 ascending, inside a step the six products in mm6's
    order, everything accumulated in f32; the bias joins the finished sum.  depth: k per group of six products (32; the filter bank's
    kernel works in 16-deep groups).

    drop: index into TERMS of a product left out -- in every step, or only in step `step` (an index, or "last": the partial / padded one).
    swap: "w" or "x": that operand's mid and lo planes exchanged (a packer or a split that files a plane in the wrong slot)."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    W = np.ascontiguousarray(W, dtype=np.float32)
    xs, ws = list(split(X)), list(split(W))
    if swap == "x":
        xs[1], xs[2] = xs[2], xs[1]
    elif swap == "w":
        ws[1], ws[2] = ws[2], ws[1]
    else:
        assert swap is None
    M, K = X.shape
    N = W.shape[0]
    nst = (K + depth - 1) // depth
    if step == "last":
        step = nst - 1
    acc = np.zeros((M, N), np.float32)
    for s in range(nst):
        k0, k1 = depth * s, min(depth * (s + 1), K)
        for t, (wi, xi) in enumerate(TERMS):
            if drop == t and (step is None or step == s):
                continue
            acc = acc + (xs[xi][:, k0:k1] @ ws[wi][:, k0:k1].T).astype(np.float32)
    if bias is not None:
        acc = acc + np.asarray(bias, dtype=np.float32)[None, :]
    return acc


def emulate_tile_mutant(faithful, X, W, bias, drop, tile):
    """The faithful result with product `drop` lost in ONE aligned 16 x 16 output tile (row0, col0) only."""
    r0, c0 = tile
    out = faithful.copy()
    b = None if bias is None else np.asarray(bias)[c0:c0 + 16]
    out[r0:r0 + 16, c0:c0 + 16] = emulate(X[r0:r0 + 16], W[c0:c0 + 16], b, drop=drop)
    return out


def reference(X, W, bias=None):
    """(ref, D, dead) in float64: the product itself, D = sum_k |x_k| |w_k| + |b|, the scale every error is measured in, and the outputs
    no product reaches (sum_k |x_k| |w_k| == 0: a dead filter row, an all-zero input row) -- those must equal the bias exactly and take
    no part in the statistic."""
    X64, W64 = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    ref = X64 @ W64.T
    D = np.abs(X64) @ np.abs(W64).T
    dead = D == 0
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)[None, :]
        ref = ref + b
        D = D + np.abs(b)
    return ref, D, dead


def tile_rms_map(Y, ref, D, dead=None):
    """rms of e = (Y - ref) / D over every aligned 16-row x 16-channel block of the output matrix (ragged edge blocks are blocks of their
    own), in units of 2^-24; NaN where a block has no live output.  Also returns the rms over all live outputs."""
    Y, ref, D = np.asarray(Y, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(D, dtype=np.float64)
    live = D > 0 if dead is None else (D > 0) & ~dead
    assert live.any()
    e2 = np.where(live, (Y - ref) / np.where(live, D, 1.0), 0.0) ** 2
    M, N = e2.shape
    Mp, Np = -(-M // 16) * 16, -(-N // 16) * 16
    pad = lambda a: np.pad(a, ((0, Mp - M), (0, Np - N))).reshape(Mp // 16, 16, Np // 16, 16)
    s, c = pad(e2).sum(axis=(1, 3)), pad(live.astype(np.float64)).sum(axis=(1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(s / c) / U24, float(np.sqrt(e2.sum() / live.sum()) / U24)


def statistic(Y, ref, D, dead=None):
    """(rms, worst tile) of e in units of 2^-24: rms over all live outputs, and the largest per-block rms of `tile_rms_map`."""
    tiles, rms = tile_rms_map(Y, ref, D, dead)
    return rms, float(np.nanmax(tiles))


# ---------------------------------------------------------------------------------------------------------------- operands of a case
def dense_inputs(rng, M, K, spread=False):
    """Standard normal activations; spread: every input channel scaled by a power of two out of 2^-20 .. 2^20 (mid / lo exponents vary)."""
    X = rng.standard_normal((M, K)).astype(np.float32)
    if spread:
        X = X * np.exp2(rng.integers(-20, 21, K)).astype(np.float32)[None, :]
    return X


def window_list(K):
    """The 8-channel windows (first channel) a layer is probed with: all of them up to K = 384; beyond that a fixed stratified list -- the
    first step, the half-step / step boundaries next to K / 2 (where a second K slice starts), one window of every fourth step, the last
    two steps whole."""
    allw = list(range(0, K, 8))
    if len(allw) <= 48:
        return allw
    nst = n_steps(K)
    keep = set(range(0, 32, 8))
    half = (K // 2) // 32 * 32
    keep.update(range(half - 32, half + 32, 8))
    keep.update(32 * s + 8 * (s % 4) for s in range(0, nst, 4))
    keep.update(range(max(0, 32 * (nst - 2)), K, 8))
    return sorted(k for k in keep if 0 <= k < K)


def window_inputs(rng, rows, K, windows):
    """One sample (rows x K) per window: standard normal in its 8 channels, zeros elsewhere.  Returns (X [len(windows) * rows, K], the k
    step of every row's window)."""
    X = np.zeros((len(windows), rows, K), np.float32)
    for i, k0 in enumerate(windows):
        X[i, :, k0:k0 + 8] = rng.standard_normal((rows, min(8, K - k0))).astype(np.float32)
    steps = np.repeat(np.array(windows) // STEP, rows)
    return X.reshape(-1, K), steps


# ---------------------------------------------------------------------------------------------------------------- bounds
def _gm(a, b):
    return float(np.sqrt(a * b))


def tile_positions(M, N):
    """The tiles a one-tile fault is tried at: first, middle, last whole tile, and the ragged edge tile where the matrix has one."""
    r = sorted({0, (M // 32) * 16, max(0, (M // 16 - 1) * 16), (M - 1) // 16 * 16})
    c = sorted({0, (N // 32) * 16, max(0, (N // 16 - 1) * 16), (N - 1) // 16 * 16})
    return list(zip(r, c)) if len(r) == len(c) else [(a, b) for a in (r[0], r[-1]) for b in (c[0], c[-1])]


def _result(model, glob, loc, Yf, ref, D, dead):
    wg, wl = min(glob, key=glob.get), min(loc, key=loc.get)
    mutant = (glob[wg], loc[wl])
    return dict(model=model, mutant=mutant, bound=(_gm(model[0], mutant[0]), _gm(model[1], mutant[1])), names=(wg, wl), faithful=Yf, ref=ref, D=D, dead=dead)


def dense_bounds(X, W, bias):
    """Faithful model, weakest mutant and bound, for both statistics, on a dense batch.  rms: against the three small products dropped
    everywhere and the two plane swaps; worst tile: against a small product lost in ONE 16 x 16 tile, the weakest over `tile_positions`.
    Returns dict(model=(rms, tile), mutant=(rms, tile), bound=(rms, tile), names=..., faithful, ref, D, dead)."""
    ref, D, dead = reference(X, W, bias)
    Yf = emulate(X, W, bias)
    model = statistic(Yf, ref, D, dead)
    glob, loc = {}, {}
    for t in SMALL_TERMS:
        glob["drop " + TERM_NAMES[t]] = statistic(emulate(X, W, bias, drop=t), ref, D, dead)[0]
        for tile in tile_positions(*ref.shape):
            loc[f"drop {TERM_NAMES[t]} in tile {tile}"] = statistic(emulate_tile_mutant(Yf, X, W, bias, t, tile), ref, D, dead)[1]
    for sw in ("w", "x"):
        glob["swap mid/lo of " + sw] = statistic(emulate(X, W, bias, swap=sw), ref, D, dead)[0]
    return _result(model, glob, loc, Yf, ref, D, dead)


def step_mutant(Yf, Ydrop, row_step, s):
    """On window inputs every row's products live in ONE k step, so losing a product in step s only gives the rows whose window lies in s
    their drop-everywhere value and leaves every other row alone (test_b3_model_cpu.py proves it against `emulate(step=s)` bit for bit)."""
    return np.where((row_step == s)[:, None], Ydrop, Yf)


def window_bounds(X, row_step, W, bias):
    """The same on a window batch: rms against the small products dropped everywhere, worst tile against a small product dropped in ONE k
    step only -- every step that holds a window, the last (partial) one included; the weakest of all of them."""
    ref, D, dead = reference(X, W, bias)
    Yf = emulate(X, W, bias)
    model = statistic(Yf, ref, D, dead)
    glob, loc = {}, {}
    for t in SMALL_TERMS:
        Yd = emulate(X, W, bias, drop=t)
        glob["drop " + TERM_NAMES[t]] = statistic(Yd, ref, D, dead)[0]
        for s in np.unique(row_step):
            loc[f"drop {TERM_NAMES[t]} in step {int(s)}"] = statistic(step_mutant(Yf, Yd, row_step, s), ref, D, dead)[1]
    return _result(model, glob, loc, Yf, ref, D, dead)


def batches(K, rows, sizes=(5,)):
    """name -> (X, row_step or None), the operands both test files use: dense standard normal batches of the given sizes, one spread over
    2^+-20, the window batch."""
    rng = np.random.default_rng(17 * K + rows)
    out = {}
    for bsz in sizes:
        out[f"dense x{bsz}"] = (dense_inputs(rng, bsz * rows, K), None)
    out["spread x5"] = (dense_inputs(rng, 5 * rows, K, spread=True), None)
    out["windows"] = window_inputs(rng, rows, K, window_list(K))
    return out


def bounds_of(X, row_step, W, bias):
    return dense_bounds(X, W, bias) if row_step is None else window_bounds(X, row_step, W, bias)


# ---------------------------------------------------------------------------------------------------------------- the quarter-folded filter bank
class CosineBank:
    """A bank of windowed cosines as the quarter-fold kernel sees it (kernels.h, GemmDesc::fold == 2): filter row c = a_c win[n] cos(2 pi
    k_c n / L), window symmetric about the frame centre with win[0] = 0.  `taps` [N, L] f32 are the ORIGINAL filters (what the reference and D use);
    the kernel works from factors -- the window tables wa[n] = win[n], wb[n] = win[L/2 - n] (f32; halved at n = 0 for wb, whole at n = L/4
    for wa, zero past it) and the pure cosines a_c cos(.) in f32, K = L/4 + 32 columns, zero past tap L/4 (and at it for odd bins)."""

    def __init__(self, L, bins, amps, win, dead_at=None):
        n = np.arange(L, dtype=np.float64)
        win = np.asarray(win, dtype=np.float64)
        rows = [a * win * np.cos(2.0 * np.pi * k * n / L) for k, a in zip(bins, amps)]
        bins, amps = list(bins), list(amps)
        if dead_at is not None:
            rows.insert(dead_at, np.zeros(L)); bins.insert(dead_at, 0); amps.insert(dead_at, 0.0)
        self.L, self.bins, self.amps = L, np.array(bins), np.array(amps, dtype=np.float64)
        self.taps = np.array(rows, dtype=np.float32)
        Q, K = L // 4, L // 4 + 32
        w32 = (win / win.max()).astype(np.float32)   # (the planner's fitted window is normalised to a maximum of one)
        self.scale = win.max()
        self.wa, self.wb = np.zeros(K, np.float32), np.zeros(K, np.float32)
        self.wa[1:Q + 1] = w32[1:Q + 1]
        self.wb[1:Q] = w32[L // 2 - np.arange(1, Q)]
        self.wb[0] = np.float32(0.5) * w32[L // 2]
        t = np.arange(Q + 1)
        self.wk = np.zeros((len(bins), K), np.float32)
        for c, (k, a) in enumerate(zip(self.bins, self.amps)):
            self.wk[c, :Q + 1] = (a * self.scale * np.cos(2.0 * np.pi * ((k * t) % L) / L)).astype(np.float32)
            if k & 1:
                self.wk[c, Q] = 0.0


def frames_of(x, L, hop):
    """[batch, S] -> [batch frames, L + 1] (the kernel also reads the sample behind a frame, against a table entry of zero)."""
    B, S = x.shape
    nf = (S - L) // hop + 1
    xp = np.concatenate([x, np.zeros((B, 1), x.dtype)], axis=1)
    idx = (np.arange(nf) * hop)[:, None] + np.arange(L + 1)[None, :]
    return xp[:, idx].reshape(B * nf, L + 1), nf


def fold_operands(F, bank):
    """The S | D operand tiles of the kernel in f32: a = x[n] + x[L-n], b = x[L/2-n] + x[L/2+n], S = wa a + wb b, D = wa a - wb b."""
    L, K = bank.L, bank.wa.size
    n = np.arange(K)
    F = np.asarray(F, dtype=np.float32)
    ya = bank.wa[None, :] * (F[:, n] + F[:, L - n])
    yb = bank.wb[None, :] * (F[:, L // 2 - n] + F[:, L // 2 + n])
    return ya + yb, ya - yb


def fold_emulate(F, bank, bias, rows=slice(None), chans=None, **mutant):
    """The bank's output for the frames F, the kernel's way: even bins against S, odd bins against D, 16-deep groups of six products."""
    chans = np.arange(len(bank.bins)) if chans is None else np.asarray(chans)
    S, Dm = fold_operands(F[rows], bank)
    out = np.empty((S.shape[0], chans.size), np.float32)
    odd = (bank.bins[chans] & 1).astype(bool)
    for sel, A in ((~odd, S), (odd, Dm)):
        if sel.any():
            out[:, sel] = emulate(A, bank.wk[chans[sel]], np.asarray(bias)[chans[sel]], depth=16, **mutant)
    return out


def fold_bounds(F, bank, bias):
    """Model, weakest mutant, bound for a filter-bank case: reference and D over the ORIGINAL taps in float64; rms against the small products
    dropped everywhere and the plane swaps, worst tile against a small product lost in one 16-frame x 16-channel tile."""
    ref, D, dead = reference(F[:, :bank.L], bank.taps, bias)
    Yf = fold_emulate(F, bank, bias)
    model = statistic(Yf, ref, D, dead)
    glob, loc = {}, {}
    for t in SMALL_TERMS:
        glob["drop " + TERM_NAMES[t]] = statistic(fold_emulate(F, bank, bias, drop=t), ref, D, dead)[0]
        for r0, c0 in tile_positions(*ref.shape):
            Yt = Yf.copy()
            ch = np.arange(c0, min(c0 + 16, ref.shape[1]))
            Yt[r0:r0 + 16, c0:c0 + 16] = fold_emulate(F, bank, bias, rows=slice(r0, r0 + 16), chans=ch, drop=t)
            loc[f"drop {TERM_NAMES[t]} in tile {(r0, c0)}"] = statistic(Yt, ref, D, dead)[1]
    for sw in ("w", "x"):
        glob["swap mid/lo of " + sw] = statistic(fold_emulate(F, bank, bias, swap=sw), ref, D, dead)[0]
    return _result(model, glob, loc, Yf, ref, D, dead)


def bank_case(which):
    """The `low` (2048 / 278: v2.4's mel-live bins) and `wide` (2048 / 200: five wave columns) banks of the quarter-fold operator test:
    Hann window, scrambled bins, per-row gains and signs, a dead row at position 3, a bias.  Returns (bank, bias, hop)."""
    L, hop = 2048, {"low": 278, "wide": 200}[which]
    rng = np.random.default_rng(L + hop)
    n = np.arange(L, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / L)
    if which == "low":
        bins = np.arange(0, 127)
    else:
        bins = rng.permutation(np.concatenate([rng.permutation(np.arange(0, L // 2 + 1, 2))[:60], rng.permutation(np.arange(1, L // 2, 2))[:90]]))
    amps = [rng.uniform(0.3, 3.0) * rng.choice([-1.0, 1.0]) for _ in bins]
    bank = CosineBank(L, bins, amps, win, dead_at=3)
    return bank, rng.standard_normal(len(bank.bins)).astype(np.float32), hop


BANK_CASES = ["low", "wide"]
BANK_STARTS = [0, 1, 2, 3]   # samples the signal view starts into the segment (0: 16-byte aligned, the float4 span load)
BANK_SAMPLES = 140770        # length of the view: 500 / 694 frames, so two samples end in a ragged row tile of 8 / 12 frames


def bank_signal(which, start, batch=2):
    rng = np.random.default_rng(31 * start + len(which))
    return rng.standard_normal((batch, 144000)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- the cases (shared by the CPU and the GPU test)
# 1x1-conv GEMMs: (K, N, h, w, kernel); rows per sample = h w; batches of 1, 5 and 33 samples
GEMM_BATCHES = (1, 5, 33)
GEMM_CASES = [
    (240, 80, 6, 32, "b3"),      # 15 K steps padded to 16
    (672, 112, 6, 32, "b3"),     # 21 steps + padding steps; seven channel tiles
    (1152, 320, 3, 16, "b3"),    # 48 rows per sample: row tiles span samples
    (136, 816, 8, 32, "b3"),     # K % 16 == 8
    (80, 100, 5, 16, "b3"),      # 80 rows per sample, a partial last channel tile
    (144, 40, 8, 16, "dma3"),    # K % 32 == 16: the half step
    (256, 24, 4, 16, "dma3"),
]
# row-streaming MBConv expand: (Cin, h, w, Cmid, k)
MBROW_CASES = [(16, 7, 9, 40, 3), (24, 12, 40, 144, 3), (24, 13, 37, 144, 5), (40, 9, 19, 240, 3), (40, 9, 19, 240, 5)]
# whole-map MBConv expand: (Cin, h, w, Cmid, k, plan text) -- one shape per configuration of the small-maps test that ends in ,ws / ,b3
MBMAP_CASES = [
    (80, 6, 32, 480, 3, "cfg1,ws "), (112, 6, 32, 600, 3, "cfg2,ws "), (192, 3, 16, 1152, 5, "cfg3,ws "), (192, 4, 16, 1152, 3, "cfg4,ws "),
    (128, 4, 16, 768, 5, "cfg4,ws "),   # K in two slices on the wave-specialised kernel
    (256, 4, 16, 520, 3, "cfg4,b3 "), (80, 8, 32, 480, 3, "cfg5,bands,ws "), (232, 16, 4, 700, 3, "cfg6,transposed,ws kpad=240"),
    (96, 32, 8, 560, 5, "cfg5,bands,transposed,ws kpad=96"), (136, 32, 8, 800, 3, "cfg5,bands,transposed,ws kpad=144"),
]


def case_weights(K, N, seed=0):
    """(W [N, K], bias [N]) of a case: standard normal / sqrt(K), standard normal bias; filter row 5 is dead (all zeros: its outputs are
    the bias, exactly)."""
    rng = np.random.default_rng(1000 * K + N + seed)
    W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    W[5] = 0.0
    return W, rng.standard_normal(N).astype(np.float32)
