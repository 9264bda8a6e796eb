"""float64 restatements of the classifier-head contract (include/birdnet_hip.h, bn_head_*): logits and their error bound, the
fit objective with its gradient and certificate, a per-class Newton solver for the optimum L*, and the fit fixtures."""
import numpy as np

U = 2.0 ** -24


def normalise64(rows):
    """the index's rule in float64: x / sqrt(sum x^2); zero norm, a non-finite element or a sum of squares that overflows f32 -> zeros"""
    x = np.asarray(rows, dtype=np.float64)
    with np.errstate(all="ignore"):
        ss = (x * x).sum(axis=1)
        bad = ~np.isfinite(x).all(axis=1) | ~(ss > 0) | ~(ss < float(np.finfo(np.float32).max))
        out = x / np.sqrt(ss)[:, None]
    out[bad] = 0.0
    return out


def logits64(W, b, rows, l2norm):
    """(logits [n, C], bound [n, C]): z = W xh + b in float64 and 2 (dim + 8) 2^-24 (sum_k |W xh| + |b|)"""
    W = np.asarray(W, dtype=np.float64)
    b = np.zeros(W.shape[0]) if b is None else np.asarray(b, dtype=np.float64)
    xh = normalise64(rows) if l2norm else np.asarray(rows, dtype=np.float64)
    z = xh @ W.T + b
    mag = np.abs(xh) @ np.abs(W).T + np.abs(b)
    return z, 2.0 * (W.shape[1] + 8) * U * mag


def _softplus(u):
    return np.maximum(u, 0.0) + np.log1p(np.exp(-np.abs(u)))


def objective(W, b, X, Y, l2, pos_weight=None):
    """(L, grad W, grad b, certificate |grad|^2 / (2 l2)) at A = [W, b]; X are the head's inputs (already normalised if they are to be)"""
    W, b, X, Y = (np.asarray(a, dtype=np.float64) for a in (W, b, X, Y))
    n, C = Y.shape
    pw = np.ones(C) if pos_weight is None else np.asarray(pos_weight, dtype=np.float64)
    z = X @ W.T + b
    s = 0.5 * (1.0 + np.tanh(0.5 * z))
    loss = (pw * Y * _softplus(-z) + (1 - Y) * _softplus(z)).sum() / n + 0.5 * l2 * ((W * W).sum() + (b * b).sum())
    # pw y (s - 1) + (1 - y) s, with s - 1 written as -1 / (1 + e^z): it keeps its digits for large z
    r = np.where(Y > 0, -pw / (1.0 + np.exp(np.minimum(z, 700.0))), s) / n
    gW = r.T @ X + l2 * W
    gb = r.sum(axis=0) + l2 * b
    gg = (gW * gW).sum() + (gb * gb).sum()
    return loss, gW, gb, gg / (2.0 * l2)


def newton(X, Y, l2, pos_weight=None, iters=60):
    """the optimum by a damped Newton iteration per class (the classes are independent); returns (W, b)"""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    n, d = X.shape
    C = Y.shape[1]
    Xt = np.concatenate([X, np.ones((n, 1))], axis=1)
    pw = np.ones(C) if pos_weight is None else np.asarray(pos_weight, dtype=np.float64)
    A = np.zeros((C, d + 1))

    def f(a, y, p):
        z = Xt @ a
        return (p * y * _softplus(-z) + (1 - y) * _softplus(z)).sum() / n + 0.5 * l2 * (a * a).sum()

    for c in range(C):
        a, y, p = A[c], Y[:, c], pw[c]
        for _ in range(iters):
            z = Xt @ a
            s = 0.5 * (1.0 + np.tanh(0.5 * z))
            r = np.where(y > 0, -p / (1.0 + np.exp(np.minimum(z, 700.0))), s) / n
            g = Xt.T @ r + l2 * a
            if (g * g).sum() / (2 * l2) < 1e-26:
                break
            wgt = np.where(y > 0, p, 1.0) * s * (1 - s) / n
            H = (Xt * wgt[:, None]).T @ Xt + l2 * np.eye(d + 1)
            step = np.linalg.solve(H, g)
            t, f0, slope = 1.0, f(a, y, p), g @ step
            while f(a - t * step, y, p) > f0 - 1e-4 * t * slope and t > 1e-8:
                t *= 0.5
            a = a - t * step
        A[c] = a
    return A[:, :d].copy(), A[:, d].copy()


# (n, dim, C, l2, pos_weight): the fit fixtures
FIXTURES = {
    "n2000_d256_c3": (2000, 256, 3, 1e-3, None),
    "n2000_d256_c3_l2_1e-4_pw4": (2000, 256, 3, 1e-4, 4.0),
    "n4096_d1536_c2": (4096, 1536, 2, 1e-3, None),
}


def fixture(name):
    """(X f32 [n, dim] L2-normalised Gaussian rows with class offsets, Y uint8 [n, C], l2, pos_weight [C] or None)"""
    n, dim, C, l2, pw = FIXTURES[name]
    rng = np.random.default_rng(1000 + n + dim + C)
    centres = rng.standard_normal((C + 1, dim))
    cls = rng.integers(0, C + 1, n)  # one class more than the head has: rows with no positive label
    X = rng.standard_normal((n, dim)) + 0.5 * centres[cls]
    X = (X / np.sqrt((X * X).sum(axis=1, keepdims=True))).astype(np.float32)
    Y = (cls[:, None] == np.arange(C)[None, :])
    Y ^= rng.random((n, C)) < 0.03
    return X, Y.astype(np.uint8), l2, (None if pw is None else np.full(C, pw, dtype=np.float32))
