"""The per-site species prior contract (include/birdnet_hip.h, bn_prior_*) stated in numpy, independent of the product.

For logit z of species j in a row at site s, with p = P[s][j]:
    admitted = p < 0 or p >= threshold
    conf     = oracle.sigmoid(z)
    conf'    = np.float32(conf) * np.float32(p) when reranking and p >= 0, else conf
SELECT:      the first K = min(top_k, n) admitted species sorted by (conf' descending under total_cmp, index ascending): np.lexsort on
             (index, -key); with a minimum, the entries where conf' >= min_conf fails (NaN fails) are then removed.
AFTER_TOPK:  oracle.top_k, then: drop what is not admitted, multiply when reranking, stable descending total_cmp sort when reranking
             (rangefilter.rs:333-386 with species matched by index)."""
import numpy as np

import oracle

UNKNOWN = np.float32(-1.0)


def total_key(x):
    """f32::total_cmp as an unsigned key, as int64."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(b & 0x80000000, b ^ 0xFFFFFFFF, b | 0x80000000)


def sigmoid_row(logits):
    """oracle.sigmoid of every element (one call per distinct bit pattern)."""
    a = np.ascontiguousarray(logits, dtype=np.float32).reshape(-1)
    u, inv = np.unique(a.view(np.uint32), return_inverse=True)
    vals = np.array([oracle.sigmoid(float(v)) for v in u.view(np.float32)], dtype=np.float32)
    # float(np.float32 NaN) -> c_float keeps the sign and the quiet payload; the result comes back the same way
    return vals[inv]


def conf_prime(conf, p, rerank):
    conf = np.asarray(conf, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    if not rerank:
        return conf.copy()
    with np.errstate(all="ignore"):
        prod = (conf * p).astype(np.float32)
    return np.where(p >= 0, prod, conf).astype(np.float32)


def admitted(p, threshold):
    p = np.asarray(p, dtype=np.float32)
    return (p < 0) | (p >= np.float32(threshold))


def select_row(conf, prow, threshold, rerank, top_k, min_conf=None):
    """conf: the row's sigmoids.  Returns (indices, confidences)."""
    n = len(conf)
    cp = conf_prime(conf, prow, rerank)
    cand = np.nonzero(admitted(prow, threshold))[0]
    order = np.lexsort((cand, -total_key(cp[cand])))
    sel = cand[order][:min(int(top_k), n)]
    c = cp[sel]
    if min_conf is not None:
        with np.errstate(invalid="ignore"):
            keep = c >= np.float32(min_conf)
        sel, c = sel[keep], c[keep]
    return sel.astype(np.uint32), c.astype(np.float32)


def filter_row(idx, conf, prow, threshold, rerank):
    """The filter rule over one prediction list given by species index."""
    idx = np.asarray(idx, dtype=np.int64)
    conf = np.asarray(conf, dtype=np.float32)
    p = np.asarray(prow, dtype=np.float32)[idx] if len(idx) else np.zeros(0, dtype=np.float32)
    keep = admitted(p, threshold)
    c = conf_prime(conf, p, rerank)[keep]
    i = idx[keep]
    if rerank:
        order = np.argsort(-total_key(c), kind="stable")
        i, c = i[order], c[order]
    return i.astype(np.uint32), c.astype(np.float32)


def after_topk_row(logits, prow, threshold, rerank, top_k, min_conf=None):
    tk = oracle.top_k(np.ascontiguousarray(logits, dtype=np.float32), top_k, min_conf)
    return filter_row([t[0] for t in tk], np.array([t[1] for t in tk], dtype=np.float32), prow, threshold, rerank)


def apply(logits, table, sites, threshold, top_k, min_conf=None, after_topk=False, rerank=False, conf=None):
    """Rows packed as bn_prior_apply_host packs them: (idx [rows, K], conf [rows, K], count [rows]), zeros past each count.
    conf: sigmoid_row of the logits, if the caller has it already (SELECT only)."""
    x = np.ascontiguousarray(logits, dtype=np.float32)
    rows, n = x.shape
    k = max(min(int(top_k), n), 1)
    idx = np.zeros((rows, k), dtype=np.uint32)
    cf = np.zeros((rows, k), dtype=np.float32)
    cnt = np.zeros(rows, dtype=np.uint32)
    if conf is None and not after_topk:
        conf = sigmoid_row(x).reshape(rows, n)
    for r in range(rows):
        prow = table[int(sites[r])]
        i, c = after_topk_row(x[r], prow, threshold, rerank, top_k, min_conf) if after_topk else select_row(conf[r], prow, threshold, rerank, top_k, min_conf)
        idx[r, :len(i)], cf[r, :len(i)], cnt[r] = i, c, len(i)
    return idx, cf, cnt
