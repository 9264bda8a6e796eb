"""The selection of bn_head_rank_index restated in numpy: given the logits of every (row, class), which rows are eligible and the
order, the lists the call must return.  It computes no logit itself; the GPU tests feed it bn_head_apply_host's logits of the stored
rows (code older than the ranking), so ids, counts and logit bytes can be compared with ==.

  eligible   inside [first_id, first_id + n_ids) (n_ids == 0: to the end), valid, not excluded, logit not NaN
  "top"        z descending, ties by id ascending (-0.0 == +0.0)
  "uncertain"  |z| ascending, ties by id ascending (z and -z tie)
Pure numpy; shared by test_rank_cpu.py (which checks it against a brute-force sort) and test_gpu_rank.py."""
import numpy as np

TOP, UNCERTAIN = 0, 1
_MODES = {"top": TOP, "uncertain": UNCERTAIN, TOP: TOP, UNCERTAIN: UNCERTAIN}


def eligible(Z, valid, first_id=0, n_ids=0, exclude=None):
    """bool [n, classes]"""
    Z = np.asarray(Z)
    n = Z.shape[0]
    row = np.asarray(valid, dtype=bool).reshape(n).copy()
    last = n if n_ids == 0 else first_id + n_ids
    if first_id > n or last > n:
        raise ValueError("range past the end")
    row[:first_id] = False
    row[last:] = False
    if exclude is not None and len(exclude):
        row[np.asarray(exclude, dtype=np.int64)] = False
    return row[:, None] & ~np.isnan(Z)


def rank(Z, valid, mode, top_m, first_id=0, n_ids=0, exclude=None, m_stride=None):
    """Z [n, classes] float32 -> (ids [classes, m_stride] uint64, logits [classes, m_stride] float32, counts [classes] uint32);
    entries past a count are left as the binding leaves them (id 0, logit NaN)."""
    Z = np.asarray(Z, dtype=np.float32)
    mode = _MODES[mode]
    n, C = Z.shape
    m_stride = top_m if m_stride is None else m_stride
    ids = np.zeros((C, m_stride), dtype=np.uint64)
    logits = np.full((C, m_stride), np.nan, dtype=np.float32)
    counts = np.zeros(C, dtype=np.uint32)
    ok = eligible(Z, valid, first_id, n_ids, exclude)
    for c in range(C):
        rows = np.flatnonzero(ok[:, c])                      # ascending ids
        z = Z[rows, c]
        with np.errstate(invalid="ignore"):
            key = np.abs(z) if mode == UNCERTAIN else -z     # ascending key = the order; numpy compares -0.0 == +0.0
        order = rows[np.argsort(key, kind="stable")][:top_m]  # stable: equal keys stay in id order
        k = len(order)
        counts[c] = k
        ids[c, :k] = order
        logits[c, :k] = Z[order, c]
    return ids, logits, counts
