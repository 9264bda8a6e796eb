"""bn_index_search_seq restated in numpy from include/birdnet_hip.h alone: given the score of every (query window, index row) pair, the
score of every start row of a sequence, which starts are eligible, and the first M of them (or of their peaks).  Pure numpy; shared by
test_seq_cpu.py (self-checks against a float64 brute force and against peaks_ref) and test_gpu_seq.py (the expected value of every GPU
comparison)."""
import numpy as np

import peaks_ref


def seq_scores(S, xbad, L):
    """S [L, n]: window score of (query window j, index row r).  -> (score [n] float32, ok [n] bool) per start row i:
    acc_0 = s_0(i); acc_j = fl32(acc_{j-1} + s_j(i + j)), j ascending; score = fl32(acc * fl32(1 / L)).  ok: i + L <= n and no row of
    i .. i + L - 1 is invalid.  The score of a start that is not ok is 0 and means nothing."""
    S = np.asarray(S, dtype=np.float32)
    xbad = np.asarray(xbad, dtype=bool)
    assert S.shape[0] == L >= 1
    n = S.shape[1]
    score, ok = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=bool)
    ns = n - L + 1                                               # starts with i + L <= n
    if ns <= 0:
        return score, ok
    acc = S[0, :ns].copy()
    for j in range(1, L):
        acc = acc + S[j, j:j + ns]                               # element-wise float32 adds, one rounding each
        assert acc.dtype == np.float32
    score[:ns] = acc * (np.float32(1) / np.float32(L))           # one float32 multiply by the rounded reciprocal
    covered = np.zeros(ns, dtype=bool)
    for j in range(L):
        covered |= xbad[j:j + ns]
    ok[:ns] = ~covered
    score[~ok] = 0
    return score, ok


def start_eligibility(ok, qbad_rows, first_id=None, exclude_radius=-1):
    """bool [n]: the starts one sequence may return: the start is ok (seq_scores), none of the sequence's own rows is invalid and, for the
    _ids form, |i - first_id| > exclude_radius (negative: nothing skipped)"""
    el = np.asarray(ok, dtype=bool).copy()
    if np.asarray(qbad_rows, dtype=bool).any():
        el[:] = False
    if first_id is not None and exclude_radius >= 0:
        el &= np.abs(np.arange(len(el), dtype=np.int64) - int(first_id)) > exclude_radius
    return el


def seq_matrix(S, qbad, xbad, L, first_ids=None, exclude_radius=-1):
    """S [n_seq * L, n], qbad [n_seq * L] -> (Z [n_seq, n] float32 sequence scores, eligible [n_seq, n] bool)"""
    S = np.asarray(S, dtype=np.float32)
    n_seq = S.shape[0] // L
    assert S.shape[0] == n_seq * L and len(qbad) == S.shape[0]
    Z = np.zeros((n_seq, S.shape[1]), dtype=np.float32)
    el = np.zeros(Z.shape, dtype=bool)
    for p in range(n_seq):
        Z[p], ok = seq_scores(S[p * L:(p + 1) * L], xbad, L)
        el[p] = start_eligibility(ok, qbad[p * L:(p + 1) * L], None if first_ids is None else first_ids[p], exclude_radius)
    return Z, el


def seq_top_m(S, qbad, xbad, L, peak_radius, M, first_ids=None, exclude_radius=-1):
    """-> (ids [n_seq, M] uint64 START rows, scores [n_seq, M] float32, counts [n_seq] uint32): the first M eligible starts (peak_radius
    0) or peaks among them by score descending, ties by id ascending; entries past a count as the binding leaves them (id 0, score NaN)"""
    Z, el = seq_matrix(S, qbad, xbad, L, first_ids, exclude_radius)
    return peaks_ref.peaks_top_m(Z, el, peak_radius, M)
