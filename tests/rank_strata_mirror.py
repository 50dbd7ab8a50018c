"""The host restatement of csrc/rank_strata.hip (include/gssgcn.h), shared by test_rank_strata.py (CPU) and the GPU
tests: a stratum is the sub-problem of its row's negatives and its own positives, gathered into a row of its own, and its three statistics
are rank_metrics_mirror.mirror_metrics on that row -- nothing is restated here but the gather."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_metrics_mirror as M  # noqa: E402


def gathered(row, row_pos, sub):
    """one row's scores [C], its positive columns and a stratum's columns -> (the sub-problem's scores [N + Q]: the negatives in column
    order, then the stratum's positives in list order; its positive columns N .. N + Q - 1)"""
    row = np.asarray(row, np.float64)
    neg = np.ones(len(row), bool)
    neg[np.asarray(row_pos, np.int64)] = False
    sub = np.asarray(sub, np.int64)
    n = int(neg.sum())
    return np.concatenate([row[neg], row[sub]]), np.arange(n, n + len(sub), dtype=np.int32)


def strata_csr(strata):
    """per row the list of its strata, each a list of columns -> (str_ptr, sub_ptr, sub_col) int32"""
    str_ptr = np.zeros(len(strata) + 1, np.int32)
    str_ptr[1:] = np.cumsum([len(row) for row in strata])
    flat = [np.asarray(q, np.int32) for row in strata for q in row]
    sub_ptr = np.zeros(len(flat) + 1, np.int32)
    sub_ptr[1:] = np.cumsum([len(q) for q in flat])
    return str_ptr, sub_ptr, np.concatenate(flat + [np.zeros(0, np.int32)]).astype(np.int32)


def mirror_strata(scores, pos_ptr, pos_col, str_ptr, sub_ptr, sub_col, ks, timings=None):
    """evaluate.device_metrics_strata on the host -> (auc [S], ap [S], hits [S, len(ks)], s_pos [S], n_pos [R], n_neg [R]); NaN in auc, ap
    and hits where a stratum is empty or its row has no negative"""
    scores = np.asarray(scores.cpu().numpy() if hasattr(scores, "cpu") else scores, dtype=np.float64)
    R, C = scores.shape
    S = int(str_ptr[-1])
    n_pos = np.diff(np.asarray(pos_ptr)).astype(np.int32)
    n_neg = (C - n_pos).astype(np.int32)
    auc, ap, hits = np.full(S, np.nan), np.full(S, np.nan), np.full((S, len(ks)), np.nan)
    s_pos = np.diff(np.asarray(sub_ptr)).astype(np.int32)
    for r in range(R):
        row_pos = pos_col[pos_ptr[r]:pos_ptr[r + 1]]
        for s in range(str_ptr[r], str_ptr[r + 1]):
            sub = sub_col[sub_ptr[s]:sub_ptr[s + 1]]
            assert set(int(c) for c in sub) <= set(int(c) for c in row_pos) and len(set(int(c) for c in sub)) == len(sub)
            if len(sub) == 0 or n_neg[r] == 0:
                continue
            x, cols = gathered(scores[r], row_pos, sub)
            a, p, h, _, _ = M.mirror_metrics(x[None, :], np.asarray([0, len(cols)], np.int32), cols, ks)
            auc[s], ap[s], hits[s] = a[0], p[0], h[0]
    return auc, ap, hits, s_pos, n_pos, n_neg
