"""Shared by test_train_eval.py (CPU) and test_gpu_train_eval.py: csrc/scores.hip's arithmetic in numpy, with the summation order that
include/gssgcn.h documents for gss_embedding_scores.  numpy's elementwise *, +, / and sqrt round once each and never fuse, which is what
the kernel does (it is compiled with contraction off), so the mirror reproduces every bit.

  norm   64 partial sums p[l] = sum of x[k]^2 over k = l, l + 64, ... (ascending, from +0.0), then p[l] = p[l] + p[l ^ m] for
         m = 32, 16, 8, 4, 2, 1; norm = sqrt(p[0]); a zero norm becomes 1
  value  float64(x) / norm
  dot    acc = +0.0; acc = acc + a[k] * b[k] for k = 0 .. d - 1
"""
import numpy as np

LANES = 64


def norms(x32, d):
    """x32: fp32 [n, >= d] -> fp64 [n] row norms over the first d values, zero norms replaced by 1"""
    x = np.asarray(x32, dtype=np.float32)[:, :d].astype(np.float64)
    p = np.zeros((x.shape[0], LANES))
    for k in range(d):
        p[:, k % LANES] = p[:, k % LANES] + x[:, k] * x[:, k]
    lane = np.arange(LANES)
    m = LANES // 2
    while m:
        p = p + p[:, lane ^ m]
        m //= 2
    assert (p == p[:, :1]).all()          # the butterfly leaves every lane with the same bits
    nrm = np.sqrt(p[:, 0])
    nrm[nrm == 0] = 1.0
    return nrm


def values(x32, d, normalize):
    """the fp64 rows the dot products are taken of"""
    x = np.asarray(x32, dtype=np.float32)[:, :d].astype(np.float64)
    return x / norms(x32, d)[:, None] if normalize else x


def scores(x32, d, rows, cols, normalize):
    """gss_embedding_scores(n, d, x32, ld, rows, cols, normalize) -> fp64 [len(rows), len(cols)]"""
    v = values(x32, d, normalize)
    a, b = v[np.asarray(rows, dtype=np.int64)], v[np.asarray(cols, dtype=np.int64)]
    acc = np.zeros((a.shape[0], b.shape[0]))
    for k in range(d):
        acc = acc + a[:, k, None] * b[None, :, k]
    return acc
