"""The host restatement of csrc/matrix_mantel.hip and of mantel.standardise_pairs (include/gssgcn.h), shared by
test_mantel.py (CPU) and the GPU tests.  Plain numpy:
  permutation         pi_s = 0 .. n - 1 sorted by (rng_key(seed, 12, s, i, 0), i) -- the keys of counter_rng.h as node2vec_mirror.py states them;
  ordered_cross_sum   the kernel's own additions, term by term in IEEE fp64: what its bits are.  Terms are signed;
  fsum_cross_sum      the correctly rounded sum (math.fsum) of the same rounded products;
  standardised        the pair values (or their average-tie ranks) centred and scaled to unit norm, as a symmetric matrix."""
from __future__ import annotations

import math

import numpy as np

from node2vec_mirror import rng_key

TAG_MANTEL_PERM = 12
U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): |computed sum - exact sum| <= gamma_{k-1} * sum |terms| for k terms added in any order"""
    return k * U / (1 - k * U)


def permutation(seed, s, n):
    i = np.arange(n, dtype=np.uint64)
    key = rng_key(seed, TAG_MANTEL_PERM, np.uint64(s), i, 0)
    return np.lexsort((i, key)).astype(np.int32)


def row_terms(A, B, pi, j):
    """the rounded products a[j][i] * b[pi(j)][pi(i)], i < j"""
    pi = np.asarray(pi, dtype=np.int64)
    return A[j, :j] * B[pi[j], pi[:j]]


def ordered_row_sum(terms):
    """r_j in the kernel's order: lane l adds the terms l, l + 64, ... ascending from +0.0 -- a lane without a term keeps its +0.0 --, then
    the butterfly p[l] = p[l] + p[l ^ o], o = 32 .. 1.  A partial sum that starts at +0.0 never becomes -0.0, so the padding's + 0.0 changes
    no bit"""
    t = np.zeros(-(-len(terms) // 64) * 64)
    t[:len(terms)] = terms
    p = np.zeros(64)
    for chunk in t.reshape(-1, 64):
        p = p + chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ o]
    return float(p[0])


def ordered_cross_sum(A, B, pi=None):
    """sum over i < j of A[j][i] * B[pi[j]][pi[i]] with the kernel's additions: T = r_1 + r_2 + ... in that order"""
    n = len(A)
    pi = np.arange(n) if pi is None else pi
    T = ordered_row_sum(row_terms(A, B, pi, 1))
    for j in range(2, n):
        T = T + ordered_row_sum(row_terms(A, B, pi, j))
    return T


def fsum_cross_sum(A, B, pi=None):
    n = len(A)
    pi = np.arange(n) if pi is None else pi
    return math.fsum(t for j in range(1, n) for t in row_terms(A, B, pi, j))


def average_ranks(v):
    """scipy.stats.rankdata(v, method="average")"""
    _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
    cum = np.cumsum(cnt)
    return ((2 * cum - cnt + 1) / 2.0)[inv]


def pair_values(D):
    """the K = n (n - 1) / 2 values D[i][j], i < j, row after row"""
    iu = np.triu_indices(len(D), 1)
    return iu, D[iu]


def standardised(D, method):
    iu, v = pair_values(np.asarray(D, dtype=np.float64))
    if method == "spearman":
        v = average_ranks(v)
    v = v - np.mean(v)
    v = v / np.sqrt(np.sum(v * v))
    out = np.zeros_like(D, dtype=np.float64)
    out[iu] = v
    out[(iu[1], iu[0])] = v
    return out


def correlation(A, B, method):
    """Mantel's r as the kernel's mode 0 adds it on the standardised matrices"""
    return ordered_cross_sum(standardised(A, method), standardised(B, method))
