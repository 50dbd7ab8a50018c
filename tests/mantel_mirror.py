"""The host restatement of csrc/matrix_mantel.hip and of mantel.standardise_pairs (include/gssgcn.h), shared by
test_mantel.py (CPU) and the GPU tests.  Plain numpy:
  ordered_cross_sum   the kernel's own additions (perm_null_mirror.ordered_row_sum per row), term by term in IEEE fp64; terms are signed;
  fsum_cross_sum      the correctly rounded sum (math.fsum) of the same rounded products;
  standardised        the pair values (or their average-tie ranks) centred and scaled to unit norm, as a symmetric matrix."""
from __future__ import annotations

import math

import numpy as np

from perm_null_mirror import gamma, ordered_row_sum, permutation as tagged_permutation  # noqa: F401

TAG_MANTEL_PERM = 12


def permutation(seed, s, n):
    return tagged_permutation(seed, TAG_MANTEL_PERM, s, n)


def row_terms(A, B, pi, j):
    """the rounded products a[j][i] * b[pi(j)][pi(i)], i < j"""
    pi = np.asarray(pi, dtype=np.int64)
    return A[j, :j] * B[pi[j], pi[:j]]


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
