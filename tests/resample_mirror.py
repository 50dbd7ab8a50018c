"""The host restatement of csrc/resample.hip (include/gssgcn.h), shared by test_resample.py (CPU) and the GPU tests.
Plain numpy:
  draw          idx(b, j) = ((rng_key(seed, 10, b, j, 0) >> 32) * n) >> 32 in uint64 -- the keys of counter_rng.h as node2vec_mirror.py states them;
  flips         the top bit of rng_key(seed, 11, b, j, 0);
  multiset      the n values of replicate b of a series, sorted ascending, -0.0 as +0.0 (the kernel sorts order_keys, which fold it);
  median        the middle value, or (the two middle values added) * 0.5;
  ordered_sum   the kernel's own order of additions, term by term in IEEE fp64: what the mean's bits are."""
from __future__ import annotations

import math

import numpy as np

from node2vec_mirror import rng_key

TAG_BOOT_DRAW = 10
TAG_SIGN_FLIP = 11
PLAIN, BOOTSTRAP, SIGN_FLIP = 0, 1, 2
SUM_LANES = 256
U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the bound on a sum of k + 1 terms added in any order, relative to the sum of their magnitudes"""
    return k * U / (1 - k * U)


def draw(seed, b, n):
    """the n places replicate b of the bootstrap reads -> int64 [n], each in [0, n)"""
    h = rng_key(seed, TAG_BOOT_DRAW, np.uint64(b), np.arange(n, dtype=np.uint64), 0)
    return (((h >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def flips(seed, b, n):
    """the places replicate b of the sign-flip null negates -> bool [n]"""
    h = rng_key(seed, TAG_SIGN_FLIP, np.uint64(b), np.arange(n, dtype=np.uint64), 0)
    return (h >> np.uint64(63)).astype(bool)


def gathered(values, mode, seed, b):
    """the multiset of replicate b in the order of the places, before the sort"""
    v = np.asarray(values, dtype=np.float64)
    if mode == PLAIN:
        return v.copy()
    if mode == BOOTSTRAP:
        return v[draw(seed, b, len(v))]
    return np.where(flips(seed, b, len(v)), -v, v)


def multiset(values, mode, seed, b):
    return np.sort(gathered(values, mode, seed, b) + 0.0)      # -0.0 + 0.0 = +0.0


def median(x):
    """of the sorted x"""
    n = len(x)
    return float(x[n // 2]) if n & 1 else float((x[n // 2 - 1] + x[n // 2]) * 0.5)


def ordered_sum(x):
    """the sorted x added in the kernel's order: p_t = x_t + x_{t+256} + ... ascending from +0.0; the butterfly p[l] += p[l ^ o], o = 32 .. 1,
    inside each group of 64; then ((W_0 + W_1) + W_2) + W_3"""
    t = np.zeros(-(-len(x) // SUM_LANES) * SUM_LANES)
    t[:len(x)] = x
    p = np.zeros(SUM_LANES)
    for chunk in t.reshape(-1, SUM_LANES):
        p = p + chunk            # a lane beyond the end adds + 0.0; no partial sum is -0.0 (the sorted values hold none), so that changes no bit
    lanes = np.arange(SUM_LANES)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ o]     # l ^ o stays inside l's group of 64
    return float(((p[0] + p[64]) + p[128]) + p[192])


def stats_of(x):
    """(mean, median) of the sorted multiset x"""
    return ordered_sum(x) / len(x), median(x)


def resample_stats(values, mode, seed, count, first=0):
    """the kernel's output [count][S][2] for the series values [S][n]"""
    v = np.atleast_2d(np.asarray(values, dtype=np.float64))
    out = np.empty((count, len(v), 2))
    for r in range(count):
        for s, row in enumerate(v):
            out[r, s] = stats_of(multiset(row, mode, seed, first + r))
    return out


def mean_bound(values):
    """|a mean whose sum was added in any order - fsum / n| is within this"""
    v = np.asarray(values, dtype=np.float64)
    return gamma(len(v) - 1) * math.fsum(np.abs(v)) / len(v)
