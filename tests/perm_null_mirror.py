"""The host restatement of csrc/perm_null.h in plain numpy, shared by class_cohesion_mirror.py, mantel_mirror.py
and enrich_mirror.py, each of which brings its tag of counter_rng.h; the keys are node2vec_mirror.py's."""
import numpy as np

from node2vec_mirror import rng_key


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): |computed sum - exact sum| <= gamma_{k-1} * sum |terms| for k terms added in any order"""
    u = 2.0 ** -53
    return k * u / (1 - k * u)


def permutation(seed, tag, s, n):
    i = np.arange(n, dtype=np.uint64)
    key = rng_key(seed, tag, np.uint64(s), i, 0)
    return np.lexsort((i, key)).astype(np.int32)


def ordered_row_sum(terms):
    """r_j in the kernels' order: lane l adds the terms l, l + 64, ... ascending from +0.0, then the butterfly p[l] = p[l] + p[l ^ o],
    o = 32 .. 1.  Signed terms (Mantel's) too: a sum that starts at +0.0 never becomes -0.0, so the padding's + 0.0 changes no bit"""
    t = np.zeros(-(-len(terms) // 64) * 64)
    t[:len(terms)] = terms
    p = np.zeros(64)
    for chunk in t.reshape(-1, 64):
        p = p + chunk
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ o]
    return float(p[0])
