"""The host restatement of csrc/class_cohesion.hip (include/gssgcn.h), shared by test_class_cohesion.py (CPU) and the
GPU tests.  Plain numpy:
  permutation   pi_s = 0 .. n - 1 sorted by (rng_key(seed, 9, s, i, 0), i) -- the keys of counter_rng.h as node2vec_mirror.py states them;
  fsum_*        every sum formed with math.fsum (correctly rounded): what the kernels' sums are held to, within gamma(K - 1) * T;
  ordered_*     the kernels' own order of additions, term by term in IEEE fp64: what their bits are.
Distances are non-negative wherever these are used."""
from __future__ import annotations

import math

import numpy as np

from node2vec_mirror import rng_key

TAG_CLASS_PERM = 9
U = 2.0 ** -53


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative bound on a sum of k + 1 non-negative terms added in any order"""
    return k * U / (1 - k * U)


def permutation(seed, s, n):
    i = np.arange(n, dtype=np.uint64)
    key = rng_key(seed, TAG_CLASS_PERM, np.uint64(s), i, 0)
    return np.lexsort((i, key)).astype(np.int32)


def pair_terms(D, a, m=None):
    """the K = m (m - 1) / 2 terms D[a[j]][a[i]], i < j < m, row after row"""
    a = np.asarray(a, dtype=np.int64)[:m]
    return np.concatenate([D[a[j], a[:j]] for j in range(1, len(a))]) if len(a) > 1 else np.zeros(0)


def fsum_pairs(D, a):
    return math.fsum(pair_terms(D, a))


def fsum_prefixes(D, a, sizes):
    """T(m) of the list's prefix for every m in sizes (ascending), each the correctly rounded sum of its terms"""
    terms = pair_terms(D, a, max(sizes))
    return np.array([math.fsum(terms[:m * (m - 1) // 2]) for m in sizes])


def ordered_row_sum(row_terms):
    """r_j in the kernel's order: lane l adds the terms l, l + 64, ... ascending from +0.0; the butterfly p[l] += p[l ^ o], o = 32 .. 1"""
    t = np.zeros(-(-len(row_terms) // 64) * 64)
    t[:len(row_terms)] = row_terms
    p = np.zeros(64)
    for chunk in t.reshape(-1, 64):
        p = p + chunk            # a lane beyond the row's end adds nothing: + 0.0 leaves a non-negative partial sum as it is
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = p + p[lanes ^ o]
    return float(p[0])


def ordered_prefixes(D, a, sizes):
    """T(m) for every m in sizes (ascending) with the kernel's additions: r_1 + r_2 + ... in that order"""
    a = np.asarray(a, dtype=np.int64)
    out, T, k = [], 0.0, 0
    for j in range(1, max(sizes)):
        r = ordered_row_sum(D[a[j], a[:j]])
        T = r if j == 1 else T + r
        if k < len(sizes) and sizes[k] == j + 1:
            out.append(T)
            k += 1
    return np.array(out)


def ordered_pairs(D, a):
    return float(ordered_prefixes(D, a, [len(a)])[0]) if len(a) > 1 else 0.0


def atc_fixture():
    """tests/golden/atc_classes.npz, the reference's drug-class table as packed by make_atc_fixture.py -> (rows of the table, the drug ids in
    order of first appearance, {level: {class code: [name, [drug ids]]}}): what classes.read_classes gives on the table itself"""
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atc_classes.npz"))
    lines = lambda key: bytes(z[key]).decode().split("\n")  # noqa: E731
    drugs, table = lines("drugs"), {}
    for k in (1, 2, 3, 4):
        ptr, members = z[f"ptr_{k}"], z[f"members_{k}"]
        table[k] = {code: [name, [drugs[i] for i in members[ptr[c]:ptr[c + 1]]]]
                    for c, (code, name) in enumerate(zip(lines(f"codes_{k}"), lines(f"names_{k}")))}
    return int(z["rows"]), drugs, table
