"""The host restatement of csrc/class_cohesion.hip (include/gssgcn.h), shared by test_class_cohesion.py (CPU) and the
GPU tests.  Plain numpy:
  fsum_*        every sum formed with math.fsum (correctly rounded): what the kernels' sums are held to, within gamma(K - 1) * T;
  ordered_*     the kernels' own order of additions (perm_null_mirror.ordered_row_sum per row), term by term in IEEE fp64: what their bits are.
Distances are non-negative wherever these are used."""
from __future__ import annotations

import math

import numpy as np

from perm_null_mirror import gamma, ordered_row_sum, permutation as tagged_permutation  # noqa: F401

TAG_CLASS_PERM = 9


def permutation(seed, s, n):
    return tagged_permutation(seed, TAG_CLASS_PERM, s, n)


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
