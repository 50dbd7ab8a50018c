"""The host restatement of csrc/rank_metrics.hip's three definitions (include/gssgcn.h), shared by
test_rank_metrics.py (CPU) and the GPU tests.  Scores compare as the kernel compares them (-0.0 folded into +0.0); a tie group is a
maximal set of equal scores.
  auc   evaluate_fixture.mirror_aucs: the kernel's own integer counts and its one division.
  ap    (1 / P) sum over the tie groups that hold a positive of pos_g TP_g / (TP_g + FP_g), in exact rationals, rounded once.
  hits  at k' = min(k, C): the group that holds rank k' has `above` items strictly before it (A positive), g items, pos_g positives;
        slots = k' - above; hits = A + pos_g if slots == g, else fl(A + fl((pos_g slots) / g)) -- the two fp64 operations spelled out."""
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from evaluate_fixture import mirror_aucs  # noqa: E402


def groups(s, mask):
    """the tie groups of one row in descending score: (size [G], positives [G]) as int64 arrays"""
    s = np.asarray(s, np.float64) + 0.0                   # -0.0 + 0.0 = +0.0
    order = np.argsort(-s, kind="stable")
    v, y = s[order], np.asarray(mask, bool)[order]
    start = np.flatnonzero(np.concatenate([[True], v[1:] != v[:-1]]))
    size = np.diff(np.concatenate([start, [len(v)]]))
    pos = np.add.reduceat(y.astype(np.int64), start)
    return size.astype(np.int64), pos


def ap_exact(s, mask):
    """average precision of one row as a Fraction (P >= 1)"""
    size, pos = groups(s, mask)
    seen, tp = np.cumsum(size), np.cumsum(pos)            # TP_g + FP_g and TP_g, down to and including group g
    P = int(tp[-1])
    hold = np.flatnonzero(pos > 0)
    dens = [int(seen[g]) for g in hold]
    common = 1
    for n in set(dens):
        common = common * n // math.gcd(common, n)
    num = sum(int(pos[g]) * int(tp[g]) * (common // n) for g, n in zip(hold, dens))
    return Fraction(num, common * P)


def hits_parts(s, mask, k):
    """-> (A, pos_g, slots, g) of the group that holds rank min(k, C): integers"""
    size, pos = groups(s, mask)
    kk = min(int(k), int(size.sum()))
    seen = np.cumsum(size)
    gi = int(np.searchsorted(seen, kk, "left"))           # the first group whose last member has rank >= k'
    above = int(seen[gi] - size[gi])
    return int(pos[:gi].sum()), int(pos[gi]), kk - above, int(size[gi])


def hits_value(parts):
    """the fp64 value the contract fixes, from hits_parts' integers"""
    A, pos_g, slots, g = parts
    assert 1 <= slots <= g
    if slots == g:
        return float(A + pos_g)
    return float(A) + float(pos_g * slots) / float(g)     # an exact integer product, one division, one sum


def mirror_metrics(scores, pos_ptr, pos_col, ks):
    """evaluate.device_metrics on the host -> (auc [R], ap [R], hits [R, len(ks)], n_pos [R], n_neg [R]); NaN in auc, ap and hits where a
    row has one class"""
    scores = np.asarray(scores, dtype=np.float64)
    R, C = scores.shape
    auc, n_pos, n_neg = mirror_aucs(scores, pos_ptr, pos_col)
    ap = np.full(R, np.nan)
    hits = np.full((R, len(ks)), np.nan)
    for r in range(R):
        if n_pos[r] == 0 or n_neg[r] == 0:
            continue
        mask = np.zeros(C, bool)
        mask[pos_col[pos_ptr[r]:pos_ptr[r + 1]]] = True
        ap[r] = float(ap_exact(scores[r], mask))          # int / int: correctly rounded
        for j, k in enumerate(ks):
            hits[r, j] = hits_value(hits_parts(scores[r], mask, k))
    return auc, ap, hits, n_pos, n_neg


def csr(rows):
    """per row the positive columns -> (pos_ptr, pos_col) int32"""
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(0, np.int32)])
    return ptr, col.astype(np.int32)


# ---- one ordering behind the three entry points: the AUC out of average-tie ranks ------------------------------------------------------

RANK_IDENTITY_WIDTHS = (2, 63, 64, 65, 200)


def tied_rows(C, R=5):
    """seeded scores [R, C] on a handful of levels with both signed zeros, and per row 1 .. C - 1 positive columns"""
    rng = np.random.RandomState(100 + C)
    s = np.round(rng.randn(R, C), 0) * 0.5
    s[s == 0] = np.where(rng.rand(int((s == 0).sum())) < 0.5, -0.0, 0.0)
    s[0, 0], s[R - 1, C - 1] = 0.0, -0.0
    assert np.any(np.signbit(s) & (s == 0)) and np.any(~np.signbit(s) & (s == 0))
    return s, [np.sort(rng.choice(C, rng.randint(1, C), replace=False)) for _ in range(R)]


def auc_from_ranks(ranks, cols):
    """ranks [C]: the average-tie ranks (1 = lowest) of one row's C scores, cols: its P positives.  2 r - 1 = 2 below + tied counts the
    whole row; the positives among themselves make P^2 of it, so 2 U = sum over positives of (2 r_i - 1) - P^2, exact in int64, and
    AUC = 2 U / (2 P N): the kernels' one division"""
    twice = np.asarray(ranks, np.float64)[cols] * 2 - 1
    assert np.all(twice == np.round(twice))
    P, N = len(cols), len(ranks) - len(cols)
    return float(int(twice.astype(np.int64).sum()) - P * P) / (2.0 * float(P) * float(N))
