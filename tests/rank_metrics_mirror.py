"""The host restatement of csrc/rank_metrics.hip's three definitions (include/gssgcn.h), shared by
test_rank_metrics.py (CPU) and the GPU tests.  Scores compare as the kernel compares them (-0.0 folded into +0.0); a tie group is a
maximal set of equal scores.
  auc   evaluate_fixture.mirror_aucs: the kernel's own integer counts and its one division.
  ap    (1 / P) sum over the tie groups that hold a positive of pos_g TP_g / (TP_g + FP_g), in exact rationals, rounded once (ap_exact);
        and the same sum in the kernel's order of fp64 additions (ap_ordered), which fixes the bits the device writes.
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


AP_THREADS, AP_WAVE = 256, 64


def ap_ordered(pos, neg, P):
    """the kernel's average precision, addition by addition (csrc/rank_score.h, DESIGN.md section 9.8 "Order of summation"): pos [P] and
    neg [N] are one class's scores each, sorted ascending with -0.0 folded into +0.0.  Sorted positive i has posL / posU positives and
    negL negatives below / not above its score; the first positive of a tie group (i == posL) speaks for it with the term
    float64(pos_g TP_g) / float64(TP_g + FP_g), pos_g = posU - posL, TP_g = P - posL, FP_g = N - negL.
      1. thread t of 256 starts from +0.0 and adds the terms of i = P-1-t, P-1-t-256, ... in that order;
      2. each wave of 64 runs the xor butterfly at offsets 32, 16, 8, 4, 2, 1: v = v + v[lane ^ o];
      3. the four lane-0 values are added in wave order from 0.0, and the sum is divided by P.
    The operands are exact integers below 2^53 and every operation is one IEEE rounding, so numpy gives the kernel's bits."""
    pos, neg = np.asarray(pos, np.float64), np.asarray(neg, np.float64)
    assert len(pos) == P >= 1 and np.all(pos[1:] >= pos[:-1]) and np.all(neg[1:] >= neg[:-1])
    posL, posU = np.searchsorted(pos, pos, "left").astype(np.int64), np.searchsorted(pos, pos, "right").astype(np.int64)
    negL = np.searchsorted(neg, pos, "left").astype(np.int64)
    tp, fp = P - posL, len(neg) - negL
    term = ((posU - posL) * tp).astype(np.float64) / (tp + fp).astype(np.float64)
    first = posL == np.arange(P)
    acc = np.zeros(AP_THREADS, np.float64)
    for top in range(P - 1, -1, -AP_THREADS):                # one trip of the threads' loop: thread t holds i = top - t
        i = top - np.arange(AP_THREADS)
        live = i >= 0
        i = np.where(live, i, 0)
        acc = np.where(live & first[i], acc + term[i], acc)
    total = 0.0
    for w in range(AP_THREADS // AP_WAVE):
        v = acc[w * AP_WAVE:(w + 1) * AP_WAVE].copy()
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(AP_WAVE) ^ o]
        total = total + float(v[0])
    return float(np.float64(total) / np.float64(P))


def ap_ordered_row(s, mask):
    """ap_ordered of one row: scores [C] and the positives' mask"""
    s, mask = np.asarray(s, np.float64) + 0.0, np.asarray(mask, bool)
    return ap_ordered(np.sort(s[mask]), np.sort(s[~mask]), int(mask.sum()))


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
