"""The host restatement of csrc/enrich.hip (include/gssgcn.h), shared by test_enrich_mirror.py (CPU) and the GPU tests.
Plain numpy and Python floats (IEEE fp64, one rounding per operation):
  order         pos[u] = the place of u in np.argsort(-x[universe], kind="stable"), w = |x[universe]|; a NaN flags the column;
  es_peak       the enrichment score and its peak of a set of places, operation by operation as the header states it;
  exact_walk    the same score as the extreme of the running sum over all M places, in exact rationals: what es_peak is held to;
  stats         n_same, p, nes, q and the leading edge of enrich.enrichment_stats, restated."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import perm_null_mirror
from node2vec_mirror import rng_key

TAG_ENRICH_PERM = 13


def order(x, universe):
    """one profile x [n] -> (pos int32 [M], w fp64 [M])"""
    v = np.asarray(x, dtype=np.float64)[np.asarray(universe, dtype=np.int64)]
    M = len(v)
    if np.isnan(v).any():
        return np.full(M, -1, dtype=np.int32), np.full(M, np.nan)
    pos = np.empty(M, dtype=np.int32)
    pos[np.argsort(-v, kind="stable")] = np.arange(M, dtype=np.int32)
    return pos, np.abs(v)


def es_peak(pos, w, members, weighted=True):
    """-> (ES, peak) of the set `members` (distinct places) in the column (pos, w)"""
    M, s = len(pos), len(members)
    if pos[0] < 0:
        return float("nan"), -1
    mem = sorted((int(u) for u in members), key=lambda u: int(pos[u]))
    a = [float(w[u]) if weighted else 1.0 for u in mem]
    N = 0.0
    for v in a:
        N = N + v
    if N == 0.0:
        return float("nan"), -1
    den = float(M - s)
    c, hi, lo, khi, klo = 0.0, -np.inf, np.inf, -1, -1
    with np.errstate(all="ignore"):
        for k, u in enumerate(mem):
            miss = np.float64(int(pos[u]) - k) / np.float64(den)
            l = np.float64(c) / np.float64(N) - miss
            c = c + a[k]
            h = np.float64(c) / np.float64(N) - miss
            if h > hi:
                hi, khi = h, k
            if l < lo:
                lo, klo = l, k
    return (float(hi), khi) if hi >= -lo else (float(lo), klo)


def exact_walk(pos, w, members, weighted=True):
    """the running sum over all M places in exact rationals: + a_u / N at a member, - 1 / (M - s) elsewhere -> (max, min) of the sum over
    the start and the value after every place"""
    M, s = len(pos), len(members)
    at = np.argsort(pos)                      # place at each position
    inside = set(int(u) for u in members)
    N = sum(Fraction(float(w[u])) if weighted else Fraction(1) for u in inside)
    run = hi = lo = Fraction(0)
    for p in range(M):
        u = int(at[p])
        if u in inside:
            run += (Fraction(float(w[u])) if weighted else Fraction(1)) / N
        else:
            run -= Fraction(1, M - s)
        hi, lo = max(hi, run), min(lo, run)
    return hi, lo


def permutation(seed, s, M):
    return perm_null_mirror.permutation(seed, TAG_ENRICH_PERM, s, M)


def first_threshold_count(seed, s, M, kmax):
    """how many keys of sample s the kernel's first threshold floor(2^64 (kmax + kmax // 4 + 8) / M) collects (M > SEL_CAP)"""
    t0 = ((kmax + kmax // 4 + 8) << 64) // M
    key = rng_key(seed, TAG_ENRICH_PERM, np.uint64(s), np.arange(M, dtype=np.uint64), 0)
    return int(np.count_nonzero(key <= np.uint64(t0)))


def random_scores(pos, w, sizes, seed, s0, P, weighted=True):
    """-> (es [P][len(sizes)], perm [P][sizes[-1]]) of one column"""
    M = len(pos)
    es = np.empty((P, len(sizes)))
    perm = np.empty((P, sizes[-1]), dtype=np.int32)
    for s in range(P):
        pi = permutation(seed, s0 + s, M)
        perm[s] = pi[:sizes[-1]]
        for k, m in enumerate(sizes):
            es[s, k] = es_peak(pos, w, pi[:m], weighted)[0]
    return es, perm


def benjamini_hochberg(p):
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    by = np.argsort(p, kind="stable")
    scaled = p[by] * n / np.arange(1, n + 1)
    q = np.empty(n)
    q[by] = np.minimum(1.0, np.minimum.accumulate(scaled[::-1])[::-1])
    return q


def stats(es, peak, sets, pos, sizes, null):
    """one profile: es [C], peak [C], sets = lists of places, pos [M], the null [P][len(sizes)] -> a list of dicts n_same, p, nes, q, lead"""
    col = {int(m): k for k, m in enumerate(sizes)}
    out = []
    for e, pk, members in zip(es, peak, sets):
        e = float(e)
        if e != e:
            out.append({"n_same": 0, "p": float("nan"), "nes": float("nan"), "q": float("nan"), "lead": []})
            continue
        t = np.asarray(null)[:, col[len(members)]]
        same = t[t >= 0] if e >= 0 else t[t < 0]
        mag = np.abs(same)
        n_same = len(same)
        p = (1 + int(np.count_nonzero(mag >= abs(e)))) / (1 + n_same)
        nes = e / float(np.mean(mag)) if n_same else float("nan")
        mem = sorted((int(u) for u in members), key=lambda u: int(pos[u]))
        out.append({"n_same": n_same, "p": p, "nes": nes, "q": float("nan"), "lead": mem[:pk + 1] if e >= 0 else mem[pk:]})
    finite = [k for k, r in enumerate(out) if r["p"] == r["p"]]
    for k, q in zip(finite, benjamini_hochberg([out[k]["p"] for k in finite])):
        out[k]["q"] = float(q)
    return out
