"""Numpy / plain Python statement of DIAMOnD as csrc/diamond.hip grows a module (include/gssgcn.h, gss_diamond_grow), for tests only.

  * lgamma_table(n): lg[i] = math.lgamma(i), lg[0] = inf (never read): the table the product uploads;
  * tail(lg, N, s, k, kb): (lt0, S, logp) of P(X >= kb), X hypergeometric (population N, s marked, k drawn): Python floats, one IEEE
    operation after the other in the header's order, so lt0 and S are the device's bits and logp differs by its log alone;
  * grow(rowptr, col, seeds, n_add, alpha): the two-stage choice, step by step -> a dict of per-step lists: node, k, kb, lt0, S, logp,
    gap (the relative distance of the runner-up's logp among stage 1's survivors, inf when there is none) and terms (the longest tail
    sum evaluated in the step); after the last candidate node = -1 and zeros, gap = inf;
  * candidates(...) beside it: every candidate's (v, k', kb') of a step, for the check against scipy over ALL of them;
  * holdout_recovery: DiamondEngine.recovery on the mirror.
"""
from __future__ import annotations

import math

import numpy as np

FIELDS = ("node", "k", "kb", "lt0", "S", "logp")


def lgamma_table(n):
    lg = np.empty(n, np.float64)
    lg[0] = np.inf
    for i in range(1, n):
        lg[i] = math.lgamma(i)
    return lg


def _log_choose(lg, a, b):
    return float(lg[a + 1]) - (float(lg[a - b + 1]) + float(lg[b + 1]))


def tail(lg, N, s, k, kb):
    """-> (lt0, S, logp, number of terms summed)"""
    lt0 = (_log_choose(lg, s, kb) + _log_choose(lg, N - s, k - kb)) - _log_choose(lg, N, k)
    term, S = 1.0, 1.0
    end = min(k, s)
    for i in range(kb, end):
        term = term * (float((s - i) * (k - i)) / float((i + 1) * (N - s - k + i + 1)))
        S = S + term
    return lt0, S, lt0 + math.log(S), max(end - kb, 0)


class State:
    """the module of one unit: ks, ka per node and the membership"""

    def __init__(self, rowptr, col, seeds, alpha):
        self.rowptr, self.col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
        self.n = len(self.rowptr) - 1
        self.deg = np.diff(self.rowptr)
        self.alpha = int(alpha)
        self.m = len(seeds)
        self.inside = np.zeros(self.n, bool)
        self.ks = np.zeros(self.n, np.int64)
        self.ka = np.zeros(self.n, np.int64)
        for v in seeds:
            self.inside[v] = True
            np.add.at(self.ks, self.col[self.rowptr[v]:self.rowptr[v + 1]], 1)
        self.added = 0

    @property
    def N(self):
        return self.n + (self.alpha - 1) * self.m

    @property
    def s(self):
        return self.alpha * self.m + self.added

    def candidates(self):
        """(v, k', kb') int64 arrays of every node outside the module with kb' > 0"""
        kb = self.alpha * self.ks + self.ka
        v = np.flatnonzero(~self.inside & (kb > 0))
        return v, self.deg[v] + (self.alpha - 1) * self.ks[v], kb[v]

    def add(self, v):
        self.inside[v] = True
        np.add.at(self.ka, self.col[self.rowptr[v]:self.rowptr[v + 1]], 1)
        self.added += 1


def choose(lg, N, s, v, k, kb):
    """the two stages over candidate arrays -> (node, k', kb', lt0, S, logp, gap, terms), or None without a candidate"""
    if len(v) == 0:
        return None
    order = np.lexsort((v, k, kb))                       # by kb', then k', then the node index
    first = order[np.r_[True, kb[order][1:] != kb[order][:-1]]]
    rows = []
    for j in first:
        lt0, S, logp, terms = tail(lg, N, s, int(k[j]), int(kb[j]))
        rows.append((logp, -int(kb[j]), int(v[j]), int(k[j]), lt0, S, terms))
    rows.sort(key=lambda r: (r[0], r[1]))                # the smallest logp, of two equal the larger kb'
    best = rows[0]
    gap = np.inf
    if len(rows) > 1:
        a, b = best[0], rows[1][0]
        gap = 0.0 if a == b else abs(b - a) / max(abs(a), abs(b))
    return best[2], best[3], -best[1], best[4], best[5], best[0], gap, max(r[6] for r in rows)


def grow(rowptr, col, seeds, n_add, alpha=1, lg=None, on_step=None):
    """on_step(state): called before every choice (the scipy check reads the candidates there)"""
    st = State(rowptr, col, seeds, alpha)
    if lg is None:
        lg = lgamma_table(st.N + 2)
    out = {f: [] for f in FIELDS + ("gap", "terms")}
    for _ in range(n_add):
        pick = None
        if out["node"] == [] or out["node"][-1] >= 0:
            if on_step is not None:
                on_step(st)
            pick = choose(lg, st.N, st.s, *st.candidates())
        if pick is None:
            pick = (-1, 0, 0, 0.0, 0.0, 0.0, np.inf, 0)
        else:
            st.add(pick[0])
        for f, x in zip(FIELDS + ("gap", "terms"), pick):
            out[f].append(x)
    return out


def table(rowptr, col, units, n_add, alpha=1):
    """units: a list of seed arrays -> {field: [len(units), n_add]}; node, k, kb int32, lt0, S, logp, gap fp64, terms int64"""
    n = len(rowptr) - 1
    lg = lgamma_table(n + (alpha - 1) * max([len(u) for u in units] + [1]) + 2)
    runs = [grow(rowptr, col, u, n_add, alpha, lg) for u in units]
    kinds = {"node": np.int32, "k": np.int32, "kb": np.int32, "terms": np.int64}
    return {f: np.array([r[f] for r in runs], kinds.get(f, np.float64)).reshape(len(units), n_add) for f in FIELDS + ("gap", "terms")}


def holdout_recovery(rowptr, col, draws, n_add, alpha=1):
    """draws: per set the list of (kept, held) node arrays of its repeats (diamond.holdout_draws) -> int64 [n_sets, n_add]: over the
    repeats, the held-out nodes among the first r + 1 nodes added"""
    out = np.zeros((len(draws), n_add), np.int64)
    for i, reps in enumerate(draws):
        for kept, held in reps:
            got = np.array(grow(rowptr, col, kept, n_add, alpha)["node"])
            out[i] += np.cumsum(np.isin(got, held) & (got >= 0))
    return out
