"""numpy mirror of csrc/rwr.hip (gss_rwr_rank, gss_rwr_null_stats), fp64.  include/gssgcn.h states the iteration and the order of every
sum; this file restates it twice:

  replay      plain Python loops, one IEEE operation per line, lane by lane and wave by wave as the header words it;
  walk_many   the same operations as array operations over many units at once.  It gives the very bits of replay
              (tests/test_rwr_mirror.py asserts that) and is fast enough for the 2016 network.

`rule` names one of ABLATIONS, a plausible wrong rule; tests/test_rwr_mirror.py shows that each of them changes an asserted output of
some case, so a kernel that had taken the wrong rule would not pass."""
from __future__ import annotations

import math

import numpy as np

THREADS, LANES = 1024, 64
WAVES = THREADS // LANES
LONG_ROW = 32                     # a row of more entries than this is summed by 64 lanes
MAX_NODES = 20000
MAX_ADD = 1024
MAX_SEEDS = 4096
MAX_BLOCKS = 2048
STEPS = (32, 16, 8, 4, 2, 1)      # the butterfly's distances

ABLATIONS = {
    "row_normalised": "s[i] = (sum of p over row i) / deg[i] instead of the sum of p[j] / deg[j]",
    "restart_uniform": "the restart mass spread over all nodes",
    "seeds_candidates": "seeds left among the candidates",
    "ties_larger": "of two equal scores the larger node first",
    "err_le": "stop at err <= tol",
    "err_max": "err as the largest change instead of the sum",
    "one_fewer": "one iteration fewer",
    "p0_unnormalised": "after a hold-out, 1 / the full set's size on the kept seeds",
    "sample_sd": "the sample's sd (n - 1) instead of the population's",
    "ge_gt": "ge counts null > obs",
}


def iteration_bound(restart, tol):
    """no walk needs more iterations than this: err_t <= 2 (1 - restart)^t"""
    return int(math.ceil(math.log(tol / 2.0) / math.log(1.0 - restart))) + 1


# ---- the literal form --------------------------------------------------------------------------------------------------------------------

def _butterfly(x):
    x = list(x)
    for o in STEPS:
        x = [x[l] + x[l ^ o] for l in range(LANES)]
    return x


def replay(rowptr, col, seeds, restart, tol, max_iter):
    """-> (p [n], iters): the kernel's operations one by one"""
    n = len(rowptr) - 1
    rowptr = [int(x) for x in rowptr]
    col = [int(x) for x in col]
    restart, tol = float(restart), float(tol)
    m = len(seeds)
    if m == 0:
        return np.full(n, np.nan), 0
    member = [False] * n
    for v in seeds:
        member[int(v)] = True
    first = 1.0 / float(m)
    p0 = [first if member[i] else 0.0 for i in range(n)]
    p = list(p0)
    keep = 1.0 - restart
    it = 0
    while it < max_iter:
        it += 1
        q = [p[j] / float(rowptr[j + 1] - rowptr[j]) for j in range(n)]
        new = [0.0] * n
        for i in range(n):
            lo, hi = rowptr[i], rowptr[i + 1]
            if hi - lo <= LONG_ROW:
                s = 0.0
                for e in range(lo, hi):
                    s = s + q[col[e]]
            else:
                part = [0.0] * LANES
                for lane in range(LANES):
                    for e in range(lo + lane, hi, LANES):
                        part[lane] = part[lane] + q[col[e]]
                s = _butterfly(part)[0]
            walk_, back = keep * s, restart * p0[i]
            new[i] = walk_ + back
        per_thread = [0.0] * THREADS
        for i in range(n):                                 # ascending i: thread i % THREADS meets its nodes in ascending order
            per_thread[i % THREADS] = per_thread[i % THREADS] + abs(new[i] - p[i])
        err = None
        for w in range(WAVES):
            x = _butterfly(per_thread[w * LANES:(w + 1) * LANES])[0]
            err = x if err is None else err + x
        p = new
        if err < tol:
            break
    return np.array(p, np.float64), it


# ---- the array form ----------------------------------------------------------------------------------------------------------------------

class Plan:
    """one CSR laid out as the kernel walks it.  scipy's CSR product adds a row's entries one by one in ascending order from 0.0 (its
    data are 1.0, and 1.0 * x is x), which is the order of a short row and of one lane of a long row: `short` holds the short rows,
    `lanes` one row per (long row, lane) with that lane's entries e = lo + lane, + 64, ... -- the products below are the header's sums"""

    def __init__(self, rowptr, col):
        import scipy.sparse as sp
        rowptr = np.asarray(rowptr, np.int64)
        col = np.asarray(col, np.int64)
        n = len(rowptr) - 1
        deg = np.diff(rowptr)
        assert n >= 2 and (deg >= 1).all(), "every row needs an entry"
        self.n, self.deg, self.degf = n, deg, deg.astype(np.float64)
        self.short_rows = np.flatnonzero(deg <= LONG_ROW)
        self.long_rows = np.flatnonzero(deg > LONG_ROW)
        entry = np.concatenate([np.arange(rowptr[i], rowptr[i + 1]) for i in self.short_rows] or [np.zeros(0, np.int64)])
        ptr = np.concatenate([[0], np.cumsum(deg[self.short_rows])])
        self.short = sp.csr_matrix((np.ones(len(entry)), col[entry], ptr), shape=(len(self.short_rows), n))
        entry, ptr = [], [0]
        for i in self.long_rows:
            for lane in range(LANES):
                e = np.arange(rowptr[i] + lane, rowptr[i + 1], LANES)
                entry.append(e)
                ptr.append(ptr[-1] + len(e))
        entry = np.concatenate(entry or [np.zeros(0, np.int64)])
        self.lanes = sp.csr_matrix((np.ones(len(entry)), col[entry], np.array(ptr)), shape=(len(self.long_rows) * LANES, n))
        self.slots = -(-n // THREADS)

    @staticmethod
    def butterfly(x):
        """lane 0's end of the butterfly over axis 1 of x [.., 64, columns]: after the step at distance o the lanes l and l ^ o hold the
        same bits (a + b is b + a), so lane 0's sum is ((x[0] + x[32]) + (x[16] + x[48])) + ..., the halves folded onto each other"""
        for o in STEPS:
            x = x[:, :o] + x[:, o:2 * o]
        return x[:, 0]

    def row_sums(self, q):
        """q [n, columns] -> s [n, columns]"""
        s = np.zeros_like(q)
        s[self.short_rows] = self.short @ q
        if len(self.long_rows):
            part = (self.lanes @ q).reshape(len(self.long_rows), LANES, q.shape[1])
            s[self.long_rows] = self.butterfly(part)
        return s

    def error(self, change):
        """change [n, columns] -> err [columns]"""
        d = np.zeros((self.slots * THREADS, change.shape[1]))
        d[:self.n] = change
        d = d.reshape(self.slots, THREADS, -1)
        acc = np.zeros_like(d[0])
        for k in range(self.slots):
            acc = acc + d[k]
        waves = self.butterfly(acc.reshape(WAVES, LANES, -1))
        err = waves[0]
        for w in range(1, WAVES):
            err = err + waves[w]
        return err


_plans = {}


def plan(rowptr, col):
    key = (id(rowptr), id(col))
    if key not in _plans:
        _plans[key] = (Plan(rowptr, col), rowptr, col)     # the arrays are held: their ids stay theirs
    return _plans[key][0]


def walk_many(rowptr, col, units, restart, tol, max_iter, rule=None, p0_sizes=None):
    """the walks of non-empty units side by side, each stopping on its own -> (p [U, n], iters [U], errs: per unit the err of every
    iteration run).  p0_sizes: per unit the m of 1.0 / m where it is not the unit's size (an ablation's)"""
    P = plan(rowptr, col)
    n, U = P.n, len(units)
    restart, tol = float(restart), float(tol)
    p0 = np.zeros((n, U))
    for u, seeds in enumerate(units):
        p0[np.asarray(seeds, np.int64), u] = 1.0 / float(len(seeds) if p0_sizes is None else p0_sizes[u])
    back = restart * (np.full((n, U), 1.0 / n) if rule == "restart_uniform" else p0)
    keep = 1.0 - restart
    degf = P.degf[:, None]
    p, before = p0.copy(), p0.copy()
    errs = [[] for _ in range(U)]
    live = np.arange(U)
    for _ in range(int(max_iter)):
        old = p[:, live]
        s = P.row_sums(old) / degf if rule == "row_normalised" else P.row_sums(old / degf)
        new = keep * s + back[:, live]
        change = np.abs(new - old)
        err = change.max(axis=0) if rule == "err_max" else P.error(change)
        before[:, live], p[:, live] = old, new
        for u, e in zip(live, err):
            errs[u].append(float(e))
        live = live[~(err <= tol if rule == "err_le" else err < tol)]
        if len(live) == 0:
            break
    iters = np.array([len(e) for e in errs], np.int32)
    if rule == "one_fewer":
        for u in np.flatnonzero(iters > 1):
            p[:, u], iters[u], errs[u] = before[:, u], iters[u] - 1, errs[u][:-1]
    return np.ascontiguousarray(p.T), iters, errs


def walk(rowptr, col, seeds, restart, tol, max_iter, rule=None, p0_size=None):
    """one unit -> (p [n], iters, errs)"""
    if len(seeds) == 0:
        return np.full(len(rowptr) - 1, np.nan), 0, []
    p, iters, errs = walk_many(rowptr, col, [seeds], restart, tol, max_iter, rule, None if p0_size is None else [p0_size])
    return p[0], int(iters[0]), errs[0]


def select(n, seeds, n_add, keys, rule=None):
    """the first n_add candidates under the keys (the last key the first to decide, all descending), ties to the smaller node, -1 padded"""
    cand = np.ones(n, bool)
    if rule != "seeds_candidates":
        cand[np.asarray(seeds, np.int64)] = False
    nodes = np.flatnonzero(cand)
    tie = -nodes if rule == "ties_larger" else nodes
    order = nodes[np.lexsort((tie,) + tuple(-np.asarray(k)[nodes] for k in keys))][:n_add]
    out = np.full(n_add, -1, np.int32)
    out[:len(order)] = order
    return out


def table(rowptr, col, units, n_add, restart, tol, max_iter, rule=None, literal=False):
    """what gss_rwr_rank writes for the units -> {"node" int32 [U, n_add], "score" [U, n_add], "iters" int32 [U], "p" [U, n]}"""
    n = len(rowptr) - 1
    out = {"node": np.full((len(units), n_add), -1, np.int32), "score": np.full((len(units), n_add), np.nan),
           "iters": np.zeros(len(units), np.int32), "p": np.full((len(units), n), np.nan)}
    done = {}                                              # a pure function of the unit: computed once
    for seeds in units:
        done.setdefault(np.asarray(seeds, np.int32).tobytes(), np.asarray(seeds, np.int32))
    todo = [k for k, seeds in done.items() if len(seeds)]
    walked = {}
    for lo in range(0, len(todo), 128):
        keys = todo[lo:lo + 128]
        if literal:
            got = [replay(rowptr, col, done[k], restart, tol, max_iter) for k in keys]
        else:
            p, iters, _ = walk_many(rowptr, col, [done[k] for k in keys], restart, tol, max_iter, rule)
            got = list(zip(p, iters))
        for k, (p, it) in zip(keys, got):
            walked[k] = (p, it, select(n, done[k], n_add, (p,), rule))
    for u, seeds in enumerate(units):
        if len(seeds) == 0:
            continue
        p, it, node = walked[np.asarray(seeds, np.int32).tobytes()]
        out["p"][u], out["iters"][u], out["node"][u] = p, it, node
        out["score"][u] = np.where(node >= 0, p[np.maximum(node, 0)], np.nan)
    return out


def null_stats(p, seeds, n_add, rank_by="p", rule=None):
    """p [R, n]: sample 0 the set, the rest its null -> {"mean", "sd", "z" [n], "ge" int32 [n], "node" int32 [n_add]} as
    gss_rwr_null_stats writes them"""
    p = np.asarray(p, np.float64)
    R, n = p.shape
    if len(seeds) == 0:
        nan = np.full(n, np.nan)
        return {"mean": nan, "sd": nan.copy(), "z": nan.copy(), "ge": np.full(n, -1, np.int32), "node": np.full(n_add, -1, np.int32)}
    count = float(R - 1)
    total = np.zeros(n)
    for k in range(1, R):
        total = total + p[k]
    mean = total / count
    sq = np.zeros(n)
    for k in range(1, R):
        d = p[k] - mean
        sq = sq + d * d
    sd = np.sqrt(sq / (count - 1.0 if rule == "sample_sd" else count))
    z = np.where(sd > 0, (p[0] - mean) / np.where(sd > 0, sd, 1.0), 0.0)
    z[np.asarray(seeds, np.int64)] = np.nan
    ge = ((p[1:] > p[0]) if rule == "ge_gt" else (p[1:] >= p[0])).sum(axis=0).astype(np.int32)
    keys = (p[0], np.where(np.isnan(z), -np.inf, z)) if rank_by == "z" else (p[0],)
    return {"mean": mean, "sd": sd, "z": z, "ge": ge, "node": select(n, seeds, n_add, keys, rule)}


def recovery(rowptr, col, draws, n_add, restart, tol, max_iter, rule=None):
    """the leave-out validation as a plain loop over diamond.holdout_draws' draws -> (recovered int64 [n_sets, n_add], held int64 [n_sets])"""
    n = len(rowptr) - 1
    rec = np.zeros((len(draws), n_add), np.int64)
    held_n = np.zeros(len(draws), np.int64)
    for i, reps in enumerate(draws):
        for kept, held in reps:
            held_n[i] += len(held)
            if len(kept) == 0:
                continue
            size = len(kept) + len(held) if rule == "p0_unnormalised" else None
            p = walk(rowptr, col, kept, restart, tol, max_iter, rule, p0_size=size)[0]
            node = select(n, kept, n_add, (p,), rule)
            gone = set(int(h) for h in held)
            hits = 0
            for r in range(n_add):
                if int(node[r]) in gone:
                    hits += 1
                rec[i, r] += hits
    return rec, held_n
