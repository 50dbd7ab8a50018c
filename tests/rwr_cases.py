"""The inputs of the random-walk-with-restart tests (tests/test_rwr_mirror.py on the CPU, tests/test_gpu_rwr_ops.py on the device): small
connected graphs as symmetric CSRs without self loops, columns ascending, every row with an entry, and per case a list of seed sets
(units) with n_add, restart, tol and max_iter.  Each is the smallest shape at which one thing can go wrong; `why` names it.
mirror(name) is tests/rwr_mirror.py's table of the case, computed once."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import rwr_mirror as M

HUB_DEG = 1150
CLASS_DEGREES = (31, 32, 33, 63, 64, 65, 96, 97, 129)      # both sides of 32 | 33, and of every turn of the 64 lanes

Case = namedtuple("Case", "name n rowptr col units n_add restart tol max_iter why")


def csr(n, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    a, b = key // n, key % n
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(a, minlength=n), out=rowptr[1:])
    return rowptr, b.astype(np.int32)


def path(n):
    return [(i, i + 1) for i in range(n - 1)]


def ring(n):
    return [(i, (i + 1) % n) for i in range(n)]


def sparse(n, mean_degree, seed):
    """a path through every node (no empty row, one component) and random edges on top"""
    rng = np.random.RandomState(seed)
    extra = rng.randint(0, n, (int(n * (mean_degree - 2) / 2), 2))
    return path(n) + [(int(a), int(b)) for a, b in extra]


def _classes():
    """nodes 0 .. 8 have exactly CLASS_DEGREES neighbours among the 400 nodes behind them, which form a path"""
    rng = np.random.RandomState(21)
    n = len(CLASS_DEGREES) + 400
    edges = [(len(CLASS_DEGREES) + i, len(CLASS_DEGREES) + i + 1) for i in range(399)]
    for h, d in enumerate(CLASS_DEGREES):
        edges += [(h, len(CLASS_DEGREES) + int(v)) for v in rng.choice(400, d, replace=False)]
    return n, edges


def _star():
    """a hub (node 0) with HUB_DEG leaves, a sparse side region of 300 nodes, and 200 of the leaves tied to it"""
    rng = np.random.RandomState(5)
    side0 = 1 + HUB_DEG
    n = side0 + 300
    edges = [(0, v) for v in range(1, side0)] + [(side0 + a, side0 + b) for a, b in sparse(300, 5, 6)]
    edges += [(int(v), side0 + int(rng.randint(300))) for v in rng.choice(np.arange(1, side0), 200, replace=False)]
    return n, edges


def _lattice(side):
    at = lambda r, c: r * side + c  # noqa: E731
    return side * side, [(at(r, c), at(r, c + 1)) for r in range(side) for c in range(side - 1)] + \
        [(at(r, c), at(r + 1, c)) for r in range(side - 1) for c in range(side)]


@functools.lru_cache(maxsize=None)
def graph(kind):
    if kind == "classes":
        n, e = _classes()
    elif kind == "star":
        n, e = _star()
    elif kind == "path":
        n, e = 50, path(50)
    elif kind == "ring64":
        n, e = 64, ring(64)
    elif kind == "k65":
        n, e = 65, [(i, j) for i in range(65) for j in range(i + 1, 65)]
    elif kind == "lattice":
        n, e = _lattice(13)
    elif kind == "limit":
        n, e = M.MAX_NODES, ring(M.MAX_NODES)
    elif kind == "n5000":
        n, e = 5000, sparse(5000, 6, 31)
    elif kind.startswith("n"):
        n = int(kind[1:])
        e = sparse(n, 6, n)
    else:
        raise KeyError(kind)
    return (n,) + csr(n, e)


def draw_units(n, count, size, seed, lo=None):
    rng = np.random.RandomState(seed)
    return [np.sort(rng.choice(n, size if lo is None else rng.randint(lo, size + 1), replace=False)).astype(np.int32) for _ in range(count)]


def _u(*lists):
    return [np.array(u, np.int32) for u in lists]


def _exact_tol(kind, seeds, restart, it):
    """the err of iteration `it`, to the bit: with it as tol the walk must go on for one more iteration (err < tol is strict)"""
    n, rowptr, col = graph(kind)
    return M.walk(rowptr, col, seeds, restart, 0.0, it)[2][-1]


A = [3, 17, 40, 41, 250]
_SPECS = {
    # name: (graph, units, n_add, restart, tol, max_iter, why)
    "classes": ("classes", lambda: _u([20, 50, 300], list(range(9)), [9]) + draw_units(409, 3, 12, 1), 40, 0.5, 1e-6, 1000,
                "rows of 31, 32 | 33, 63, 64 | 65, 96 | 97, 129 entries: both sides of the lane | wave class and of every turn of the lanes"),
    "star": ("star", lambda: _u([0], [5, 1200, 1300]) + draw_units(1451, 2, 30, 2), 50, 0.75, 1e-6, 1000,
             "a row longer than the workgroup: the hub as seed and as candidate"),
    "path": ("path", lambda: _u([0], [49], [10, 11, 30]), 20, 0.25, 1e-6, 1000, "degrees 1 and 2, the slowest mixing of all"),
    "n1023": ("n1023", lambda: draw_units(1023, 2, 9, 3), 30, 0.75, 1e-6, 1000, "n just below the thread count"),
    "n1024": ("n1024", lambda: draw_units(1024, 2, 9, 4), 30, 0.75, 1e-6, 1000, "n at the thread count"),
    "n1025": ("n1025", lambda: draw_units(1025, 2, 9, 5) + _u([1024]), 30, 0.75, 1e-6, 1000, "one node in a thread's second register"),
    "n2047": ("n2047", lambda: draw_units(2047, 2, 9, 6), 30, 0.5, 1e-6, 1000, "n just below twice the thread count"),
    "n2048": ("n2048", lambda: draw_units(2048, 2, 9, 7), 30, 0.5, 1e-6, 1000, "n at twice the thread count"),
    "n2049": ("n2049", lambda: draw_units(2049, 2, 9, 8) + _u([2048]), 1024, 0.5, 1e-6, 1000, "a third register; n_add at its cap"),
    "limit": ("limit", lambda: _u([0, 5, 9], [M.MAX_NODES - 1]), 8, 0.75, 1e-6, 1000, "n at the limit: twenty registers, 160,000 bytes of q"),
    "sizes": ("n40", lambda: _u([], [7], [i for i in range(40) if i != 13], list(range(40)), [0, 39]), 60, 0.75, 1e-6, 1000,
              "units of 0, 1, n - 1 and n seeds; n_add over the number of candidates"),
    "wide": ("n5000", lambda: draw_units(5000, 1, M.MAX_SEEDS, 9) + draw_units(5000, 1, 3, 10), 100, 0.75, 1e-6, 1000,
             "a table row of 4,096 seeds; a second selection round"),
    "one": ("n300", lambda: draw_units(300, 3, 6, 11), 1, 0.75, 1e-6, 1000, "n_add = 1"),
    "ring": ("ring64", lambda: _u([0], [0, 32], [5]), 5, 0.75, 1e-6, 1000, "nodes i and -i tie bit for bit; n_add cuts a pair"),
    "k65": ("k65", lambda: _u([3], [0, 64]), 10, 0.5, 1e-6, 1000, "every candidate ties; rows of 64 entries"),
    "lattice": ("lattice", lambda: _u([84], [0], [84, 85]), 6, 0.5, 1e-6, 1000, "ties by symmetry, four and eight at a time, across n_add"),
    "iter1": ("n300", lambda: draw_units(300, 3, 6, 12), 20, 0.75, 0.0, 1, "tol = 0: exactly one iteration; most candidates tie at 0"),
    "iter2": ("n300", lambda: draw_units(300, 3, 6, 12), 20, 0.75, 0.0, 2, "tol = 0: exactly two"),
    "iter30": ("n300", lambda: draw_units(300, 3, 6, 12), 20, 0.75, 0.0, 30, "tol = 0: thirty, far past the fixed point of fp64"),
    "stop1": ("n300", lambda: draw_units(300, 3, 6, 12), 20, 0.75, 3.0, 1000, "err <= 2 < tol: stops after the first iteration"),
    "strict": ("n300", lambda: _u(A), 20, 0.5, lambda: _exact_tol("n300", A, 0.5, 4), 1000, "tol is iteration 4's err to the bit: strict < goes on"),
    "same": ("n300", lambda: [np.array(A, np.int32)] + draw_units(300, 1, 80, 13) + [np.array(A, np.int32)] + draw_units(300, 2, 2, 14)
             + [np.array(A, np.int32)], 25, 0.25, 1e-6, 1000, "one unit at three table positions beside others"),
    "many": ("n300", lambda: draw_units(300, M.MAX_BLOCKS + 6, 8, 15, lo=1), 3, 0.75, 1e-4, 1000, "more units than workgroups"),
}
CASES = tuple(_SPECS)
NOT_CONVERGED = ("n300", lambda: draw_units(300, 3, 6, 12), 20, 0.25, 1e-12, 3, "max_iter before err < tol")


def _build(name, spec):
    kind, units, n_add, restart, tol, max_iter, why = spec
    n, rowptr, col = graph(kind)
    return Case(name, n, rowptr, col, units(), n_add, restart, tol() if callable(tol) else tol, max_iter, why)


@functools.lru_cache(maxsize=None)
def case(name):
    return _build(name, NOT_CONVERGED if name == "not_converged" else _SPECS[name])


@functools.lru_cache(maxsize=None)
def mirror(name):
    """treat as read-only"""
    c = case(name)
    return M.table(c.rowptr, c.col, c.units, c.n_add, c.restart, c.tol, c.max_iter)


def max_degree(c):
    return int(np.diff(c.rowptr).max())


def seed_table(c, max_size=None, pad=-1):
    """(nodes [U, max_size], sizes [U]) int32 as the kernel takes them"""
    width = max_size or max(1, max(len(u) for u in c.units))
    nodes = np.full((len(c.units), width), pad, np.int32)
    for i, u in enumerate(c.units):
        nodes[i, :len(u)] = u
    return nodes, np.array([len(u) for u in c.units], np.int32)


# ---- the null's cases: p [R, n] tables built by hand, so that sd = 0, ties in ge and ties in z are certain --------------------------------

def null_case(name):
    """-> (p [n_sets, R, n], seeds per set, n_add)"""
    rng = np.random.RandomState(41)
    if name == "r3":                                       # the smallest null; n past one thread each
        n, R = 1500, 3
        p = rng.rand(3, R, n)
        seeds = _u([1, 700, 1499], [5], list(range(0, 1500, 7)))
    elif name == "r65":
        n, R = 300, 65
        p = rng.rand(3, R, n)
        seeds = _u([0, 1, 2], [299], [150, 151])
    elif name == "flat":                                   # sd = 0, ge ties, tied z (0 for many; equal z at different p)
        n, R = 200, 5
        p = rng.rand(3, R, n)
        p[:, 1:, :50] = 0.25                               # sd = 0 on nodes 0 .. 49: z = 0 whatever p_0 is
        p[:, 0, 20:30] = 0.25                              # obs = every null sample: ge = R - 1
        p[:, 2, 60:70] = p[:, 0, 60:70]                    # one sample equal to obs: >= counts it, > does not
        p[:, :, 100:120] = p[:, :, 80:100]                 # twenty nodes with the bits of twenty others: z, p and all tie
        p[:, 0, 120:130] = 2.0 * p[:, 0, 130:140]          # (below) equal z at different p: the null scaled with obs
        p[:, 1:, 120:130] = 2.0 * p[:, 1:, 130:140]
        seeds = _u([3, 25, 64, 101], [], [130])
    else:
        raise KeyError(name)
    return p, seeds, {"r3": 1024, "r65": 17, "flat": 60}[name]


NULL_CASES = ("r3", "r65", "flat")
