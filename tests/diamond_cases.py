"""The inputs of the DIAMOnD tests (tests/test_diamond_mirror.py on the CPU, tests/test_gpu_diamond_ops.py on the device): small graphs as
symmetric CSRs without self loops, columns ascending, and per case a list of seed sets (units), n_add and alpha.  Each is the smallest
shape at which one thing can go wrong; `why` names it.  mirror(name) is tests/diamond_mirror.py's table of the case, computed once.

Different (k', kb') can have hypergeometric tails that are equal as rationals or closer than the error of one log; which of two such
candidates wins is reproducible but implementation-defined (include/gssgcn.h).  So every case here is chosen (the random graphs' seeds
below were searched for it) so that at every step the runner-up's logp is more than MIN_GAP relative away from the winner's;
tests/test_diamond_mirror.py asserts that for every step of every case."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import diamond_mirror as M

MIN_GAP = 1e-9
MAX_NODES = 30720                 # gss_diamond_grow's limit on n
THREADS = 1024                    # its workgroup
MAX_BLOCKS = 1024                 # its grid: more units than this walk the grid stride
HUB, HUB_DEG = 0, 1150

Case = namedtuple("Case", "name n rowptr col units n_add alpha why")


def csr(n, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    key = np.unique(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
    a, b = key // n, key % n
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(a, minlength=n), out=rowptr[1:])
    return rowptr, b.astype(np.int32)


def gnp(n, p, seed):
    rng = np.random.RandomState(seed)
    iu = np.triu_indices(n, 1)
    keep = rng.rand(len(iu[0])) < p
    return np.stack([iu[0][keep], iu[1][keep]], axis=1)


def draw_units(n, count, size, seed, lo=None):
    rng = np.random.RandomState(seed)
    return [np.sort(rng.choice(n, size if lo is None else rng.randint(lo, size + 1), replace=False)).astype(np.int32) for _ in range(count)]


def _star_edges():
    """the hub with HUB_DEG leaves (1 .. HUB_DEG), a side region of 750 nodes (sparse random), and 300 leaves tied to the side region"""
    n = 1 + HUB_DEG + 750
    rng = np.random.RandomState(5)
    side0 = 1 + HUB_DEG
    edges = [(HUB, v) for v in range(1, side0)]
    edges += [(side0 + a, side0 + b) for a, b in gnp(750, 0.008, 6)]
    edges += [(int(v), side0 + int(rng.randint(750))) for v in rng.choice(np.arange(1, side0), 300, replace=False)]
    return n, edges


def _odd_edges(seed):
    """41 nodes: a path 0-1-2-3-4-5 apart from everything, a ring 6 .. 25 with chords, node 26 alone, 27 .. 40 random and tied to the ring"""
    rng = np.random.RandomState(seed)
    edges = [(i, i + 1) for i in range(5)]
    edges += [(6 + i, 6 + (i + 1) % 20) for i in range(20)] + [(6 + int(a), 6 + int(b)) for a, b in rng.randint(0, 20, (9, 2))]
    edges += [(27 + int(a), 27 + int(b)) for a, b in rng.randint(0, 14, (16, 2))] + [(27 + i, 6 + int(rng.randint(20))) for i in range(14)]
    return 41, edges


@functools.lru_cache(maxsize=None)
def _graphs(kind):
    if kind == "n40":
        return (40,) + csr(40, gnp(40, 0.2, 3))
    if kind == "n300":
        return (300,) + csr(300, gnp(300, 0.03, 1))
    if kind == "n1500":
        return (1500,) + csr(1500, gnp(1500, 0.006, 2))
    if kind == "star":
        n, e = _star_edges()
        return (n,) + csr(n, e)
    if kind == "odd":
        n, e = _odd_edges(4)
        return (n,) + csr(n, e)
    if kind == "ring":
        n = MAX_NODES
        return (n,) + csr(n, [(i, (i + 1) % n) for i in range(n)])
    raise KeyError(kind)


def _tail_units():
    """600 seeds of which 50 are leaves of the hub: the hub is a candidate with kb' = 50, k' = 1150, s' = 600 -- a sum of 550 terms"""
    rng = np.random.RandomState(9)
    leaves = rng.choice(np.arange(1, 1 + HUB_DEG), 50, replace=False)
    side = 1 + HUB_DEG + rng.choice(750, 550, replace=False)
    return [np.sort(np.concatenate([leaves, side])).astype(np.int32)]


def _star_units():
    rng = np.random.RandomState(8)
    as_seed = np.sort(np.concatenate([[HUB], 1 + HUB_DEG + rng.choice(750, 6, replace=False)])).astype(np.int32)
    as_candidate = np.sort(np.concatenate([rng.choice(np.arange(1, 1 + HUB_DEG), 30, replace=False),       # 30 leaves: the hub is the first node added
                                           1 + HUB_DEG + rng.choice(750, 5, replace=False)])).astype(np.int32)
    return [as_seed, as_candidate]


_SPECS = {
    # name: (graph, units, n_add, alpha, why)
    "n40_a1": ("n40", lambda: draw_units(40, 3, 5, 12), 30, 1, "dense-ish, n no multiple of 64, most of the graph added"),
    "n40_a3": ("n40", lambda: draw_units(40, 3, 5, 12), 30, 3, "the seed weight in kb', k', s' and N'"),
    "n300_a1": ("n300", lambda: draw_units(300, 6, 12, 12), 100, 1, "100 steps; the units of the split over three calls"),
    "n300_a2": ("n300", lambda: draw_units(300, 6, 12, 12), 100, 2, "100 steps with a seed weight"),
    "n1500": ("n1500", lambda: draw_units(1500, 2, 40, 13), 60, 1, "more nodes than the workgroup has lanes"),
    "star": ("star", _star_units, 12, 1, "a row longer than the workgroup: the hub as seed (unit 0) and as candidate (unit 1)"),
    "tail": ("star", _tail_units, 6, 1, "a tail sum of 550 terms"),
    "odd": ("odd", lambda: [np.array(u, np.int32) for u in ([1, 3], [26], [8, 10, 26], [7], [], [0, 1, 2, 3, 4, 5])], 10, 1,
            "a component used up before n_add, a seed without neighbours alone and among others, one seed, no seed, nothing to add"),
    "odd_a2": ("odd", lambda: [np.array(u, np.int32) for u in ([1, 3], [8, 10, 26], [7])], 10, 2, "the same with a seed weight"),
    "ring": ("ring", lambda: [np.array([0, 5, 9], np.int32), np.array([30719], np.int32)], 8, 1, "n at the limit"),
    "many": ("n300", lambda: draw_units(300, MAX_BLOCKS + 6, 8, 14, lo=3), 3, 1, "more units than workgroups"),
}
CASES = tuple(_SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    kind, units, n_add, alpha, why = _SPECS[name]
    n, rowptr, col = _graphs(kind)
    return Case(name, n, rowptr, col, units(), n_add, alpha, why)


@functools.lru_cache(maxsize=None)
def mirror(name):
    """treat as read-only"""
    c = case(name)
    return M.table(c.rowptr, c.col, c.units, c.n_add, c.alpha)


def max_degree(c):
    return int(np.diff(c.rowptr).max())


def seed_table(c, max_size=None, pad=-1):
    """(seeds [U, max_size], sizes [U]) int32 as the kernel takes them"""
    width = max_size or max(1, max(len(u) for u in c.units))
    seeds = np.full((len(c.units), width), pad, np.int32)
    for i, u in enumerate(c.units):
        seeds[i, :len(u)] = u
    return seeds, np.array([len(u) for u in c.units], np.int32)
