"""The inputs of the Steiner tree tests (tests/test_steiner_mirror.py on the CPU, tests/test_gpu_steiner_ops.py on the device): small
graphs as symmetric CSRs without self loops, columns ascending, and per case a list of terminal sets (units) and max_add.  Each is the
smallest shape at which one thing can go wrong; `why` names it.  mirror(name) is tests/steiner_mirror.py's table of the case, computed
once.  Every quantity is an integer and both orders are total: the device must equal the mirror everywhere."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import steiner_mirror as M
from diamond_cases import HUB, HUB_DEG, _graphs as _diamond_graphs, csr, draw_units, gnp

MAX_NODES = 30720                 # gss_steiner_trees' limit on n
MAX_SEEDS = 4096                  # ... on max_size
MAX_DEG = (1 << 20) - 1           # ... on max_deg
LDS_BUDGET = 160 * 1024 - 512     # ... on 4 n + 16 max_size
THREADS = 1024                    # its workgroup
MAX_BLOCKS = 1024                 # its grid: more units than this walk the grid stride
LANE_ROW = 32                     # csrc/steiner.hip kLane: a longer row is walked by a wave
SIDE = 9                          # the lattice's side
BIG_N = 6000                      # nodes of the graph that holds up to 4,096 terminals
FAR = 20000                       # the open ring's second terminal: w = 20,000 > 2^14

Case = namedtuple("Case", "name n rowptr col units max_add why")


def _parts_edges():
    """a path 0 .. 5, a ring 6 .. 15, a star 16 with leaves 17 .. 20, node 21 alone, a square 22 .. 25 that no unit touches"""
    edges = [(i, i + 1) for i in range(5)] + [(6 + i, 6 + (i + 1) % 10) for i in range(10)] + [(16, v) for v in range(17, 21)]
    return 26, edges + [(22, 23), (23, 24), (24, 25), (25, 22)]


def _lattice_edges():
    at = lambda r, c: r * SIDE + c  # noqa: E731
    edges = [(at(r, c), at(r, c + 1)) for r in range(SIDE) for c in range(SIDE - 1)]
    return SIDE * SIDE, edges + [(at(r, c), at(r + 1, c)) for r in range(SIDE - 1) for c in range(SIDE)]


def _big_edges():
    rng = np.random.RandomState(21)
    return BIG_N, np.concatenate([rng.randint(0, BIG_N, (3 * BIG_N, 2)), np.stack([np.arange(BIG_N - 1), np.arange(1, BIG_N)], axis=1)[::7]])


@functools.lru_cache(maxsize=None)
def _graph(kind):
    if kind in ("n40", "n300", "star"):
        return _diamond_graphs(kind)
    if kind == "n12":
        return (12,) + csr(12, gnp(12, 0.22, 5))
    if kind == "k65":
        return (65,) + csr(65, gnp(65, 2.0, 0))
    if kind == "ring":
        n = MAX_NODES
        return (n,) + csr(n, [(i, (i + 1) % n) for i in range(n)])
    if kind == "open":
        n = MAX_NODES
        return (n,) + csr(n, [(i, i + 1) for i in range(n - 1)])
    if kind == "mixed":                          # the lattice with its nodes renumbered at random: (u, v) and (v, u) order bridges differently
        n, edges = _lattice_edges()
        return (n,) + csr(n, np.random.RandomState(17).permutation(n)[np.asarray(edges)])
    n, edges = {"parts": _parts_edges, "lattice": _lattice_edges, "big": _big_edges}[kind]()
    return (n,) + csr(n, edges)


def _ints(*units):
    return lambda: [np.array(u, np.int32) for u in units]


def _star_units():
    """the hub of degree HUB_DEG as a terminal; as the Steiner node between two of its leaves; as the end of a bridge: leaf 1 is a terminal
    and so is the side node next to another leaf (the hub is at distance 1 of the one, that leaf at distance 1 of the other)"""
    n, rowptr, col = _graph("star")
    side0 = 1 + HUB_DEG
    tied = next(v for v in range(2, side0) if rowptr[v + 1] - rowptr[v] == 2)          # a leaf with a neighbour in the side region
    far = int(col[rowptr[tied]:rowptr[tied + 1]].max())
    rng = np.random.RandomState(8)
    many = np.sort(np.concatenate([[HUB], side0 + rng.choice(750, 12, replace=False)])).astype(np.int32)
    return [many, np.array([3, 900], np.int32), np.array([1, far], np.int32), np.array([HUB, 5], np.int32)]


def _sized(T, seed):
    return lambda: [np.sort(np.random.RandomState(seed).choice(BIG_N, T, replace=False)).astype(np.int32)]


_SPECS = {
    # name: (graph, units, max_add, why)
    "n12": ("n12", lambda: draw_units(12, 8, 5, 3, lo=2), 12, "small enough for the optimum by enumeration"),
    "n40": ("n40", lambda: draw_units(40, 5, 6, 12, lo=2), 40, "dense-ish, n no multiple of 64"),
    "n300": ("n300", lambda: draw_units(300, 6, 14, 12, lo=5), 64, "several levels and rounds; the units of the split over three calls"),
    "capped": ("n300", lambda: draw_units(300, 6, 14, 12, lo=5), 2, "n_steiner above max_add: the first two are listed, the counts stay"),
    "parts": ("parts", _ints([], [7], [0, 1], [0, 2, 5], [0, 4, 6, 11, 17, 19, 21], [21], [17, 18, 19, 20]), 12,
              "no terminal, one, two adjacent (w = 1), all on one path, three components and an isolated terminal, nodes no terminal reaches"),
    "lattice": ("lattice", _ints([0, SIDE - 1, SIDE * (SIDE - 1), SIDE * SIDE - 1], [0, 40, 80], [4, 36, 44, 76], [0, 2, 4, 6, 8, 72, 74, 76, 78, 80],
                                 [10, 16, 40, 64, 70]), 81, "nearest terminals and bridge weights tie everywhere: the src rule and the (u, v) order decide"),
    "mixed": ("mixed", lambda: draw_units(SIDE * SIDE, 6, 6, 2, lo=2), 81, "the lattice's ties under a numbering in which (w, u, v) and (w, v, u) differ"),
    "k65": ("k65", _ints([0, 1, 2], range(65), [5], [0, 64]), 4, "a complete graph: rows of 64, every bridge of weight 1"),
    "star": ("star", _star_units, 20, "a row longer than the workgroup: the hub as terminal, as Steiner node and as the end of a bridge"),
    "t63": ("big", _sized(63, 1), 300, "one terminal short of a wave"),
    "t64": ("big", _sized(64, 2), 300, "a wave of terminals"),
    "t65": ("big", _sized(65, 3), 300, "one more than a wave"),
    "t1023": ("big", _sized(1023, 4), 600, "one short of the workgroup"),
    "t1024": ("big", _sized(1024, 5), 600, "the workgroup"),
    "t1025": ("big", _sized(1025, 6), 600, "one more than the workgroup"),
    "t4096": ("big", _sized(MAX_SEEDS, 7), 64, "max_size at its limit: src = 4,095 in twelve bits"),
    "ring": ("ring", _ints([0, 2, 4, 6], [0, MAX_NODES // 2], [0, MAX_NODES - 2], [MAX_NODES - 1]), 5,
             "n at the limit: terminals two apart, half a ring apart (7,680 levels, 15,359 Steiner nodes), across the last node"),
    "open": ("open", _ints([0, FAR]), 3, "w beyond 2^14 (on a ring of n nodes no two terminals are more than n / 2 = 15,360 apart): 10,000 levels"),
    "many": ("n300", lambda: draw_units(300, MAX_BLOCKS + 6, 8, 14, lo=3), 8, "more units than workgroups: 1,030 in one launch"),
}
CASES = tuple(_SPECS)
SMALL = ("n12", "n40", "n300", "parts", "lattice", "mixed", "k65", "star")        # where every ablation is run


@functools.lru_cache(maxsize=None)
def case(name):
    kind, units, max_add, why = _SPECS[name]
    n, rowptr, col = _graph(kind)
    return Case(name, n, rowptr, col, units(), max_add, why)


@functools.lru_cache(maxsize=None)
def mirror(name, ablation=None):
    """treat as read-only"""
    c = case(name)
    return M.table(c.rowptr, c.col, c.units, ablation)


def max_degree(c):
    return int(np.diff(c.rowptr).max())


def seed_table(c, max_size=None, pad=-1):
    """(seeds [U, max_size], sizes [U]) int32 as the kernel takes them"""
    width = max_size or max(1, max(len(u) for u in c.units))
    seeds = np.full((len(c.units), width), pad, np.int32)
    for i, u in enumerate(c.units):
        seeds[i, :len(u)] = u
    return seeds, np.array([len(u) for u in c.units], np.int32)
