"""The inputs of the seed connector tests (tests/test_connectors_mirror.py on the CPU, tests/test_gpu_connectors_ops.py on the device):
small graphs as symmetric CSRs without self loops, columns ascending, and per case a list of seed sets (units) and n_add.  Each is the
smallest shape at which one thing can go wrong; `why` names it.  mirror(name) is tests/connectors_mirror.py's table of the case,
computed once.  Every quantity is an integer and the key is a total order: the device must equal the mirror everywhere."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

import connectors_mirror as M
from diamond_cases import HUB, HUB_DEG, _graphs as _diamond_graphs, csr, draw_units, gnp

MAX_NODES = 30720                 # gss_seed_connectors' limit on n
MAX_SEEDS = 4096                  # ... on max_size
MAX_MEMBERS = 8192                # ... on max_size + n_add
MAX_DEG = (1 << 20) - 1           # ... on max_deg
THREADS = 1024                    # its workgroup: a longer row is walked by all of it
MAX_BLOCKS = 1024                 # its grid: more units than this walk the grid stride
K_ROOTS = 8                       # csrc/seed_connect.hip kRoots: distinct components a lane holds; a candidate next to more takes the slow path

Case = namedtuple("Case", "name n rowptr col units n_add why")


def _once_edges():
    """0-1-2-3 a path of seeds, 4 a seed apart; 5 is next to all of 0..3 and to 4 (tot = 1 + 4 + 1, not 1 + 4 x 4 + 1); 6 next to 3 only"""
    return 7, [(0, 1), (1, 2), (2, 3), (5, 0), (5, 1), (5, 2), (5, 3), (5, 4), (6, 3)]


def _stars_edges():
    """centre 0 with 70 leaves 1..70, centre 71 with K_ROOTS + 1 leaves 72..80, centre 81 with K_ROOTS leaves 82..89; every leaf has a
    pendant node of its own (leaf + 100), so each step has fast-path candidates beside the centre"""
    leaves = list(range(1, 71)) + list(range(72, 72 + K_ROOTS + 1)) + list(range(82, 82 + K_ROOTS))
    edges = [(0, v) for v in range(1, 71)] + [(71, v) for v in range(72, 72 + K_ROOTS + 1)] + [(81, v) for v in range(82, 82 + K_ROOTS)]
    return 200, edges + [(v, v + 100) for v in leaves]


def _overtake_edges():
    """seeds 0..4 a path (the first LCC, 5 nodes) with the pendant 5; seeds 6..9 and 10..13 two paths that 14 joins (9 nodes); 15 next to 14"""
    edges = [(i, i + 1) for i in range(4)] + [(4, 5)] + [(6, 7), (7, 8), (8, 9), (10, 11), (11, 12), (12, 13), (14, 9), (14, 10), (14, 15)]
    return 16, edges


def _ties_edges():
    """seeds 0, 1, 2, 3 apart.  4 joins 0 and 1 with degree 3 (pendant 6), 5 joins 0 and 1 with degree 2: the degree decides for 5.  7 and 8
    both join 2 and 3 with degree 2: the node decides for 7"""
    return 9, [(4, 0), (4, 1), (4, 6), (5, 0), (5, 1), (7, 2), (7, 3), (8, 2), (8, 3)]


@functools.lru_cache(maxsize=None)
def _graph(kind):
    if kind in ("n300", "star", "odd"):
        return _diamond_graphs(kind)
    if kind == "n40":
        return (40,) + csr(40, gnp(40, 0.12, 3))
    if kind == "ring":
        n = MAX_NODES
        return (n,) + csr(n, [(i, (i + 1) % n) for i in range(n)])
    n, edges = {"once": _once_edges, "stars": _stars_edges, "overtake": _overtake_edges, "ties": _ties_edges}[kind]()
    return (n,) + csr(n, edges)


def _star_units():
    rng = np.random.RandomState(8)
    as_seed = np.sort(np.concatenate([[HUB], 1 + HUB_DEG + rng.choice(750, 6, replace=False)])).astype(np.int32)
    as_connector = np.sort(rng.choice(np.arange(1, 1 + HUB_DEG), 30, replace=False)).astype(np.int32)   # 30 leaves: the hub joins them all
    return [as_seed, as_connector]


def _ints(*units):
    return lambda: [np.array(u, np.int32) for u in units]


_SPECS = {
    # name: (graph, units, n_add, why)
    "n40": ("n40", lambda: draw_units(40, 5, 6, 12, lo=2), 30, "dense-ish, n no multiple of 64, n_add beyond the stop: the -1 fill"),
    "n300": ("n300", lambda: draw_units(300, 6, 14, 12, lo=5), 40, "several steps per unit; the units of the split over three calls"),
    "capped": ("n300", lambda: draw_units(300, 6, 14, 12, lo=5), 2, "n_add reached before the stop rule"),
    "once": ("once", _ints([0, 1, 2, 3, 4]), 4, "a component reached through four neighbours is counted once"),
    "stars": ("stars", _ints(range(1, 71), range(72, 72 + K_ROOTS + 1), range(82, 82 + K_ROOTS)), 3,
              "a centre next to 70, to K_ROOTS + 1 (the slow path) and to K_ROOTS (the fast path's last) singleton components"),
    "overtake": ("overtake", _ints([0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13]), 5,
                 "two components merge through a node and overtake the largest: the first LCC ends outside the final one"),
    "ties": ("ties", _ints([0, 1], [2, 3], [0, 1, 2, 3]), 3, "a tie on L' that the degree decides, one that the node index decides"),
    "star": ("star", _star_units, 6, "a row longer than the workgroup: the hub as seed (unit 0) and as the first connector (unit 1)"),
    "odd": ("odd", _ints([1, 3], [26], [8, 10, 26], [7], [], [0, 1, 2, 3, 4, 5], range(6, 16)), 10,
            "a bridge, a seed without neighbours alone and among others, one seed, no seed, a connected set without and with candidates"),
    "ring": ("ring", _ints([0, 2, 4, 6], [0, 3, 6], [1, MAX_NODES - 1], [MAX_NODES - 1]), 5,
             "n at the limit: seeds two apart (gains of 2), three apart (no gain), across the last node"),
    "many": ("n300", lambda: draw_units(300, MAX_BLOCKS + 6, 8, 14, lo=3), 3, "more units than workgroups"),
}
CASES = tuple(_SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    kind, units, n_add, why = _SPECS[name]
    n, rowptr, col = _graph(kind)
    return Case(name, n, rowptr, col, units(), n_add, why)


@functools.lru_cache(maxsize=None)
def mirror(name):
    """treat as read-only"""
    c = case(name)
    return M.table(c.rowptr, c.col, c.units, c.n_add)


def max_degree(c):
    return int(np.diff(c.rowptr).max())


def seed_table(c, max_size=None, pad=-1):
    """(seeds [U, max_size], sizes [U]) int32 as the kernel takes them"""
    width = max_size or max(1, max(len(u) for u in c.units))
    seeds = np.full((len(c.units), width), pad, np.int32)
    for i, u in enumerate(c.units):
        seeds[i, :len(u)] = u
    return seeds, np.array([len(u) for u in c.units], np.int32)
