"""Inputs of the tests of the component search (tests/test_set_modules_mirror.py on the CPU, tests/test_gpu_set_modules_ops.py on the GPU):
named, small, deterministic, each built for a branch of csrc/set_modules.hip and carrying the values it must give (`want`).

A case is a graph (n, rowptr, col: symmetric CSR, columns ascending; `selfloop` keeps a stored self loop) and a list of units (ascending
member arrays); case.max_size is the table's row length and case.fill what stands past every size.
  size_<s>_path     one path threaded through the s members in shuffled node order (min-label propagation needs about s rounds); every
                    member also has a neighbour outside the set.  s runs over SIZES: both sides of the one-wave workgroup (max_size <= 64),
                    of the 256 threads, of a wave's 64 lanes, and the LDS limit 4,096.  The table's row is exactly s long;
  size_<s>_apart    no edge among the members, three outside neighbours each: lcc 1, n_comp s, n_edges 0;
  size_<s>_tie      two components of equal size and a smaller one (s >= 63);
  k65               65 mutually adjacent members;
  hub               a hub of degree 2,300 with 100 of its leaves at the row positions HUB_AT (its row is searched from the members' side),
                    the leaves alone (100 singletons), and the hub with all its leaves (its row is walked, lanes over entries);
  bounds            members 0 and n - 1 adjacent; rows with neighbours below the first member and above the last;
  selfloop          a stored self loop on a member;
  oneway            the one case whose CSR is not symmetric: an entry stored in one row only still joins its two members;
  many_3000         3,000 units of sizes 0 .. 130 in one launch, -1 and 0x7fffffff past every size;
  grid_70000        70,000 units of sizes 1 .. 3 in one launch (past a 16-bit grid dimension, past the kernel's workgroup stride).
Mirror results are computed once and shared; treat every array as read-only."""
import functools
import types

import numpy as np

import set_modules_mirror as M

N = 5000
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)
HUB, HUB_DEG = 2500, 2300
HUB_AT = (0, 63, 64, 65, 255, 256, HUB_DEG - 1)
FILL = (-1, 0x7FFFFFFF)


def csr(n, edges, loops=(), oneway=()):
    """undirected edge list (+ stored self loops, + entries (row, column) stored in one row only) -> (rowptr, col) int32, no duplicates,
    columns ascending; symmetric without `oneway`"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    lp = np.asarray(loops, np.int64).reshape(-1)
    ow = np.asarray(oneway, np.int64).reshape(-1, 2)
    a, b = np.concatenate([e[:, 0], e[:, 1], lp, ow[:, 0]]), np.concatenate([e[:, 1], e[:, 0], lp, ow[:, 1]])
    key = np.unique(a * n + b)
    a, b = key // n, key % n
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(a, minlength=n), out=rowptr[1:])
    return rowptr, b.astype(np.int32)


def _case(name, why, edges, units, want=None, max_size=None, loops=(), oneway=(), fill=FILL, n=N):
    rowptr, col = csr(n, edges, loops, oneway)
    units = [np.asarray(u, np.int64) for u in units]
    for u in units:
        assert (np.diff(u) > 0).all() and (len(u) == 0 or (u[0] >= 0 and u[-1] < n))
    return types.SimpleNamespace(name=name, why=why, n=n, rowptr=rowptr, col=col, units=units, want=want, fill=fill, symmetric=not len(oneway),
                                 max_size=max_size or max(1, max(len(u) for u in units)))


def _outside(rng, members, per):
    """`per` neighbours outside the set for every member"""
    out = np.setdiff1d(np.arange(N), members)
    return [(v, w) for v in members for w in rng.choice(out, per, replace=False)]


def _size_path(s):
    rng = np.random.RandomState(100 + s)
    members = np.sort(rng.choice(N, s, replace=False))
    order = rng.permutation(members)
    edges = list(zip(order[:-1], order[1:])) + (_outside(rng, members, 1) if s else [])
    return _case(f"size_{s}_path", "one path in shuffled node order", edges, [members], want=[(s, min(s, 1), max(s - 1, 0))])


def _size_apart(s):
    rng = np.random.RandomState(200 + s)
    members = np.sort(rng.choice(N, s, replace=False))
    return _case(f"size_{s}_apart", "no edge among the members", _outside(rng, members, 3) if s else [], [members], want=[(min(s, 1), s, 0)])


def _tree(rng, nodes):
    return [(nodes[i], nodes[rng.randint(0, i)]) for i in range(1, len(nodes))]


def _size_tie(s):
    rng = np.random.RandomState(300 + s)
    members = np.sort(rng.choice(N, s, replace=False))
    k = s // 2 - 1
    order = rng.permutation(members)
    parts = (order[:k], order[k:2 * k], order[2 * k:])
    assert 1 <= len(parts[2]) < k
    edges = _tree(rng, parts[0]) + _tree(rng, parts[1]) + _tree(rng, parts[2]) + _outside(rng, members, 1)
    c = _case(f"size_{s}_tie", "two components of equal size and a smaller one", edges, [members], want=[(k, 3, s - 3)])
    pos = {int(v): i for i, v in enumerate(members)}
    c.tie_labels = sorted(min(pos[int(v)] for v in p) for p in parts[:2])      # the labels of the two equal components
    return c


def _k65():
    rng = np.random.RandomState(65)
    members = np.sort(rng.choice(N, 65, replace=False))
    edges = [(a, b) for a in members for b in members if a < b] + _outside(rng, members, 2)
    return _case("k65", "65 mutually adjacent members", edges, [members], want=[(65, 1, 65 * 64 // 2)])


def _hub():
    rng = np.random.RandomState(7)
    leaves = np.sort(rng.choice(np.setdiff1d(np.arange(N), [HUB]), HUB_DEG, replace=False))      # the hub's row, ascending
    at = np.sort(np.concatenate([HUB_AT, rng.choice(np.setdiff1d(np.arange(HUB_DEG), HUB_AT), 100 - len(HUB_AT), replace=False)]))
    picked = leaves[at]
    assert len(picked) == 100 and set(HUB_AT) <= set(at.tolist())
    edges = [(HUB, v) for v in leaves]
    with_hub = np.sort(np.concatenate([picked, [HUB]]))
    everything = np.sort(np.concatenate([leaves, [HUB]]))
    c = _case("hub", "a hub row of 2,300 entries against 101 members; its leaves alone; the hub with all its leaves", edges,
              [with_hub, picked, everything], want=[(101, 1, 100), (1, 100, 0), (HUB_DEG + 1, 1, HUB_DEG)])
    c.row_positions = at
    return c


def _bounds():
    edges = [(0, N - 1), (20, 5), (20, 4000), (20, 30), (10, 3), (10, 4), (30, 4999), (0, 1)]
    return _case("bounds", "members 0 and n - 1 adjacent; neighbours below the first member and above the last", edges,
                 [[0, 100, N - 1], [10, 20, 30], [0, N - 1]], want=[(2, 2, 1), (2, 2, 1), (2, 1, 1)], max_size=5)


def _selfloop():
    return _case("selfloop", "a stored self loop on a member", [(5, 9), (12, 40)], [[5, 9, 12], [9], [9, 12]], loops=[9, 12],
                 want=[(2, 2, 1), (1, 1, 0), (1, 2, 0)], max_size=4)


def _oneway():
    return _case("oneway", "entries stored in one row only: members are adjacent when one is in the other's row, an edge counts in row i "
                 "for j > i", [(50, 60)], [[10, 30], [11, 31], [10, 11, 30, 31]], oneway=[(30, 10), (11, 31)],
                 want=[(2, 1, 0), (2, 1, 1), (2, 2, 1)], max_size=4)


def _many():
    rng = np.random.RandomState(3000)
    dense = 700                                                     # the members come from a region dense enough for induced edges
    edges = np.concatenate([rng.randint(0, dense, (4 * dense, 2)), rng.randint(0, N, (3 * N, 2))])
    sizes = rng.randint(0, 131, 3000)
    sizes[:4] = (0, 130, 1, 64)
    units = [np.sort(rng.choice(dense, s, replace=False)) for s in sizes]
    return _case("many_3000", "3,000 units of sizes 0 .. 130 in one launch", edges, units, max_size=132)


GRID_REGION = 48


def _grid():
    rng = np.random.RandomState(70000)
    edges = np.concatenate([rng.randint(0, GRID_REGION, (200, 2)), rng.randint(0, N, (N, 2))])
    sizes = rng.randint(1, 4, 70000)
    pick = np.sort(np.argsort(rng.rand(70000, GRID_REGION), axis=1)[:, :3], axis=1)      # three distinct nodes per unit, ascending
    units = [pick[u, :s] for u, s in enumerate(sizes)]
    return _case("grid_70000", "70,000 units of sizes 1 .. 3 in one launch", edges, units, max_size=4)


_BUILDERS = {}
for _s in SIZES:
    _BUILDERS[f"size_{_s}_path"] = functools.partial(_size_path, _s)
    _BUILDERS[f"size_{_s}_apart"] = functools.partial(_size_apart, _s)
    if _s >= 63:
        _BUILDERS[f"size_{_s}_tie"] = functools.partial(_size_tie, _s)
_BUILDERS.update(k65=_k65, hub=_hub, bounds=_bounds, selfloop=_selfloop, oneway=_oneway, many_3000=_many, grid_70000=_grid)
SIZE_CASES = [k for k in _BUILDERS if k.startswith("size_")]
SMALL_CASES = SIZE_CASES + ["k65", "hub", "bounds", "selfloop", "oneway"]
CASES = list(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def table_arrays(c, max_size=None):
    """the case's set table -> (nodes [n_units, max_size] int32 with c.fill alternating past every size, sizes [n_units] int32)"""
    max_size = max_size or c.max_size
    nodes = np.empty((len(c.units), max_size), np.int32)
    nodes[:, 0::2], nodes[:, 1::2] = c.fill[0], c.fill[1]
    sizes = np.array([len(u) for u in c.units], np.int32)
    for k, u in enumerate(c.units):
        nodes[k, :len(u)] = u
    return nodes, sizes


def _small3(c):
    """closed form for units of at most 3 members: the three possible edges decide everything"""
    A = np.zeros((GRID_REGION, GRID_REGION), bool)
    rows = np.repeat(np.arange(c.n), np.diff(c.rowptr))
    m = (rows < GRID_REGION) & (c.col < GRID_REGION) & (rows != c.col)
    A[rows[m], c.col[m]] = True
    nodes, sizes = table_arrays(c)
    a, b, d = nodes[:, 0].clip(0, GRID_REGION - 1), nodes[:, 1].clip(0, GRID_REGION - 1), nodes[:, 2].clip(0, GRID_REGION - 1)
    e01, e02, e12 = A[a, b] & (sizes >= 2), A[a, d] & (sizes >= 3), A[b, d] & (sizes >= 3)
    n_edges = e01.astype(np.int64) + e02 + e12
    joined = np.minimum(n_edges, sizes - 1)
    lab = np.full((len(sizes), c.max_size), -1, np.int64)
    lab[:, 0] = 0
    l1 = np.where(e01 | (e02 & e12), 0, 1)
    l2 = np.where(e02 | (e12 & e01), 0, np.where(e12, 1, 2))
    lab[sizes >= 2, 1] = l1[sizes >= 2]
    lab[sizes >= 3, 2] = l2[sizes >= 3]
    return 1 + joined, sizes - joined, n_edges, lab


@functools.lru_cache(maxsize=None)
def mirror(name):
    """-> int64 lcc, n_comp, n_edges [n_units] and labels [n_units, max_size] (-1 past every size) of the case, read-only"""
    c = case(name)
    if name == "grid_70000":
        out = _small3(c)
    else:
        lcc, n_comp, n_edges, labels = M.table(c.rowptr, c.col, c.units)
        lab = np.full((len(c.units), c.max_size), -1, np.int64)
        for k, l in enumerate(labels):
            lab[k, :len(l)] = l
        out = (lcc, n_comp, n_edges, lab)
    for a in out:
        a.setflags(write=False)
    return out
