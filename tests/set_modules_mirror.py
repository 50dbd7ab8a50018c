"""Numpy / plain Python statement of the component search of csrc/set_modules.hip, for tests only.

  * components(rowptr, col, members): the induced subgraph of one unit by a plain union-find -> (lcc, n_comp, n_edges, labels); labels[i]
    is the position within the unit of the smallest member of i's component.  Two members are adjacent when one is in the other's CSR
    row; a stored self loop is ignored; n_edges counts the hits (i, j), j > i, found in row i;
  * largest_label(labels): the label of the largest component, the smaller label of two as large (the members file's in_lcc);
  * module_nulls(): components over a set and proximity_mirror.random_sets of it -- the integer tables of the golden file;
  * ABLATIONS: named wrong rules components / largest_label take as `ablate`; tests/test_set_modules_mirror.py shows that every one
    changes an asserted output of some case of tests/set_modules_cases.py.
"""
from __future__ import annotations

import os

import numpy as np

import proximity_mirror as PM

ABLATIONS = {
    "one_sweep": "a single sweep of min-label propagation over the edges, no iteration to a fixed point",
    "rounds_32": "min-label propagation stopped after 32 rounds",
    "miss_last": "the binary search of the member list never finds the last member",
    "miss_first": "the binary search of the member list never finds the first member",
    "row_64": "rows cut at 64 entries",
    "self_loop_edge": "a stored self loop counted as an edge",
    "tie_larger": "of two largest components the one with the larger label",
    "past_size": "the entry after the last member read as a member",
}


def _hits(rowptr, col, members, ablate=None):
    """the hits (i, j), positions within the unit, i != j unless self loops count, of every member's row against the member list"""
    m = len(members)
    if m == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    members = np.asarray(members, np.int64)
    start = np.asarray(rowptr)[members].astype(np.int64)
    deg = np.asarray(rowptr)[members + 1].astype(np.int64) - start
    if ablate == "row_64":
        deg = np.minimum(deg, 64)
    total = int(deg.sum())
    i = np.repeat(np.arange(m), deg)
    c = np.asarray(col)[np.repeat(start - (np.cumsum(deg) - deg), deg) + np.arange(total)].astype(np.int64)
    lo, hi = (1 if ablate == "miss_first" else 0), (m - 1 if ablate == "miss_last" else m)
    searched = members[lo:hi]
    j = np.searchsorted(searched, c)
    ok = j < len(searched)
    ok[ok] = searched[j[ok]] == c[ok]
    i, j = i[ok], j[ok] + lo
    if ablate != "self_loop_edge":
        keep = i != j
        i, j = i[keep], j[keep]
    return i, j


def _labels_by_propagation(m, i, j, rounds, in_place):
    lab = list(range(m))
    for _ in range(rounds):
        new = lab if in_place else list(lab)
        for a, b in zip(i, j):
            low = min(lab[a], lab[b]) if not in_place else min(new[a], new[b])
            new[a] = min(new[a], low)
            new[b] = min(new[b], low)
        lab = new
    return lab


def components(rowptr, col, members, ablate=None, tail=()):
    """-> (lcc, n_comp, n_edges, labels int64 [len(members)]); tail: the entries of the unit's row after its size (read only by the
    `past_size` ablation: the first of them counts as one more member, an isolated one where it is no node or out of order)"""
    members = [int(v) for v in members]
    extra = 0
    if ablate == "past_size" and len(tail):
        t, n = int(tail[0]), len(rowptr) - 1
        if 0 <= t < n and (not members or t > members[-1]):
            members = members + [t]
        else:
            extra = 1
    m = len(members)
    i, j = _hits(rowptr, col, members, ablate)
    i, j = i.tolist(), j.tolist()
    n_edges = sum(1 for a, b in zip(i, j) if b > a) + sum(1 for a, b in zip(i, j) if b == a)
    if ablate == "one_sweep":
        parent = _labels_by_propagation(m, i, j, 1, True)
    elif ablate == "rounds_32":
        parent = _labels_by_propagation(m, i, j, 32, False)
    else:
        parent = list(range(m))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for a, b in zip(i, j):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
        parent = [find(x) for x in range(m)]
    labels = np.array(parent, np.int64).reshape(-1)
    count = np.bincount(labels, minlength=1) if m else np.zeros(1, np.int64)
    return int(count.max()) if m else 0, len(set(parent)) + extra, n_edges, labels


def largest_label(labels, ablate=None):
    """the label of the largest component (None for an empty unit); of two as large the smaller label"""
    labels = np.asarray(labels, np.int64)
    if len(labels) == 0:
        return None
    count = np.bincount(labels)
    best = np.flatnonzero(count == count.max())
    return int(best[-1] if ablate == "tie_larger" else best[0])


def table(rowptr, col, units):
    """units: a list of member arrays -> int64 lcc, n_comp, n_edges [len(units)] and the list of labels"""
    out = [components(rowptr, col, u) for u in units]
    return (np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out], np.int64), np.array([o[2] for o in out], np.int64),
            [o[3] for o in out])


def module_nulls(rowptr, col, members, node_bin, bin_list, seed, side, set_index, n_random):
    """-> int64 [3, n_random + 1] (lcc, n_comp, n_edges; sample 0 the set itself) and sizes [n_random + 1]"""
    units = [np.asarray(members, np.int64)] + PM.random_sets(members, node_bin, bin_list, seed, side, set_index, n_random)
    lcc, n_comp, n_edges, _ = table(rowptr, col, units)
    return np.stack([lcc, n_comp, n_edges]), np.array([len(u) for u in units], np.int64)


# ---- the fixture (tests/golden/set_modules_2016.npz, made by tests/golden/make_set_modules_fixture.py from proximity_2016.npz alone) ----

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "set_modules_2016.npz")
SEED, N_RANDOM, MIN_BIN = 452456, 1000, 100


def fixture_inputs(fx):
    """(bins, node_bin, disease node sets, drug node sets) of a proximity_mirror.Fixture, as module_table builds them"""
    bin_list = PM.bins(fx.net.degree, MIN_BIN)
    return bin_list, PM.bin_of(bin_list, fx.net.n), [fx.net.node_set(s) for s in fx.diseases], [fx.net.node_set(s) for s in fx.drugs]


def load_fixture(path=FIXTURE):
    """{"disease": int16 [3, 78, 1001] (lcc, n_comp, n_edges), "disease_size": int16 [78, 1001], "drug": int16 [3, 238] (observed)}"""
    return PM.unpack(np.load(path))
