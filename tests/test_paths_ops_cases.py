"""CPU: the conditions tests/test_gpu_paths_ops.py rests on, established on the inputs of tests/paths_ops_cases.py with the numpy
mirrors (tests/paths_mirror.py, tests/trace_mirror.py) and, for the small cases, networkx's enumeration of every shortest path: a case
that loses the property it exists for fails here and not on the GPU.

  boundary_count_graph     the products are exactly 2^53; which rows are read by one lane and which by the whole wave; the mirror
                           accepts 2^53 at the top node and refuses 2^53 + 1 naming it, for both chain placements
  lane_local_overcount     the one row in which a single lane holds the whole overflow
  tie_rule_graph           row lengths, the first-carrier positions, the lanes that own the hubs, and the closed form of dist / next
                           against mirror_trees (and against networkx for L = 32, 33)
  tie_weight_graph         rows of 33 / 64 / 65 successors, all one hop closer, and that the weight tables do tie
  between_graph            256 < n < 512, the named pairs (many routes over both 256-node iterations, one route, source = target,
                           unreachable)
  row_boundary_graph       equal neighbours across row boundaries that are no repeat, and the repeats of each variant"""
import os
import sys

import networkx as nx
import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import paths_mirror as M  # noqa: E402
import paths_ops_cases as K  # noqa: E402
import trace_mirror as T  # noqa: E402


def row_lengths(adj):
    return np.diff(adj.indptr)


def digraph(adj):
    G = nx.DiGraph()
    G.add_nodes_from(range(adj.shape[0]))
    rows = np.repeat(np.arange(adj.shape[0]), np.diff(adj.indptr))
    G.add_edges_from(zip(rows.tolist(), adj.indices.tolist()))
    return G


def enumerated(adj, targets):
    """dist, next (smallest first hop over all shortest paths) and the number of shortest paths, from networkx"""
    G = digraph(adj)
    n = adj.shape[0]
    dist = np.full((len(targets), n), 255, np.uint8)
    nxt = np.full((len(targets), n), -1, np.int32)
    sigma = np.zeros((len(targets), n))
    for q, t in enumerate(targets):
        for v in range(n):
            try:
                paths = list(nx.all_shortest_paths(G, v, int(t)))
            except nx.NetworkXNoPath:
                continue
            dist[q, v] = len(paths[0]) - 1
            sigma[q, v] = len(paths)
            if v != t:
                nxt[q, v] = min(p[1] for p in paths)
    return dist, nxt, sigma


# ---- counts ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("widths,n_plain,n_extra,top_row", [(K.ONE_LANE_WIDTHS, 330, 341, 8), (K.WHOLE_WAVE_WIDTHS, 546, 555, 64)])
def test_boundary_counts_are_two_to_the_53_and_one_more(widths, n_plain, n_extra, top_row):
    g = K.boundary_count_graph(widths, False)
    assert g["product"] == 2 ** 53 and g["n"] == n_plain and g["top"] == n_plain - 1
    lens = row_lengths(g["adj"])
    assert lens[g["top"]] == top_row and (top_row > K.SHORT_ROW) == (widths is K.WHOLE_WAVE_WIDTHS)
    if widths is K.ONE_LANE_WIDTHS:
        assert lens.max() == K.SHORT_ROW                                  # no row of this graph reaches the whole-wave path
    else:
        assert (lens[np.concatenate(g["layers"][2:])] == 64).all()        # layers 3 .. 9 and the top: the whole-wave path
    d, s, _, _ = T.mirror_toward(g["adj"], [0])
    assert s[0, g["top"]] == 2.0 ** 53 and d[0, g["top"]] == len(widths) + 1
    for j, lay in enumerate(g["layers"]):
        want = 1
        for w in widths[:j]:
            want *= w
        assert [int(x) for x in s[0, lay]] == [want] * len(lay) and (d[0, lay] == j + 1).all()
    for chain_first in (False, True):
        e = K.boundary_count_graph(widths, True, chain_first)
        assert e["n"] == n_extra
        row = e["adj"].indices[e["adj"].indptr[e["top"]]:e["adj"].indptr[e["top"] + 1]]
        assert len(row) == top_row + 1 and row[0 if chain_first else -1] == e["head"]
        with pytest.raises(T.CountRefused, match=rf"node {e['top']} has more than 2\^53 shortest paths to target 0"):
            T.mirror_toward(e["adj"], [0])
        d2, _ = M.mirror_trees(e["adj"], [0])
        assert d2[0, e["head"]] == len(widths) == d2[0, e["layers"][-1][0]] and d2[0, e["top"]] == len(widths) + 1


def test_far_above_the_limit():
    g = K.boundary_count_graph(K.FAR_ABOVE_WIDTHS, False)
    assert g["product"] == 2 ** 60 and g["n"] == 642 and g["top"] == 641 and row_lengths(g["adj"])[g["top"]] == 64
    with pytest.raises(T.CountRefused, match=r"2\^53"):
        T.mirror_toward(g["adj"], [0])


def test_lane_local_overcount_row():
    g = K.lane_local_overcount_graph()
    a = g["adj"]
    assert g["n"] == 620 and g["n"] % K.WAVE
    row = a.indices[a.indptr[g["apex"]]:a.indptr[g["apex"] + 1]]
    assert len(row) == 65 and row[0] == g["top"] and row[64] == g["head"] and row[1:64].tolist() == g["sinks"]
    assert g["apex"] % K.WAVE == 43                                      # the owner is not the lane that sees the overflow (lane 0)
    d, _ = M.mirror_trees(a, [0])
    assert d[0, g["top"]] == d[0, g["head"]] == 10 and d[0, g["apex"]] == 11 and (d[0, g["sinks"]] == 255).all()
    with pytest.raises(T.CountRefused, match=rf"node {g['apex']} has more than 2\^53"):
        T.mirror_toward(a, [0])
    # without the chain's entry the apex has exactly 2^53: the overflow is that one entry
    b = a.tolil()
    b[g["apex"], g["head"]] = 0
    _, s, _, _ = T.mirror_toward(b.tocsr(), [0])
    assert s[0, g["apex"]] == 2.0 ** 53


# ---- the tie rule ---------------------------------------------------------------------------------------------------------------------

def test_tie_cases_cover_the_lanes_and_lengths():
    assert [c[0] for c in K.TIE_CASES] == [32, 33, 64, 65, 128, 129, 200]
    lanes = [set(c[1]) for c in K.TIE_CASES]
    assert any(0 in s for s in lanes) and any(63 in s for s in lanes) and any(len(s) > 1 for s in lanes)
    assert any(c[2] for c in K.TIE_CASES)


@pytest.mark.parametrize("L,hub_lanes,last_wave", K.TIE_CASES)
def test_tie_rule_graph_has_its_closed_form(L, hub_lanes, last_wave):
    g = K.tie_rule_graph(L, hub_lanes, last_wave)
    a, n = g["adj"], g["n"]
    assert n % 4 and n % K.WAVE and n <= 700
    lens = row_lengths(a)
    assert [h % K.WAVE for h in g["hubs"]] == sorted(hub_lanes) and len({h // K.WAVE for h in g["hubs"]}) == 1
    assert ((n - 1) // K.WAVE == g["hubs"][0] // K.WAVE) == last_wave
    for h in g["hubs"]:
        assert lens[h] == L and np.array_equal(a.indices[a.indptr[h]:a.indptr[h + 1]], g["succ"])
    assert lens[g["succ"]].max() <= K.SHORT_ROW                           # the successors' own rows are read by one lane
    first = g["first"]
    taken = {p for p in first if p is not None}
    assert {p for p in (0, 31, 32, 63, 64, 65, L - 1) if p < L} <= taken
    assert first[63] == (63 if L >= 64 else L - 1)
    assert [q for q in range(64) if first[q] is None] == [K.TIE_DIRECT, *K.TIE_UNREACHED]
    for q, p in enumerate(first):
        if p is None:
            continue
        carriers = [i for i, u in enumerate(g["succ"]) if a[u, q] != 0]
        assert carriers[0] == p and len(carriers) >= (2 if p + 1 < L else 1)
    if L > 64:                                                            # a bit carried only from the second chunk on, one claimed again later
        assert any(p is not None and p >= 64 for p in first)
        assert any(p is not None and p < 64 and p + 64 < L for p in first)
    d, nx_ = M.mirror_trees(a, g["targets"])
    assert np.array_equal(d, g["dist"]) and np.array_equal(nx_, g["next"])
    for h in g["hubs"]:
        assert g["dist"][K.TIE_DIRECT, h] == 1 and (g["dist"][list(K.TIE_UNREACHED), h] == 255).all()
        rest = [q for q in range(64) if first[q] is not None]
        assert (g["dist"][rest, h] == 2).all() and g["next"][rest, h].tolist() == [int(g["succ"][first[q]]) for q in rest]
    if L <= 33:
        ed, en, es = enumerated(a, g["targets"])
        _, s, _, _ = T.mirror_toward(a, g["targets"])
        assert np.array_equal(ed, g["dist"]) and np.array_equal(en, g["next"]) and np.array_equal(es, s)


def test_tie_weight_graph_ties():
    g = K.tie_weight_graph()
    a = g["adj"]
    lens = row_lengths(a)
    assert {k: int(lens[h]) for k, h in g["hubs"].items()} == {33: 33, 64: 64, 65: 65}
    assert g["hubs"][64] // K.WAVE == g["hubs"][65] // K.WAVE and g["hubs"][33] % K.WAVE == 0 and g["n"] % 4
    d, _ = M.mirror_trees(a, g["targets"])
    for k, h in g["hubs"].items():
        row = a.indices[a.indptr[h]:a.indptr[h + 1]]
        assert (d[:, row] == 1).all() and (d[:, h] == 2).all()            # every successor is one hop closer
    assert (d[:, g["above"]] == 3).all()
    zero = K.tie_weight_tables(g, "zero")
    assert (zero == 0).all() and np.signbit(zero).any() and not np.signbit(zero).all()
    _, _, b, nb = T.mirror_toward(a, g["targets"], zero)
    assert not np.signbit(b).any()                                        # w + (+0.0): every best is +0.0, the smallest index wins
    assert all(nb[q, h] == g["layer"][0] for q in range(2) for h in g["hubs"].values())
    ints = K.tie_weight_tables(g, "int")
    _, _, b, nb = T.mirror_toward(a, g["targets"], ints)
    for q in range(2):
        for k, h in g["hubs"].items():
            row = g["layer"][:k]
            top = b[q, row].max()
            assert nb[q, h] == row[b[q, row] == top][0]
            assert (b[q, row] == top).sum() > 1 or top == 2.0             # ties everywhere but where a placed 2 alone decides
    lay, hubs = g["layer"], g["hubs"]
    assert nb[0, hubs[64]] == nb[0, hubs[65]] == lay[63] and b[0, lay[63]] == b[0, lay[64]]      # lane 63 against lane 0's second entry
    assert nb[1, hubs[65]] == lay[64] and nb[1, hubs[64]] < lay[63] and nb[0, hubs[33]] < lay[32]


# ---- between --------------------------------------------------------------------------------------------------------------------------

def test_between_graph_pairs():
    g = K.between_graph()
    n = g["n"]
    assert 256 < n < 512 and n % K.WAVE and n == 303
    src, tgt = g["sources"], g["targets"]
    pairs = [K.PAIR_MANY, K.PAIR_SINGLE, K.PAIR_SAME, K.PAIR_UNREACHABLE, K.PAIR_HALF, (1, 0)]
    r = T.mirror_between(g["adj"], src[:3], tgt[:5], pairs)
    length, paths, nodes = r["length"], r["n_paths"], r["n_nodes"]
    many = r["tables"][K.PAIR_MANY][0]
    assert length[0, 0] == 6 and paths[0, 0] > 1000 and many.min() < K.FILL_NODES <= many.max()
    assert (many < K.FILL_NODES).sum() > 64 and (many >= K.FILL_NODES).sum() >= 3      # both iterations, more than one wave in the first
    assert length[1, 1] == 5 and paths[1, 1] == 1 and r["tables"][K.PAIR_SINGLE][0].tolist() == g["chain"]
    assert length[2, 2] == 0 and paths[2, 2] == 1 and nodes[2, 2] == 1 and src[2] == tgt[2]
    same = r["tables"][K.PAIR_SAME]
    assert same[0].tolist() == [src[2]] and same[1].tolist() == [0] and same[2].tolist() == [0] and same[5].tolist() == [1.0]
    assert length[0, 3] == -1 and length[1, 0] == -1 and nodes[0, 3] == 0 and len(r["tables"][K.PAIR_UNREACHABLE][0]) == 0
    half = r["tables"][K.PAIR_HALF][0]
    assert length[2, 0] == 3 and half.min() == src[2] and half.max() == tgt[0]
    # Python's integers over the layers: the count of the many-route pair is exact
    count = {int(tgt[0]): 1}
    a = g["adj"]
    for lay in g["layers"][-2::-1]:
        for v in lay:
            count[int(v)] = sum(count.get(int(u), 0) for u in a.indices[a.indptr[v]:a.indptr[v + 1]])
    assert int(paths[0, 0]) == count[int(src[0])] < 2 ** 53
    # the full pass: some pairs unreachable, mediators present
    full = T.mirror_between(g["adj"], src, tgt)
    assert (full["length"] == -1).any() and (full["length"] > 0).sum() > 1000 and (full["mediators"][1] > 1).any()
    # the single-route and the small tables against networkx's enumeration
    G = digraph(a)
    for (i, j) in (K.PAIR_SINGLE, K.PAIR_HALF):
        ps = list(nx.all_shortest_paths(G, int(src[i]), int(tgt[j])))
        tab = r["tables"][(i, j)]
        assert len(ps) == paths[i, j] and sorted({v for p in ps for v in p}) == tab[0].tolist()
        assert tab[4].tolist() == [sum(1 for p in ps if v in p) for v in tab[0]]


# ---- the duplicate check --------------------------------------------------------------------------------------------------------------

def _repeats(rowptr, col):
    return [v for v in range(len(rowptr) - 1) if len(set(col[rowptr[v]:rowptr[v + 1]].tolist())) < rowptr[v + 1] - rowptr[v]]


def test_row_boundary_graph():
    rowptr, col = K.row_boundary_graph()
    n = len(rowptr) - 1
    lens = np.diff(rowptr)
    assert n == 20 and rowptr[0] == 0 and rowptr[-1] == len(col) and lens[0] == 0 and lens[-1] > 0
    assert _repeats(rowptr, col) == []
    full = [v for v in range(n) if lens[v]]
    equal = [(a, b) for a, b in zip(full, full[1:]) if col[rowptr[a + 1] - 1] == col[rowptr[b]]]
    assert any(b == a + 1 for a, b in equal) and any(b > a + 1 for a, b in equal) and len(equal) == 5
    for v in range(n):
        assert (np.diff(col[rowptr[v]:rowptr[v + 1]]) > 0).all()
    a = K.csr_of(rowptr, col)
    d, s, _, _ = T.mirror_toward(a, K.ROW_BOUNDARY_TARGETS)
    ed, en, es = enumerated(a, K.ROW_BOUNDARY_TARGETS)
    _, nx_ = M.mirror_trees(a, K.ROW_BOUNDARY_TARGETS)
    assert np.array_equal(d, ed) and np.array_equal(s, es) and np.array_equal(nx_, en) and s.max() > 1
    named = {"first": 2, "last": 19, "after_empty": 7, "two": 13}
    for variant, row in named.items():
        rp, c = K.row_boundary_graph(variant)
        rep = _repeats(rp, c)
        assert rep and max(rep) == row and (len(rep) == 2) == (variant == "two")
        for v in range(n):
            assert (np.diff(c[rp[v]:rp[v + 1]]) >= 0).all()               # still not descending: the handle accepts it
    first_full = full[0]
    assert named["first"] == first_full and named["last"] == n - 1 and lens[named["after_empty"] - 1] == 0
    rp, c = K.row_boundary_graph("after_empty")
    assert c[rp[7]] == c[rp[7] - 1] == c[rp[7] + 1]                       # the row's first entry equals the entry before it, too
