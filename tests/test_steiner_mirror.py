"""CPU: the mirror of the Steiner trees (tests/steiner_mirror.py) on every case of tests/steiner_cases.py against independent oracles --
scipy's BFS distances for (dist, src), scipy's minimum spanning tree of the terminals' metric closure for the length (Mehlhorn's
theorem), networkx for the forest properties, enumeration for the approximation bound on graphs of up to 12 nodes --, that every
ablation of the definition changes an asserted output somewhere, that both tie rules decide outcomes, the statistics and writers of
steiner.py, and that header, library and binding hold gss_steiner_trees.  Integers throughout: every comparison is an equality."""
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import steiner_cases as K  # noqa: E402
import steiner_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import set_modules, steiner, steiner_cli  # noqa: E402
from gcn_drug_repurposing_amd.proximity import ProximityError  # noqa: E402


def sampled(name):
    """the units of a case the oracles look at: all, but of "many" (one shape repeated) every 23rd"""
    c = K.case(name)
    return range(len(c.units)) if name != "many" else range(0, len(c.units), 23)


def matrix(c):
    import scipy.sparse as sp
    return sp.csr_matrix((np.ones(len(c.col), np.int8), c.col, c.rowptr), shape=(c.n, c.n))


def terminal_distances(c, terminals):
    """hop distances [T, n] from every terminal by scipy's BFS, inf where unreachable"""
    from scipy.sparse.csgraph import shortest_path
    if len(terminals) == 0:
        return np.zeros((0, c.n))
    return shortest_path(matrix(c), method="D", unweighted=True, indices=np.asarray(terminals))


def closure_forest_weight(d_tt):
    """(the weight of the minimum spanning forest of the terminals' metric closure, its trees)"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components, minimum_spanning_tree
    T = len(d_tt)
    if T == 0:
        return 0, 0
    w = np.where(np.isfinite(d_tt), d_tt, 0)
    g = sp.csr_matrix(w)
    return int(round(minimum_spanning_tree(g).sum())), int(connected_components(g, directed=False)[0])


@pytest.mark.parametrize("name", K.CASES)
def test_nearest_terminal_and_length_against_scipy(name):
    c = K.case(name)
    for u in sampled(name):
        t = M.tree(c.rowptr, c.col, c.units[u])
        d = terminal_distances(c, c.units[u])
        if len(c.units[u]) == 0:
            assert (t["dist"] == -1).all() and (t["src"] == -1).all()
        else:
            near = d.min(axis=0)
            reached = np.isfinite(near)
            assert np.array_equal(t["dist"] >= 0, reached), (name, u)
            assert np.array_equal(t["dist"][reached], near[reached].astype(np.int64)), (name, u)
            assert np.array_equal(t["src"][reached], np.argmax(d == near[None, :], axis=0)[reached]), (name, u)      # the first = the smallest position
            assert (t["src"][~reached] == -1).all()
        weight, comps = closure_forest_weight(d[:, c.units[u]] if len(c.units[u]) else np.zeros((0, 0)))
        assert (t["length"], t["n_comp"]) == (weight, comps), (name, u)                                               # Mehlhorn's theorem, per component


@pytest.mark.parametrize("name", K.CASES)
def test_the_edge_list_is_a_forest_over_the_terminals(name):
    import networkx as nx
    c = K.case(name)
    want = K.mirror(name)
    from scipy.sparse.csgraph import connected_components
    inside = set(zip(np.repeat(np.arange(c.n), np.diff(c.rowptr)).tolist(), c.col.tolist()))
    label = connected_components(matrix(c), directed=False)[1]
    for u in sampled(name):
        terminals = c.units[u].tolist()
        g = nx.Graph()
        g.add_nodes_from(terminals)
        for a, b, kind in want["edges"][u]:
            assert (a, b) in inside and not g.has_edge(a, b), (name, u, a, b)
            g.add_edge(a, b)
        assert g.number_of_nodes() == len(terminals) + want["n_steiner"][u] and set(g) == set(terminals) | set(want["steiner"][u].tolist())
        assert g.number_of_edges() == want["n_edges"][u] == len(terminals) + want["n_steiner"][u] - want["n_comp"][u], (name, u)
        assert nx.number_connected_components(g) == want["n_comp"][u] and (len(terminals) == 0 or nx.is_forest(g)), (name, u)
        for comp in nx.connected_components(g):                                      # a tree spans all terminals of its component of the graph
            ts = [t for t in terminals if t in comp]
            assert ts == [t for t in terminals if label[t] == label[ts[0]]], (name, u)
        assert all(g.degree(v) >= 2 for v in want["steiner"][u].tolist()), (name, u)  # every leaf is a terminal
        assert [tuple(x) for x in want["bridge"][u].tolist()] == sorted(tuple(x) for x in want["bridge"][u].tolist())
        assert np.array_equal(want["steiner"][u], np.sort(want["steiner"][u])) and want["max_w"][u] <= max(want["length"][u], 0)


def optimum(c, terminals):
    """the fewest edges of a tree that spans `terminals` (one component), and that tree's fewest leaves, by enumeration of the Steiner
    node subsets: a subset works when terminals + subset induce a connected subgraph"""
    import networkx as nx
    g = nx.Graph()
    g.add_nodes_from(range(c.n))
    g.add_edges_from(zip(np.repeat(np.arange(c.n), np.diff(c.rowptr)).tolist(), c.col.tolist()))
    others = [v for v in range(c.n) if v not in terminals]
    for k in range(len(others) + 1):
        leaves = []
        for extra in itertools.combinations(others, k):
            sub = g.subgraph(list(terminals) + list(extra))
            if nx.is_connected(sub):
                tree = nx.minimum_spanning_tree(sub)
                leaves.append(sum(1 for v in tree if tree.degree(v) == 1))
        if leaves:
            return len(terminals) + k - 1, min(leaves)
    return None


def test_the_approximation_bound_by_enumeration():
    checked = 0
    for graph_seed in range(4):
        n, (rowptr, col) = 11 + graph_seed % 2, K.csr(11 + graph_seed % 2, K.gnp(11 + graph_seed % 2, 0.24, 40 + graph_seed))
        c = K.Case("tiny", n, rowptr, col, K.draw_units(n, 6, 5, graph_seed, lo=2), 0, "")
        for unit in c.units:
            t = M.tree(rowptr, col, unit)
            if t["n_comp"] != 1:
                continue
            best, leaves = optimum(c, unit.tolist())
            assert best <= t["n_edges"] <= t["length"], (graph_seed, unit)
            # the bound holds for every optimal tree: the fewest leaves among those enumerated asserts the strictest of them
            assert t["length"] * leaves <= 2 * (leaves - 1) * best, (graph_seed, unit, t["length"], best, leaves)
            checked += 1
    c = K.case("n12")
    for u, unit in enumerate(c.units):
        if K.mirror("n12")["n_comp"][u] == 1:
            best, leaves = optimum(c, unit.tolist())
            assert K.mirror("n12")["length"][u] * leaves <= 2 * (leaves - 1) * best, u
            checked += 1
    assert checked >= 12


def asserted(t, u):
    """what the tests assert of unit u of a table, as one comparable value"""
    return (tuple(int(t[f][u]) for f in M.COUNTS), t["steiner"][u].tolist(), t["parent"][u].tolist(), t["bridge"][u].tolist())


def test_every_ablation_changes_an_asserted_output():
    where = {}
    for ablation in M.ABLATIONS:
        for name in K.SMALL:
            right, wrong = K.mirror(name), K.mirror(name, ablation)
            hits = [u for u in range(len(K.case(name).units)) if asserted(right, u) != asserted(wrong, u)]
            if hits:
                where.setdefault(ablation, []).append((name, hits[0]))
    assert sorted(where) == sorted(M.ABLATIONS), where
    assert any(name == "lattice" for name, _ in where["src_larger"]) and any(name == "mixed" for name, _ in where["order_wvu"])


def test_the_src_rule_and_the_bridge_order_both_decide():
    lattice = K.mirror("lattice")
    assert (lattice["src_decided"] > 0).all() and (lattice["order_decided"] > 0).all()
    mixed = K.mirror("mixed")
    assert (mixed["src_decided"] > 0).any() and (mixed["order_decided"] > 0).any()
    for name in ("n300", "many"):                                                    # and on the random graphs both kinds occur
        assert (K.mirror(name)["src_decided"] > 0).any() and (K.mirror(name)["order_decided"] > 0).any(), name


def test_every_case_has_the_property_it_was_built_for():
    for name in K.CASES:                                                             # the table's contract: strictly ascending nodes
        assert all((np.diff(u) > 0).all() and (len(u) == 0 or 0 <= u[0] and u[-1] < K.case(name).n) for u in K.case(name).units), name
    parts = K.mirror("parts")
    assert parts["n_comp"].tolist() == [0, 1, 1, 1, 4, 1, 1] and parts["length"].tolist() == [0, 0, 1, 5, 4 + 5 + 2, 0, 6]
    assert parts["n_steiner"].tolist() == [0, 0, 0, 3, 3 + 4 + 1, 0, 1] and parts["max_w"].tolist() == [0, 0, 1, 3, 5, 0, 2]
    assert parts["bridge"][2].tolist() == [[0, 1]] and parts["steiner"][3].tolist() == [1, 3, 4] and parts["steiner"][6].tolist() == [16]
    assert (M.tree(K.case("parts").rowptr, K.case("parts").col, K.case("parts").units[4])["dist"][22:] == -1).all()
    capped, n300 = K.mirror("capped"), K.mirror("n300")
    assert (capped["n_steiner"] > K.case("capped").max_add).all() and np.array_equal(capped["n_steiner"], n300["n_steiner"])
    k65 = K.mirror("k65")
    assert k65["length"].tolist() == [2, 64, 0, 1] and (k65["n_steiner"] == 0).all() and k65["bridge"][1].tolist() == [[0, v] for v in range(1, 65)]
    star = K.case("star")
    got = K.mirror("star")
    assert np.diff(star.rowptr)[K.HUB] == K.HUB_DEG > K.THREADS and K.HUB in star.units[0] and K.HUB in star.units[3]
    assert got["steiner"][1].tolist() == [K.HUB] and got["length"][1] == 2
    assert K.HUB in got["bridge"][2].ravel() and K.HUB in got["steiner"][2] and got["bridge"][3].tolist() == [[K.HUB, 5]]
    for name, T in (("t63", 63), ("t64", 64), ("t65", 65), ("t1023", 1023), ("t1024", 1024), ("t1025", 1025), ("t4096", 4096)):
        c = K.case(name)
        assert len(c.units[0]) == T and 4 * c.n + 16 * T <= K.LDS_BUDGET and K.mirror(name)["n_steiner"][0] > 0
        assert np.diff(c.rowptr).max() > 8 and K.mirror(name)["n_comp"][0] >= 1
    assert K.MAX_SEEDS == steiner.MAX_SEEDS == 4096
    ring = K.mirror("ring")
    assert K.case("ring").n == K.MAX_NODES == steiner.MAX_NODES and ring["length"].tolist() == [6, K.MAX_NODES // 2, 2, 0]
    assert ring["n_steiner"].tolist() == [3, K.MAX_NODES // 2 - 1, 1, 0] and ring["steiner"][2].tolist() == [K.MAX_NODES - 1]
    assert ring["max_w"][1] == K.MAX_NODES // 2 > 2 * 64 * 64                          # 7,680 levels: far past two wave-strides
    far = K.mirror("open")
    assert far["max_w"][0] == far["length"][0] == K.FAR > 1 << 14 and far["n_steiner"][0] == K.FAR - 1
    assert len(K.case("many").units) == 1030 > K.MAX_BLOCKS and K.LDS_BUDGET == steiner.LDS_BUDGET
    assert 4 * 13329 + 16 * 4096 <= K.LDS_BUDGET < 4 * K.MAX_NODES + 16 * K.MAX_SEEDS     # the reference network fits with the largest table
    text = open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "steiner.hip")).read()
    assert int(re.search(r"constexpr int kLane = (\d+);", text).group(1)) == K.LANE_ROW < np.diff(K.case("k65").rowptr).max()
    assert int(re.search(r"constexpr int kThreads = (\d+);", text).group(1)) == K.THREADS


def test_header_library_and_binding_hold_the_export():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    header = open(os.path.join(ROOT, "include", "gssgcn.h")).read()
    assert re.search(r"^int gss_steiner_trees\(", header, flags=re.M)
    assert int(re.search(r"#define GSS_ABI_VERSION (\d+)", header).group(1)) == pkg._lib.ABI_VERSION == 25      # additive: the number stays
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T gss_steiner_trees$", out, flags=re.M)
    res, args = pkg._lib.SIGNATURES["gss_steiner_trees"]
    assert len(args) == 18 and pkg._lib.load().gss_steiner_trees.argtypes == args
    assert "steiner.hip" in open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "Makefile")).read()
    assert "steiner.hip" in pkg._lib.source_hashes()


# ---- the host side of steiner.py ----------------------------------------------------------------------------------------------------------

def test_table_stats_on_hand_made_integers():
    n = np.array([4, 3, 1, 2])
    sizes = np.array([[4, 4, 4, 3, 4], [3, 3, 3, 3, 3], [1, 1, 1, 1, 1], [2, 2, 2, 2, 2]])
    st = np.array([[1, 3, 2, 1, 2], [2, 2, 2, 2, 2], [0, 0, 0, 0, 0], [5, 1, 2, 3, 4]])
    ln = np.array([[4, 6, 5, 6, 7], [4, 4, 4, 4, 4], [0, 0, 0, 0, 0], [6, 2, 3, 4, 5]])
    s = steiner.table_stats(n, sizes, st, ln)
    a, b = s["steiner_stats"], s["length_stats"]
    assert a["mean"][0] == 2.0 and a["sd"][0] == np.sqrt(0.5) and a["z"][0] == -1.0 / np.sqrt(0.5) and a["p"][0] == 0.4       # 1 of 4 random sets needs as few
    assert b["mean"][0] == 6.0 and b["p"][0] == 0.2 and b["z"][0] < 0                                                       # none is as short
    assert a["mean"][1] == 2.0 and np.isnan(a["z"][1]) and a["p"][1] == 1.0                                                 # sd = 0
    assert np.isnan([a[f][2] for f in set_modules.STAT_FIELDS]).all() and not np.isnan(a["q"][[0, 1, 3]]).any()             # one gene: no part in q
    assert a["p"][3] == 1.0 and a["z"][3] > 0 and b["p"][3] == 1.0                                                          # more than every random set: the lower tail holds them all
    assert s["short"].tolist() == [1, 0, 0, 0]
    upper = set_modules.null_stats(st[:, 0], st[:, 1:], n < 2)
    assert np.array_equal(upper["mean"], a["mean"], equal_nan=True) and np.array_equal(upper["z"], a["z"], equal_nan=True) and upper["p"][3] == 0.2
    with pytest.raises(ValueError, match="the null holds no sample"):
        steiner.table_stats(n, sizes[:, :1], st[:, :1], ln[:, :1])


def test_refusals_need_no_device():
    eng = steiner.SteinerEngine.__new__(steiner.SteinerEngine)
    eng.net = type("Net", (), {"n": 100})()
    eng._rowptr = eng._col = eng._torch = None                                          # what close() leaves; __del__ closes again
    with pytest.raises(ProximityError, match="the engine is closed"):
        eng.check(5)
    with pytest.raises(ProximityError, match="the engine is closed"):
        eng.trees([np.array([1, 2], np.int32)])
    eng._rowptr = object()
    for args, words in (((5, -1), "max_add=-1 must be >= 0"), ((4097, 5), "a set has 4097 seeds; at most 4096")):
        with pytest.raises(ProximityError, match=words):
            eng.check(*args)
    eng.check(4096, 4096)
    eng.net.n = 13329
    eng.check(4096)
    eng.net.n = steiner.MAX_NODES
    eng.check(2528)
    with pytest.raises(ProximityError, match="needs 163344 bytes of LDS; 4 n \\+ 16 max_size may be 163328"):
        eng.check(2529)
    eng.net.n = steiner.MAX_NODES + 1
    with pytest.raises(ProximityError, match="a network of 30721 nodes; between 1 and 30720"):
        eng.check(5)
    for kw, words in ((dict(n_random=1), "n_random=1: need at least 2"), (dict(min_bin_size=0), "min_bin_size=0 must be >= 1"),
                      (dict(side=2), "side=2 must be 0"), (dict(gene_sets=[]), "gene_sets must not be empty")):
        with pytest.raises(ProximityError, match=words):
            eng.tree_table(**{"gene_sets": [["a"]], "side": 1, **kw})
    eng._rowptr = None


def test_writers_and_arguments(tmp_path, capsys):
    trees = {"n_comp": np.array([1, 2]), "length": np.array([4, 0]), "n_steiner": np.array([2, 0]), "n_edges": np.array([4, 0]), "max_w": np.array([3, 0]),
             "terminals": [np.array([0, 3, 5]), np.array([1, 4])], "steiner": [np.array([2, 4]), np.zeros(0, np.int64)],
             "parent": [np.array([0, 5]), np.zeros(0, np.int64)], "bridge": [np.array([[2, 3], [2, 4]]), np.zeros((0, 2), np.int64)]}
    trees["edges"] = [steiner.tree_edges(s, p, b) for s, p, b in zip(trees["steiner"], trees["parent"], trees["bridge"])]
    genes = ["g0", "g1", "g2", "g3", "g4", "g5"]
    steiner_cli.write_edges(tmp_path / "e.tsv", ["a", "b c"], genes, trees)
    assert (tmp_path / "e.tsv").read_text() == "set\ta\tb\tkind\na\tg2\tg0\tpath\na\tg4\tg5\tpath\na\tg2\tg3\tbridge\na\tg2\tg4\tbridge\n"
    steiner_cli.write_nodes(tmp_path / "n.tsv", ["a", "b c"], genes, trees)
    assert (tmp_path / "n.tsv").read_text() == ("set\tgene\trole\tparent\tdegree\na\tg0\tseed\tNA\t1\na\tg3\tseed\tNA\t1\na\tg5\tseed\tNA\t1\n"
                                                "a\tg2\tsteiner\tg0\t3\na\tg4\tsteiner\tg5\t2\nb c\tg1\tseed\tNA\t0\nb c\tg4\tseed\tNA\t0\n")
    steiner_cli.write_genes(tmp_path / "g.tsv", ["a", "b c"], genes, trees)
    assert (tmp_path / "g.tsv").read_text() == "\ta\tg0\tg3\tg5\tg2\tg4\n\tb c\tg1\tg4\n"
    from gcn_drug_repurposing_amd.proximity import load_disease_genes
    assert load_disease_genes(tmp_path / "g.tsv") == {"a": {"g0", "g2", "g3", "g4", "g5"}, "b.c": {"g1", "g4"}}       # what disease_modules.py reads
    res = {"n": np.array([3, 2]), "trees": trees}
    steiner_cli.write_summary(tmp_path / "s0.tsv", ["a", "b c"], res)
    lines = (tmp_path / "s0.tsv").read_text().split("\n")
    assert lines[0].split("\t") == steiner_cli.SUMMARY_HEADER and len(steiner_cli.SUMMARY_HEADER) == 19
    assert lines[1].split("\t") == ["a", "3", "1", "2", "4", "4", "3", "2"] + ["NA"] * 11 and lines[2].split("\t")[:8] == ["b c", "2", "2", "0", "0", "0", "0", "0"]
    stats = steiner.table_stats(res["n"], [[3, 3, 3], [2, 2, 2]], [[2, 4, 3], [0, 1, 1]], [[4, 6, 8], [0, 2, 2]])
    steiner_cli.write_summary(tmp_path / "s.tsv", ["a", "b c"], dict(res, **stats))
    row = (tmp_path / "s.tsv").read_text().split("\n")[1].split("\t")
    assert row[8:13] == [repr(float(stats["steiner_stats"][f][0])) for f in set_modules.STAT_FIELDS] and float(row[8]) == 3.5 and row[-1] == "0"
    assert row[13:18] == [repr(float(stats["length_stats"][f][0])) for f in set_modules.STAT_FIELDS] and float(row[16]) == 1 / 3
    base = ["--network", "n.sif"]
    for args, words in ((base, "one of the arguments --diseases --drugs --seeds is required"),
                        (base + ["--seeds", "s", "--drugs", "t"], "not allowed with argument"),
                        (base + ["--seeds", "s", "--max-add", "0"], "--max-add 0 must be >= 1"),
                        (base + ["--seeds", "s", "--n-random", "1"], "--n-random 1: need at least 2"),
                        (base + ["--seeds", "s", "--min-bin-size", "0"], "--min-bin-size 0 must be >= 1"),
                        (base + ["--seeds", "s", "--n-random", "0", "--null", "x"], "--null needs --n-random >= 2")):
        with pytest.raises(SystemExit) as e:
            steiner_cli.parse_args(args)
        assert e.value.code == 2 and words in capsys.readouterr().err, args
    a = steiner_cli.parse_args(base + ["--diseases", "d.tsv", "--set", "x"])
    assert (a.max_add, a.n_random, a.seed, a.min_bin_size, a.out, a.nodes, a.summary, a.genes, a.null, a.set) == (
        4096, 1000, 452456, 100, "edges.tsv", None, None, None, None, ["x"])
    assert steiner_cli.parse_args(base + ["--seeds", "s", "--n-random", "0"]).n_random == 0
