"""CPU: the mirror of the seed connector growth (tests/connectors_mirror.py) against a brute-force oracle at every step of every case of
tests/connectors_cases.py -- scipy's connected_components on the subgraph induced by M and v, for EVERY node v outside M (a node without
a neighbour in M has LCC = L and cannot win, so this asks more than scanning the candidates) --, against networkx on the final module,
that every case has the property it was built for (the tie rule among them), the statistics and writers of connectors.py, and that
header, library and binding hold gss_seed_connectors.  Integers throughout: every comparison is an equality."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import connectors_cases as K  # noqa: E402
import connectors_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import connectors, connectors_cli, set_modules  # noqa: E402
from gcn_drug_repurposing_amd.proximity import ProximityError  # noqa: E402


def brute_force_lcc(rowptr, col, members):
    """-> (nodes outside M, the LCC size of the subgraph induced by M + {v} for each of them): one connected_components call on the
    disjoint union of those subgraphs, copy b holding M at b * (k + 1) .. + k and v at b * (k + 1) + k"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n, k = len(rowptr) - 1, len(members)
    src = np.repeat(np.arange(n), np.diff(rowptr))
    pos = np.full(n, -1, np.int64)
    pos[members] = np.arange(k)
    outside = np.flatnonzero(pos < 0)
    copy = np.full(n, -1, np.int64)
    copy[outside] = np.arange(len(outside))
    inner = (pos[src] >= 0) & (pos[col] >= 0)                                   # edges inside M, repeated in every copy
    a = (np.arange(len(outside))[:, None] * (k + 1) + pos[src[inner]][None, :]).ravel()
    b = (np.arange(len(outside))[:, None] * (k + 1) + pos[col[inner]][None, :]).ravel()
    cross = (pos[src] < 0) & (pos[col] >= 0)                                    # v -- a member, in v's copy only
    a = np.concatenate([a, copy[src[cross]] * (k + 1) + k])
    b = np.concatenate([b, copy[src[cross]] * (k + 1) + pos[col[cross]]])
    total = len(outside) * (k + 1)
    g = sp.csr_matrix((np.ones(len(a), np.int8), (a, b)), shape=(total, total))
    label = connected_components(g, directed=False)[1]
    count = np.bincount(label, minlength=1)
    return outside, count[label].reshape(len(outside), k + 1).max(axis=1)


def lcc_of(rowptr, col, members):
    """the LCC size of the subgraph M induces, by scipy"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    if len(members) == 0:
        return 0
    n = len(rowptr) - 1
    g = sp.csr_matrix((np.ones(len(col), np.int8), col, rowptr), shape=(n, n))[members][:, members]
    return int(np.bincount(connected_components(g, directed=False)[1]).max())


@pytest.mark.parametrize("name", K.CASES)
def test_every_choice_is_the_brute_force_minimum_over_all_nodes(name):
    c = K.case(name)
    want = K.mirror(name)
    degree = np.diff(c.rowptr)
    units = range(len(c.units)) if name != "many" else range(0, len(c.units), 23)    # "many" repeats one shape: every 23rd unit
    for u in units:
        seen = []
        got = M.grow(c.rowptr, c.col, c.units[u], c.n_add, on_step=lambda members, L: seen.append((members, L)))
        steps = int(want["steps"][u])
        assert got["steps"] == steps and len(seen) == min(steps + 1, c.n_add), (name, u)
        for t, (members, L) in enumerate(seen):
            assert np.array_equal(members, want["members"][u][:len(c.units[u]) + t])
            outside, lcc = brute_force_lcc(c.rowptr, c.col, members)
            assert L == lcc_of(c.rowptr, c.col, members), (name, u, t)
            best = np.lexsort((outside, degree[outside], -lcc))[0] if len(outside) else None
            if t < steps:
                assert best is not None and lcc[best] >= L + 2, (name, u, t)
                assert (outside[best], lcc[best], degree[outside[best]]) == (want["node"][u, t], want["lcc"][u, t], want["deg"][u, t]), (name, u, t)
            else:                                                                   # the mirror stopped here, and not because n_add ran out
                assert best is None or lcc[best] < L + 2, (name, u, t, L)
        if steps == c.n_add:                                                        # n_add ended it: the stop rule is not owed
            assert len(seen) == c.n_add
        assert (want["node"][u, steps:] == -1).all() and all((want[f][u, steps:] == 0).all() for f in ("lcc", "merged", "deg"))


@pytest.mark.parametrize("name", K.CASES)
def test_the_final_module_against_networkx(name):
    import networkx as nx
    c = K.case(name)
    want = K.mirror(name)
    g = nx.Graph()
    g.add_nodes_from(range(c.n))
    g.add_edges_from(zip(np.repeat(np.arange(c.n), np.diff(c.rowptr)).tolist(), c.col.tolist()))
    for u in (range(len(c.units)) if name != "many" else range(0, len(c.units), 23)):
        members = want["members"][u].tolist()
        m = len(c.units[u])
        where = {v: i for i, v in enumerate(members)}
        comps = [sorted(where[v] for v in comp) for comp in nx.connected_components(g.subgraph(members))]
        label = np.full(len(members), -1, np.int64)
        for comp in comps:
            label[comp] = comp[0]
        assert np.array_equal(label, want["label"][u]), (name, u)
        first = [sorted(where[v] for v in comp) for comp in nx.connected_components(g.subgraph(members[:m]))]
        assert want["first_lcc"][u] == max([len(x) for x in first], default=0)
        assert want["final_lcc"][u] == max([len(x) for x in comps], default=0)
        top = min((x for x in comps if len(x) == want["final_lcc"][u]), key=lambda x: x[0], default=[])
        assert (want["seeds_in"][u], want["added_in"][u]) == (sum(i < m for i in top), sum(i >= m for i in top)), (name, u)
        for t in range(int(want["steps"][u])):                                       # the components the connector of step t joined
            before = list(nx.connected_components(g.subgraph(members[:m + t])))
            assert want["merged"][u, t] == sum(1 for comp in before if any(v in comp for v in g[members[m + t]])), (name, u, t)


def test_every_case_has_the_property_it_was_built_for():
    n40, n300 = K.mirror("n40"), K.mirror("n300")
    assert K.case("n40").n % 64 != 0 and n40["steps"].max() < K.case("n40").n_add and (n40["node"][:, -1] == -1).all()
    assert n300["steps"].min() >= 1 and n300["steps"].max() >= 6
    capped = K.mirror("capped")
    assert (capped["steps"] == 2).sum() >= 4 and (n300["steps"][capped["steps"] == 2] > 2).any()       # n_add cut growth that would go on
    assert np.array_equal(capped["node"][:, :2], np.where(np.arange(2)[None, :] < capped["steps"][:, None], n300["node"][:, :2], -1))
    once = K.mirror("once")
    assert once["node"][0, 0] == 5 and once["lcc"][0, 0] == 6 and once["merged"][0, 0] == 2 and once["first_lcc"][0] == 4
    stars = K.mirror("stars")
    assert stars["node"][:, 0].tolist() == [0, 71, 81] and stars["merged"][:, 0].tolist() == [70, K.K_ROOTS + 1, K.K_ROOTS]
    assert stars["lcc"][:, 0].tolist() == [71, K.K_ROOTS + 2, K.K_ROOTS + 1] and (stars["steps"] == 1).all()
    over = K.mirror("overtake")
    assert over["first_lcc"][0] == 5 and over["node"][0].tolist() == [14, -1, -1, -1, -1] and over["final_lcc"][0] == 9
    assert over["seeds_in"][0] == 8 and over["added_in"][0] == 1 and over["label"][0][:5].tolist() == [0] * 5       # the first LCC is left outside
    star = K.case("star")
    assert np.diff(star.rowptr)[K.HUB] == K.HUB_DEG > K.THREADS and K.HUB in star.units[0] and K.HUB not in star.units[1]
    assert K.mirror("star")["node"][1, 0] == K.HUB and K.mirror("star")["merged"][1, 0] == 30 and K.mirror("star")["steps"][0] >= 1
    odd = K.mirror("odd")
    assert odd["node"][0, 0] == 2 and odd["steps"].tolist() == [1, 0, 1, 0, 0, 0, 0] and np.diff(K.case("odd").rowptr)[26] == 0
    assert odd["final_lcc"].tolist() == [3, 1, 3, 1, 0, 6, 10] and odd["seeds_in"].tolist() == [2, 1, 2, 1, 0, 6, 10]
    seen = []
    M.grow(K.case("odd").rowptr, K.case("odd").col, K.case("odd").units[6], 10, on_step=lambda members, L: seen.append(L))
    assert seen == [10]                                                                  # candidates exist; the best gain is 1
    ring = K.mirror("ring")
    assert K.case("ring").n == K.MAX_NODES == connectors.MAX_NODES and ring["node"][0].tolist() == [1, 3, 5, -1, -1]
    assert ring["lcc"][0].tolist() == [3, 5, 7, 0, 0] and ring["steps"].tolist() == [3, 0, 1, 0] and ring["node"][2, 0] == 0
    assert len(K.case("many").units) > K.MAX_BLOCKS
    assert (connectors.MAX_SEEDS, connectors.MAX_MEMBERS) == (K.MAX_SEEDS, K.MAX_MEMBERS)
    text = open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "seed_connect.hip")).read()
    assert int(re.search(r"constexpr int kRoots = (\d+);", text).group(1)) == K.K_ROOTS
    assert int(re.search(r"constexpr int kThreads = (\d+);", text).group(1)) == K.THREADS


def test_the_degree_and_the_node_index_both_decide_ties():
    ties = K.mirror("ties")
    assert ties["node"][:, 0].tolist() == [5, 7, 5]
    assert (ties["ties_lcc"][0, 0], ties["ties_deg"][0, 0]) == (2, 1)                    # 4 and 5 tie on L'; 5 has the smaller degree
    assert (ties["ties_lcc"][1, 0], ties["ties_deg"][1, 0]) == (2, 2)                    # 7 and 8 tie on (L', deg); 7 is the smaller node
    assert (ties["ties_lcc"][2, 0], ties["ties_deg"][2, 0]) == (4, 3)
    for name in ("n300", "many"):                                                        # and on the random graphs both kinds occur
        r = K.mirror(name)
        live = r["node"] >= 0
        assert (live & (r["ties_lcc"] > r["ties_deg"]) & (r["ties_deg"] == 1)).any() and (live & (r["ties_deg"] > 1)).any(), name
    # a wrong rule changes the result: the larger degree, or the larger node, picks another node on "ties"
    c = K.case("ties")
    degree = np.diff(c.rowptr)
    assert degree[4] > degree[5] and degree[7] == degree[8]


def test_header_library_and_binding_hold_the_export():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    header = open(os.path.join(ROOT, "include", "gssgcn.h")).read()
    assert re.search(r"^int gss_seed_connectors\(", header, flags=re.M)
    assert int(re.search(r"#define GSS_ABI_VERSION (\d+)", header).group(1)) == pkg._lib.ABI_VERSION == 25      # additive: the number stays
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T gss_seed_connectors$", out, flags=re.M)
    res, args = pkg._lib.SIGNATURES["gss_seed_connectors"]
    assert len(args) == 20 and pkg._lib.load().gss_seed_connectors.argtypes == args
    assert "seed_connect.hip" in open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "Makefile")).read()
    assert "seed_connect.hip" in pkg._lib.source_hashes() and "lds_union_find.h" in pkg._lib.source_hashes()


# ---- the host side of connectors.py ----------------------------------------------------------------------------------------------------

def test_table_stats_on_hand_made_integers():
    n = np.array([4, 3, 1, 2])
    sizes = np.array([[4, 4, 4, 3, 4], [3, 3, 3, 3, 3], [1, 1, 1, 1, 1], [2, 2, 2, 2, 2]])
    steps = np.array([[2, 0, 1, 0, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1]])
    final = np.array([[6, 1, 3, 1, 3], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [3, 3, 3, 3, 3]])
    joined = np.array([[4, 1, 2, 1, 2], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [2, 2, 2, 2, 2]])
    s = connectors.table_stats(n, sizes, steps, final, joined)
    empty = np.array([False, False, True, False])
    for key, obs in (("joined_stats", joined), ("lcc_stats", final)):
        want = set_modules.null_stats(obs[:, 0], obs[:, 1:], empty)
        for f in set_modules.STAT_FIELDS:
            assert np.array_equal(s[key][f], want[f], equal_nan=True), (key, f)
    j = s["joined_stats"]
    assert j["mean"][0] == 1.5 and j["sd"][0] == 0.5 and j["z"][0] == 5.0 and j["p"][0] == 0.2 and np.isnan(j["z"][1]) and j["p"][1] == 1.0
    assert np.isnan([j[f][2] for f in set_modules.STAT_FIELDS]).all() and not np.isnan(j["q"][[0, 1, 3]]).any()    # one gene: no statistics, no part in q
    fr = s["fraction_stats"]
    assert fr["mean"][0] == (0.25 + 0.5 + 1 / 3 + 0.5) / 4 and fr["p"][0] == 0.2 and fr["mean"][3] == 1.0           # the short sample counts by its own size
    assert s["connectors"].tolist() == [2, 0, 0, 1] and s["connectors_null_mean"][0] == 0.5 and s["connectors_null_sd"][0] == 0.5
    assert np.isnan(s["connectors_null_mean"][2]) and s["short"].tolist() == [1, 0, 0, 0]
    with pytest.raises(ValueError, match="the null holds no sample"):
        connectors.table_stats(n, sizes[:, :1], steps[:, :1], final[:, :1], joined[:, :1])
    whole = set_modules.null_stats([3, 9], [[1, 2, 3, 4], [5, 6, 7, 8]])                                             # integers are untouched by `real`
    assert whole["p"].tolist() == [0.6, 0.2] and set_modules.null_stats([2.5], [[1.5, 2.5, 3.5, 0.5]], real=True)["p"][0] == 0.6


def test_refusals_need_no_device():
    eng = connectors.ConnectorEngine.__new__(connectors.ConnectorEngine)
    eng.net = type("Net", (), {"n": 100})()
    eng._rowptr = eng._col = eng._torch = None                                          # what close() leaves; __del__ closes again
    with pytest.raises(ProximityError, match="the engine is closed"):
        eng.check(5, 5)
    with pytest.raises(ProximityError, match="the engine is closed"):
        eng.grow([np.array([1, 2], np.int32)])
    eng._rowptr = object()
    for args, words in (((5, 0), "n_add=0 must be >= 1"), ((4097, 5), "a set has 4097 seeds; at most 4096"),
                        ((4096, 4097), "4096 seeds \\+ n_add=4097 is over 8192 members")):
        with pytest.raises(ProximityError, match=words):
            eng.check(*args)
    eng.check(4096, 4096)
    eng.net.n = connectors.MAX_NODES + 1
    with pytest.raises(ProximityError, match="a network of 30721 nodes; between 1 and 30720"):
        eng.check(5, 5)
    for kw, words in ((dict(n_random=1), "n_random=1: need at least 2"), (dict(min_bin_size=0), "min_bin_size=0 must be >= 1"),
                      (dict(side=2), "side=2 must be 0"), (dict(gene_sets=[]), "gene_sets must not be empty")):
        with pytest.raises(ProximityError, match=words):
            eng.connector_table(**{"gene_sets": [["a"]], "side": 1, **kw})
    eng._rowptr = None


def test_writers_and_arguments(tmp_path, capsys):
    grown = {"node": np.array([[2, 0, -1], [-1, -1, -1]]), "lcc": np.array([[3, 6, 0], [0, 0, 0]]), "merged": np.array([[2, 3, 0], [0, 0, 0]]),
             "deg": np.array([[5, 7, 0], [0, 0, 0]]), "steps": np.array([2, 0]), "first_lcc": np.array([1, 2]), "final_lcc": np.array([6, 2]),
             "seeds_in": np.array([3, 2]), "added_in": np.array([2, 0]), "members": [np.array([1, 3, 4, 5, 2, 0]), np.array([3, 4])],
             "label": [np.array([0, 0, 2, 0, 0, 0]), np.array([0, 0])]}
    genes = ["g0", "g1", "g2", "g3", "g4", "g5"]
    connectors_cli.write_modules(tmp_path / "m.tsv", ["a", "b c"], genes, grown)
    assert (tmp_path / "m.tsv").read_text() == "set\trank\tgene\tlcc\tmerged\tdegree\na\t1\tg2\t3\t2\t5\na\t2\tg0\t6\t3\t7\n"
    connectors_cli.write_connectors(tmp_path / "c.tsv", ["a", "b c"], genes, grown)
    assert (tmp_path / "c.tsv").read_text() == ("set\tstep\tgene\tdegree\tlcc.before\tlcc.after\tgain\tmerged\tin.final.lcc\n"
                                                "a\t1\tg2\t5\t1\t3\t2\t2\t1\na\t2\tg0\t7\t3\t6\t3\t3\t1\n")
    connectors_cli.write_genes(tmp_path / "g.tsv", ["a", "b c"], genes, grown)
    assert (tmp_path / "g.tsv").read_text() == "\ta\tg1\tg3\tg4\tg5\tg2\tg0\n\tb c\tg3\tg4\n"
    from gcn_drug_repurposing_amd.proximity import load_disease_genes
    assert load_disease_genes(tmp_path / "g.tsv") == {"a": {"g0", "g1", "g2", "g3", "g4", "g5"}, "b.c": {"g3", "g4"}}   # what disease_modules.py reads
    res = {"n": np.array([4, 2]), "grow": grown}
    connectors_cli.write_summary(tmp_path / "s0.tsv", ["a", "b c"], res)
    lines = (tmp_path / "s0.tsv").read_text().split("\n")
    assert lines[0].split("\t") == connectors_cli.SUMMARY_HEADER and len(connectors_cli.SUMMARY_HEADER) == 24
    assert lines[1].split("\t") == ["a", "4", "1", "6", "3", "2"] + ["NA"] * 18 and lines[2].split("\t")[:6] == ["b c", "2", "2", "2", "2", "0"]
    stats = connectors.table_stats(res["n"], [[4, 4, 4], [2, 2, 2]], [[2, 0, 1], [0, 1, 1]], [[6, 1, 3], [2, 3, 3]], [[3, 1, 2], [2, 2, 2]])
    connectors_cli.write_summary(tmp_path / "s.tsv", ["a", "b c"], dict(res, **stats))
    row = (tmp_path / "s.tsv").read_text().split("\n")[1].split("\t")
    assert row[:8] == ["a", "4", "1", "6", "3", "2", "0.5", "0.5"] and row[8:13] == [repr(float(stats["joined_stats"][f][0])) for f in set_modules.STAT_FIELDS]
    assert row[-1] == "0" and float(row[10]) == 3.0
    base = ["--network", "n.sif"]
    for args, words in ((base, "one of the arguments --diseases --drugs --seeds is required"),
                        (base + ["--seeds", "s", "--drugs", "t"], "not allowed with argument"),
                        (base + ["--seeds", "s", "--max-add", "0"], "--max-add 0 must be >= 1"),
                        (base + ["--seeds", "s", "--n-random", "1"], "--n-random 1: need at least 2"),
                        (base + ["--seeds", "s", "--min-bin-size", "0"], "--min-bin-size 0 must be >= 1"),
                        (base + ["--seeds", "s", "--n-random", "0", "--null", "x"], "--null needs --n-random >= 2")):
        with pytest.raises(SystemExit) as e:
            connectors_cli.parse_args(args)
        assert e.value.code == 2 and words in capsys.readouterr().err, args
    a = connectors_cli.parse_args(base + ["--diseases", "d.tsv", "--set", "x"])
    assert (a.max_add, a.n_random, a.seed, a.min_bin_size, a.out, a.connectors, a.summary, a.genes, a.null, a.set) == (
        500, 1000, 452456, 100, "modules.tsv", None, None, None, None, ["x"])
    assert connectors_cli.parse_args(base + ["--seeds", "s", "--n-random", "0"]).n_random == 0
