"""CPU: the component search's mirror (tests/set_modules_mirror.py) against scipy and networkx on every case of
tests/set_modules_cases.py, the property each case was built for, that every named wrong rule (ABLATIONS) changes an asserted output, the
statistics (set_modules.null_stats) on hand values, the writers and the argument refusals of disease_modules.py, and the golden file
tests/golden/set_modules_2016.npz: four diseases recomputed in full, and the figures the module check was proposed with, computed from
the file."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proximity_mirror as PM  # noqa: E402
import set_modules_cases as K  # noqa: E402
import set_modules_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import modules_cli, set_modules  # noqa: E402

CHECKED_UNITS = 1500            # of the 70,000-unit case: the closed form it carries against the mirror, scipy and networkx


def _units(name):
    c = K.case(name)
    return c, (c.units[:CHECKED_UNITS] if name == "grid_70000" else c.units)


def _canonical(comp):
    """component ids of one unit -> per member the smallest position with the same id"""
    first = {}
    for i, x in enumerate(comp):
        first.setdefault(int(x), i)
    return np.array([first[int(x)] for x in comp], np.int64)


def _summary(lab):
    return (int(np.bincount(lab).max()) if len(lab) else 0, len(set(lab.tolist())))


@pytest.mark.parametrize("name", K.CASES)
def test_mirror_equals_scipy_and_networkx(name):
    import networkx as nx
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    c, units = _units(name)
    lcc, n_comp, n_edges, lab = K.mirror(name)
    A = sp.csr_matrix((np.ones(len(c.col), np.int8), c.col, c.rowptr), shape=(c.n, c.n))
    G = nx.Graph()
    G.add_nodes_from(range(c.n))
    rows = np.repeat(np.arange(c.n), np.diff(c.rowptr))
    G.add_edges_from(zip(rows.tolist(), c.col.tolist()))
    for k, u in enumerate(units):
        m = len(u)
        got = lab[k, :m]
        assert (lab[k, m:] == -1).all()
        assert (lcc[k], n_comp[k]) == _summary(got), (name, k)
        if m == 0:
            assert (lcc[k], n_comp[k], n_edges[k]) == (0, 0, 0)
            continue
        sub = A[u][:, u]
        assert np.array_equal(got, _canonical(connected_components(sub, directed=False)[1])), (name, k)
        where = {int(v): i for i, v in enumerate(u)}
        by_nx = np.empty(m, np.int64)
        for comp in nx.connected_components(G.subgraph(u.tolist())):
            by_nx[[where[v] for v in comp]] = min(where[v] for v in comp)
        assert np.array_equal(got, by_nx), (name, k)
        if c.symmetric:
            assert n_edges[k] == (sub.nnz - sub.diagonal().sum()) // 2 == G.subgraph(u.tolist()).number_of_edges() - int(sub.diagonal().sum())


@pytest.mark.parametrize("name", [n for n in K.CASES if K.case(n).want is not None])
def test_every_case_has_the_property_it_was_built_for(name):
    c = K.case(name)
    lcc, n_comp, n_edges, lab = K.mirror(name)
    assert [(int(a), int(b), int(e)) for a, b, e in zip(lcc, n_comp, n_edges)] == [tuple(w) for w in c.want]
    deg = np.diff(c.rowptr)
    if name.endswith("_path") or name.endswith("_apart") or name.endswith("_tie"):
        u = c.units[0]
        assert c.max_size == max(len(u), 1)                                      # the row is exactly as long as the set
        inside = np.isin(c.col, u)
        rows = np.repeat(np.arange(c.n), deg)
        assert len(u) == 0 or (~inside[np.isin(rows, u)]).any()                  # neighbours outside the set
    if name.endswith("_path") and len(c.units[0]) > 64:
        # in node order the path is shuffled: a sweep of min-label propagation in row order leaves many labels unresolved
        assert M.components(c.rowptr, c.col, c.units[0], "one_sweep")[1] > 1
    if name.endswith("_tie"):
        a, b = c.tie_labels
        count = np.bincount(lab[0, :len(c.units[0])])
        assert a < b and count[a] == count[b] == count.max() and (count == count.max()).sum() == 2
        assert M.largest_label(lab[0, :len(c.units[0])]) == a == set_modules.largest_component(lab[0, :len(c.units[0])])
    if name == "hub":
        assert deg[K.HUB] == K.HUB_DEG and set(K.HUB_AT) <= set(c.row_positions.tolist())
        row = c.col[c.rowptr[K.HUB]:c.rowptr[K.HUB + 1]]
        assert np.array_equal(np.sort(row[c.row_positions]), c.units[1])
    if name == "selfloop":
        assert 9 in c.col[c.rowptr[9]:c.rowptr[10]]
    if name == "bounds":
        r20 = c.col[c.rowptr[20]:c.rowptr[21]]
        assert r20.min() < 10 and r20.max() > 30
    if name == "oneway":
        assert not c.symmetric and 10 in c.col[c.rowptr[30]:c.rowptr[31]] and 30 not in c.col[c.rowptr[10]:c.rowptr[11]]


def test_the_large_launches_are_what_they_claim():
    c = K.case("many_3000")
    sizes = np.array([len(u) for u in c.units])
    nodes, sz = K.table_arrays(c)
    assert len(c.units) == 3000 and sizes.min() == 0 and sizes.max() == 130 < c.max_size and np.array_equal(sz, sizes)
    assert set(np.unique(nodes[0]).tolist()) == {-1, 0x7FFFFFFF} and nodes[1, 130] in K.FILL and nodes[1, 131] in K.FILL
    lcc, n_comp, n_edges, _ = K.mirror("many_3000")
    assert lcc.max() > 20 and n_edges.max() > 20 and (n_comp[sizes > 0] >= 1).all()
    g = K.case("grid_70000")
    gs = np.array([len(u) for u in g.units])
    assert len(g.units) == 70000 > 65535 and set(gs.tolist()) == {1, 2, 3}
    glcc, gcomp, gedges, glab = K.mirror("grid_70000")
    want = M.table(g.rowptr, g.col, g.units[:CHECKED_UNITS])                   # the closed form against the union-find
    assert np.array_equal(glcc[:CHECKED_UNITS], want[0]) and np.array_equal(gcomp[:CHECKED_UNITS], want[1])
    assert np.array_equal(gedges[:CHECKED_UNITS], want[2])
    for k, l in enumerate(want[3]):
        assert np.array_equal(glab[k, :len(l)], l) and (glab[k, len(l):] == -1).all()
    assert set(glcc.tolist()) == {1, 2, 3} and set(gedges.tolist()) == {0, 1, 2, 3}


# every wrong rule, and a case (unit 0 unless named) on which an asserted output changes
ABLATION_CASE = {"one_sweep": "size_257_path", "rounds_32": "size_255_path", "miss_last": "bounds", "miss_first": "oneway", "row_64": "hub",
                 "self_loop_edge": "selfloop", "tie_larger": "size_63_tie", "past_size": "bounds"}


def test_every_ablation_changes_an_asserted_output():
    assert set(ABLATION_CASE) == set(M.ABLATIONS)
    for rule, name in ABLATION_CASE.items():
        c = K.case(name)
        lcc, n_comp, n_edges, lab = K.mirror(name)
        m = len(c.units[0])
        if rule == "tie_larger":
            assert M.largest_label(lab[0, :m], rule) == c.tie_labels[1] != M.largest_label(lab[0, :m])
            continue
        tail = K.table_arrays(c)[0][0, m:]
        got = M.components(c.rowptr, c.col, c.units[0], rule, tail=tail)
        assert got[:3] != (lcc[0], n_comp[0], n_edges[0]) or not np.array_equal(got[3], lab[0, :m]), rule
        assert M.components(c.rowptr, c.col, c.units[0], None, tail=tail)[:3] == (lcc[0], n_comp[0], n_edges[0])


# ---- the statistics -------------------------------------------------------------------------------------------------------------------

def test_null_stats_on_hand_values():
    obs = np.array([5, 3, 0, 2])
    null = np.array([[1, 2, 3, 6], [3, 3, 3, 3], [0, 0, 0, 0], [1, 3, 1, 3]])
    s = set_modules.null_stats(obs, null, empty=np.array([False, False, True, False]))
    assert s["mean"][0] == 3.0 and s["sd"][0] == np.sqrt(3.5) and s["z"][0] == 2.0 / np.sqrt(3.5) and s["p"][0] == 2 / 5
    assert s["mean"][1] == 3.0 and s["sd"][1] == 0.0 and np.isnan(s["z"][1]) and s["p"][1] == 1.0      # sd = 0: no z, p counts the ties
    assert all(np.isnan(s[k][2]) for k in set_modules.STAT_FIELDS)                                       # an empty set
    assert s["mean"][3] == 2.0 and s["sd"][3] == 1.0 and s["z"][3] == 0.0 and s["p"][3] == 3 / 5
    # q: Benjamini-Hochberg over the three live sets, p = 0.4, 1.0, 0.6 -> 0.4 * 3 / 1 capped by the later ones, 0.6 * 3 / 2, 1.0
    assert np.array_equal(s["q"][[0, 1, 3]], [min(1.0, 0.4 * 3, 0.6 * 3 / 2), 1.0, 0.6 * 3 / 2])
    everyone = set_modules.null_stats(obs, null)
    assert everyone["mean"][2] == 0.0 and everyone["p"][2] == 1.0 and np.isnan(everyone["z"][2]) and not np.isnan(everyone["q"]).any()
    sd = set_modules.null_stats([7], [[1, 2, 3, 4, 5, 6, 7, 8]])                                       # population sd, ddof = 0
    assert sd["sd"][0] == np.std(np.arange(1, 9)) != np.std(np.arange(1, 9), ddof=1) and sd["p"][0] == 3 / 9
    with pytest.raises(ValueError, match="no sample"):
        set_modules.null_stats([1], np.zeros((1, 0)))


def _injected():
    nan = np.nan
    lcc = {"mean": np.array([1.5, nan]), "sd": np.array([0.5, nan]), "z": np.array([3.0, nan]), "p": np.array([0.25, nan]),
           "q": np.array([0.25, nan])}
    edges = {"mean": np.array([0.1, nan]), "sd": np.array([0.0, nan]), "z": np.array([nan, nan]), "p": np.array([1 / 3, nan]),
             "q": np.array([1 / 3, nan])}
    return {"n": np.array([5, 0]), "lcc": np.array([2, 0]), "n_comp": np.array([3, 0]), "n_edges": np.array([2, 0]), "short": np.array([4, 0]),
            "lcc_stats": lcc, "edges_stats": edges, "members": [np.array([0, 2, 3, 5, 6]), np.zeros(0, np.int64)],
            "label": [np.array([0, 1, 0, 1, 4]), np.zeros(0, np.int64)]}


def test_writers_on_injected_arrays(tmp_path):
    res = _injected()
    modules_cli.write_table(tmp_path / "m.tsv", ["a.b", "empty"], res)
    lines = (tmp_path / "m.tsv").read_text().split("\n")
    assert lines[0] == ("set\tn\tn.lcc\tn.components\tn.edges\tlcc.mean\tlcc.sd\tlcc.z\tlcc.p\tlcc.q\tedges.mean\tedges.sd\tedges.z\tedges.p\t"
                        "edges.q\tshort")
    assert lines[1] == f"a.b\t5\t2\t3\t2\t1.5\t0.5\t3.0\t0.25\t0.25\t0.1\t0.0\tNA\t{1 / 3!r}\t{1 / 3!r}\t4"
    assert lines[2] == "empty\t0\t0\t0\t0" + "\tNA" * 10 + "\t0" and lines[3:] == [""]
    genes = [f"g{i}" for i in range(7)]
    modules_cli.write_members(tmp_path / "mem.tsv", ["a.b", "empty"], genes, res)
    # two components of two members each: the one with the smaller label (0) is the LCC
    assert (tmp_path / "mem.tsv").read_text() == ("set\tgene\tcomponent\tin_lcc\na.b\tg0\t0\t1\na.b\tg2\t1\t0\na.b\tg3\t0\t1\na.b\tg5\t1\t0\n"
                                                  "a.b\tg6\t4\t0\n")


def test_argument_refusals_exit_2(capsys):
    base = ["--network", "n.sif"]
    for args, words in ((base, "one of the arguments --diseases --drugs is required"),
                        (base + ["--diseases", "d.tsv", "--drugs", "t.pcl"], "not allowed with argument"),
                        (["--diseases", "d.tsv"], "--network"),
                        (base + ["--diseases", "d.tsv", "--n-random", "1"], "--n-random 1: need at least 2 random samples"),
                        (base + ["--drugs", "t.pcl", "--min-bin-size", "0"], "--min-bin-size 0 must be >= 1")):
        with pytest.raises(SystemExit) as e:
            modules_cli.parse_args(args)
        assert e.value.code == 2 and words in capsys.readouterr().err, args
    a = modules_cli.parse_args(base + ["--drugs", "t.pcl"])
    assert (a.n_random, a.seed, a.min_bin_size, a.out, a.members, a.null, a.diseases) == (1000, 452456, 100, "modules.tsv", None, None, None)


def test_module_table_refusals_need_no_device():
    """the argument checks of module_table come before anything touches the GPU"""
    eng = set_modules.ModuleEngine.__new__(set_modules.ModuleEngine)
    eng.net = type("Net", (), {"node_set": staticmethod(lambda s: np.arange(len(s), dtype=np.int32))})()
    for kw, words in ((dict(n_random=1), "n_random=1: need at least 2 random samples"), (dict(min_bin_size=0), "min_bin_size=0 must be >= 1")):
        with pytest.raises(set_modules.ProximityError, match=words):
            eng.module_table([{"1"}], 1, **kw)
    with pytest.raises(set_modules.ProximityError, match="a set has 4097 genes in the LCC; at most 4096 are supported"):
        eng.module_table([set(range(4097))], 1)
    eng._rowptr = eng._col = None                         # what close() leaves; __del__ closes again


# ---- the golden file ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fx():
    return PM.Fixture()


@pytest.fixture(scope="module")
def golden():
    return M.load_fixture()


def test_golden_file_is_what_the_mirror_computes(fx, golden):
    bin_list, node_bin, diseases, drugs = M.fixture_inputs(fx)
    assert golden["disease"].shape == (3, 78, M.N_RANDOM + 1) and golden["drug"].shape == (3, 238) and golden["disease"].dtype == np.int16
    for j in (0, 9, 40, 77):
        t, sizes = M.module_nulls(fx.net.rowptr, fx.net.col, diseases[j], node_bin, bin_list, M.SEED, 1, j, M.N_RANDOM)
        assert np.array_equal(t, golden["disease"][:, j]), j
        assert int((sizes[1:] < sizes[0]).sum()) == golden["disease_short"][j]
    assert np.array_equal(np.stack(M.table(fx.net.rowptr, fx.net.col, drugs)[:3]), golden["drug"])


def test_the_fixture_carries_signal(fx, golden):
    """the figures the check was proposed with, from the file"""
    net = fx.net
    assert (net.n, len(net.col), int(np.diff(net.rowptr).max())) == (13329, 276712, 870)
    n = np.array([len(net.node_set(s)) for s in fx.diseases])
    assert (n.min(), n.max()) == (20, 482)
    d = golden["disease"].astype(np.int64)
    assert tuple(d[:, 0, 0]) == (6, 24, 9) and n[0] == 32 and tuple(d[:, 77, 0]) == (53, 111, 88) and n[77] == 181
    assert (golden["disease_short"] == 0).all()
    s = set_modules.null_stats(d[0, :, 0], d[0, :, 1:])
    assert (s["sd"] > 0).all() and not np.isnan(s["z"]).any()
    assert (round(float(s["z"].min()), 2), round(float(s["z"].max()), 1), round(float(np.median(s["z"])), 2)) == (-0.96, 33.2, 3.88)
    assert int((s["z"] > 1.65).sum()) == 61
    sizes = np.array([len(net.node_set(t)) for t in fx.drugs])
    assert (sizes == 1).sum() == 76 and sizes.max() == 26
    assert np.array_equal(golden["drug"][1].astype(np.int64) <= sizes, np.ones(238, bool))
