"""-m gpu: the module check on the 2016 network (tests/golden/proximity_2016.npz through proximity_mirror.Fixture) against the golden
integers of tests/golden/set_modules_2016.npz (the mirror's; tests/test_set_modules_mirror.py keeps that file honest), and
disease_modules.py as a fresh child process on a toy network.

Exact throughout: the set tables of ModuleEngine and ProximityEngine bit for bit (these are the random sets the proximity z-scores are
computed against: side 0 the drugs, side 1 the diseases, one seed), the integer tables of all 78 diseases x 1,001 samples and of the 238
drug sets, the statistics as null_stats of the golden integers, the labels as the mirror's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import proximity_mirror as PM  # noqa: E402
import set_modules_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import modules_cli, proximity as P, set_modules  # noqa: E402
from gcn_drug_repurposing_amd._nulls import benjamini_hochberg  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return PM.Fixture()


@pytest.fixture(scope="module")
def golden():
    return M.load_fixture()


@pytest.fixture(scope="module")
def engine(fx):
    eng = set_modules.ModuleEngine(fx.net)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def inputs(fx):
    _, _, diseases, drugs = M.fixture_inputs(fx)
    return P.degree_bins(fx.net.degree, M.MIN_BIN), diseases, drugs


@pytest.fixture(scope="module")
def disease_table(engine, inputs):
    bins, diseases, _ = inputs
    return engine.set_table(diseases, 1, M.N_RANDOM, M.SEED, bins)


@pytest.fixture(scope="module")
def result(engine, fx):
    return engine.module_table(fx.diseases, 1, n_random=M.N_RANDOM, seed=M.SEED, min_bin_size=M.MIN_BIN)


def test_set_tables_equal_the_proximity_engines_bit_for_bit(fx, engine, inputs, disease_table):
    bins, diseases, drugs = inputs
    prox = P.ProximityEngine(fx.net)
    try:
        for side, sets, mine in ((1, diseases, disease_table), (0, drugs, engine.set_table(drugs, 0, M.N_RANDOM, M.SEED, bins))):
            nodes, sizes = prox.set_table(sets, side, M.N_RANDOM, M.SEED, bins)
            assert mine[0].shape == nodes.shape and mine[0].dtype == nodes.dtype == torch.int32
            assert torch.equal(mine[0], nodes) and torch.equal(mine[1], sizes), side
            assert nodes.shape[:2] == (len(sets), M.N_RANDOM + 1) and nodes.shape[2] == max(len(s) for s in sets)
    finally:
        prox.close()
    other = engine.set_table(diseases[:3], 0, 5, M.SEED, bins)                  # the sides do draw differently
    assert not torch.equal(other[0][:, 1:], disease_table[0][:3, 1:6, :other[0].shape[2]])


def test_disease_tables_equal_the_golden_file(engine, disease_table, golden):
    lcc, n_comp, n_edges = (x.cpu().numpy() for x in engine.components(*disease_table))
    want = golden["disease"].astype(np.int32)
    for got, w, field in ((lcc, want[0], "lcc"), (n_comp, want[1], "n_comp"), (n_edges, want[2], "n_edges")):
        assert got.dtype == np.int32 and got.shape == (78, M.N_RANDOM + 1)
        assert np.array_equal(got, w), (field, np.argwhere(got != w)[:5])
    again = engine.components(*disease_table)
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(again, (lcc, n_comp, n_edges)))
    half = engine.components(disease_table[0][40:], disease_table[1][40:])      # a split of the units: the same integers
    assert np.array_equal(half[0].cpu().numpy(), lcc[40:]) and np.array_equal(half[2].cpu().numpy(), n_edges[40:])


def test_drug_triples_equal_the_golden_file(engine, inputs, golden):
    bins, _, drugs = inputs
    nodes, sizes = engine.set_table(drugs, 0, 0, M.SEED, bins)
    got = np.stack([x.cpu().numpy()[:, 0] for x in engine.components(nodes, sizes)])
    assert nodes.shape == (238, 1, 26) and np.array_equal(got, golden["drug"].astype(np.int32))


def test_module_table_statistics_equal_null_stats_of_the_golden_integers(result, golden, inputs):
    d = golden["disease"].astype(np.int64)
    assert np.array_equal(result["n"], [len(s) for s in inputs[1]]) and np.array_equal(result["short"], golden["disease_short"])
    for key, row in (("lcc", 0), ("n_comp", 1), ("n_edges", 2)):
        assert np.array_equal(result[key], d[row, :, 0]), key
    assert np.array_equal(result["null_lcc"], d[0, :, 1:]) and np.array_equal(result["null_edges"], d[2, :, 1:])
    assert result["null_lcc"].dtype == np.int32 and result["null_lcc"].shape == (78, M.N_RANDOM)
    for key, row in (("lcc_stats", 0), ("edges_stats", 2)):
        want = set_modules.null_stats(d[row, :, 0], d[row, :, 1:])
        for f in set_modules.STAT_FIELDS:
            assert np.array_equal(result[key][f].view(np.int64), want[f].view(np.int64)), (key, f)
    assert int((result["lcc_stats"]["z"] > 1.65).sum()) == 61


def test_observed_labels_equal_the_mirror(result, fx, inputs):
    for j, members in enumerate(inputs[1]):
        lcc, n_comp, _, labels = M.components(fx.net.rowptr, fx.net.col, members)
        assert np.array_equal(result["members"][j], members) and np.array_equal(result["label"][j], labels), j
        assert np.bincount(result["label"][j]).max() == lcc == result["lcc"][j] and len(set(result["label"][j].tolist())) == n_comp


def test_an_empty_set_is_nan_and_takes_no_part_in_q(engine, fx):
    r = engine.module_table([fx.diseases[0], {"no such gene"}, fx.diseases[77]], 1, n_random=50)
    alone = engine.module_table([fx.diseases[0], fx.diseases[77]], 1, n_random=50)
    assert r["n"].tolist() == [32, 0, 181] and r["lcc"].tolist() == [6, 0, 53] and r["n_comp"][1] == 0 and r["short"][1] == 0
    for key in ("lcc_stats", "edges_stats"):
        assert all(np.isnan(r[key][f][1]) for f in set_modules.STAT_FIELDS)
        assert np.array_equal(r[key]["q"][[0, 2]], benjamini_hochberg(r[key]["p"][[0, 2]]))   # q over the two live sets
        assert np.array_equal(r[key]["z"][[0]], alone[key]["z"][[0]])
    assert len(r["members"][1]) == 0 and len(r["label"][1]) == 0
    # set 2 of the first call is set 1 of the second: other random sets (the key holds the set's index), the same observed values
    assert r["lcc"][2] == alone["lcc"][1] and r["n_edges"][2] == alone["n_edges"][1]


# ---- the command, as a fresh child process ---------------------------------------------------------------------------------------------

N_RANDOM, SEED, MIN_BIN = 40, 11, 4


def write_toy(tmp_path):
    """a ring of 40 genes with chords and pendant genes (degrees 1 .. 6), and a triangle apart from it (outside the LCC)"""
    rng = np.random.RandomState(1)
    edges = [(i, (i + 1) % 40) for i in range(40)] + [tuple(e) for e in rng.randint(0, 40, (25, 2))] + [(40 + i, i * 3) for i in range(10)]
    edges += [(100, 101), (101, 102), (100, 102)]
    (tmp_path / "net.sif").write_text("".join(f"{a} pp {b}\n" for a, b in edges))
    sets = {"Alpha disease": [0, 1, 2, 3, 4, 10, 11, 41, 100], "beta, two": [5, 15, 25, 35, 45, 46], "Gamma": [100, 101, 777]}
    (tmp_path / "dis.tsv").write_text("".join("\t" + name + "\t" + "\t".join(map(str, g)) + "\n" for name, g in sets.items()))
    return str(tmp_path / "net.sif"), str(tmp_path / "dis.tsv")


def program(tmp_path, *args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, "disease_modules.py"), *args], cwd=str(tmp_path), capture_output=True, text=True,
                          env=env, timeout=600)


def test_disease_modules_end_to_end(tmp_path):
    net_path, dis_path = write_toy(tmp_path)
    r = program(tmp_path, "--network", net_path, "--diseases", dis_path, "--n-random", str(N_RANDOM), "--seed", str(SEED), "--min-bin-size",
                str(MIN_BIN), "--out", "m.tsv", "--members", "mem.tsv", "--null", "null.npy")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    net = P.read_network(net_path)
    assert net.n == 50
    sets = P.load_disease_genes(dis_path)
    names = sorted(sets)
    assert names == ["alpha.disease", "beta.two", "gamma"]
    last = r.stdout.strip().split("\n")[-1]
    assert last.startswith(f"disease_modules: 3 sets, n_random={N_RANDOM}, LCC 50 nodes, ") and last.endswith(" s")
    # the mirror on the same inputs, in the order of the program's rows; side 1 and the row's index key the random sets
    bin_list = PM.bins(net.degree, MIN_BIN)
    node_bin = PM.bin_of(bin_list, net.n)
    members = [net.node_set(sets[n]) for n in names]
    assert [len(m) for m in members] == [8, 6, 0]
    tabs = [M.module_nulls(net.rowptr, net.col, m, node_bin, bin_list, SEED, 1, j, N_RANDOM) for j, m in enumerate(members)]
    t = np.stack([x[0] for x in tabs], axis=1)                                    # [3 fields, 3 sets, 1 + n_random]
    null = np.load(tmp_path / "null.npy")
    assert null.dtype == np.int32 and null.shape == (3, 2, N_RANDOM)
    assert np.array_equal(null[:, 0], t[0, :, 1:]) and np.array_equal(null[:, 1], t[2, :, 1:])
    empty = np.array([len(m) == 0 for m in members])
    want = {"n": [len(m) for m in members], "lcc": t[0, :, 0], "n_comp": t[1, :, 0], "n_edges": t[2, :, 0],
            "short": [int((x[1][1:] < x[1][0]).sum()) for x in tabs], "lcc_stats": set_modules.null_stats(t[0, :, 0], t[0, :, 1:], empty),
            "edges_stats": set_modules.null_stats(t[2, :, 0], t[2, :, 1:], empty), "members": members,
            "label": [M.components(net.rowptr, net.col, m)[3] for m in members]}
    assert want["lcc"][0] >= 5 and want["n_comp"][1] >= 3 and f"{int(np.sum(want['lcc_stats']['q'] <= 0.05))} with lcc.q <= 0.05" in last
    modules_cli.write_table(tmp_path / "want.tsv", names, want)
    modules_cli.write_members(tmp_path / "want_mem.tsv", names, net.names, want)
    assert (tmp_path / "m.tsv").read_text() == (tmp_path / "want.tsv").read_text()
    assert (tmp_path / "mem.tsv").read_text() == (tmp_path / "want_mem.tsv").read_text()
    rows = (tmp_path / "m.tsv").read_text().split("\n")
    assert rows[3].split("\t")[:5] == ["gamma", "0", "0", "0", "0"] and rows[3].split("\t")[5:15] == ["NA"] * 10
    assert (tmp_path / "mem.tsv").read_text().count("\n") == 1 + 8 + 6


def test_disease_modules_exit_statuses(tmp_path):
    net_path, dis_path = write_toy(tmp_path)
    r = program(tmp_path, "--network", net_path, "--diseases", dis_path, "--n-random", "1")
    assert r.returncode == 2 and "--n-random 1: need at least 2 random samples" in r.stderr and r.stdout == ""
    r = program(tmp_path, "--network", net_path)
    assert r.returncode == 2 and "one of the arguments --diseases --drugs is required" in r.stderr
    r = program(tmp_path, "--network", net_path, "--diseases", str(tmp_path / "missing.tsv"))
    assert r.returncode == 1 and r.stderr.startswith("disease_modules: ") and r.stderr.count("\n") == 1, r.stderr
    assert not os.path.exists(tmp_path / "modules.tsv")
