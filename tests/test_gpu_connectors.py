"""-m gpu: ConnectorEngine (gcn-drug-repurposing_amd/connectors.py) and seed_connectors.py as a fresh child process on the toy network
tests/golden/diamond_toy.sif with the three seed sets of tests/golden/diamond_toy_seeds.tsv (two of them grow by a step, one is connected
already), against the mirror (tests/connectors_mirror.py): modules.tsv, connectors.tsv and the gene table are the mirror's growth
through the same writers, summary.tsv is table_stats over the mirror's growth of the very random sets the engine drew (read back through
ModuleEngine.set_table, which draws them bit for bit), and disease_modules.py reads the gene table that was written."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import connectors_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import connectors, connectors_cli, diamond_cli, proximity as P, set_modules  # noqa: E402

pytestmark = pytest.mark.gpu
NET = os.path.join(HERE, "golden", "diamond_toy.sif")
SEEDS = os.path.join(HERE, "golden", "diamond_toy_seeds.tsv")
MAX_ADD, N_RANDOM, SEED, MIN_BIN = 4, 12, 7, 3
STEP, UNIT = ("node", "lcc", "merged", "deg"), ("steps", "first_lcc", "final_lcc", "seeds_in", "added_in")


@pytest.fixture(scope="module")
def toy():
    net = P.read_network(NET)
    sets = diamond_cli.load_seed_sets(SEEDS)
    names = sorted(sets)
    members = [net.node_set(sets[n]) for n in names]
    assert net.n == 11 and names == ["first set", "second", "third"] and [len(m) for m in members] == [3, 2, 3]      # Z is no node
    return net, names, sets, members


def mirrored(net, units, n_add):
    """the mirror's table of `units` in the shape of ConnectorEngine.grow's return"""
    want = M.table(net.rowptr, net.col, units, n_add)
    return dict({f: want[f] for f in STEP + UNIT}, members=[x.astype(np.int32) for x in want["members"]], label=want["label"])


def same_growth(got, want):
    for f in STEP + UNIT:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), f
    for key in ("members", "label"):
        assert len(got[key]) == len(want[key]) and all(np.array_equal(a, b) for a, b in zip(got[key], want[key])), key


def random_units(net, members, side):
    """the engine's random sets, read back: a list over sets of lists over samples (sample 0 the set) of node arrays, and the sizes"""
    mod = set_modules.ModuleEngine(net)
    try:
        nodes, sizes = mod.set_table(members, side, N_RANDOM, SEED, P.degree_bins(net.degree, MIN_BIN))
    finally:
        mod.close()
    nodes, sizes = nodes.cpu().numpy(), sizes.cpu().numpy()
    return [[nodes[i, r, :sizes[i, r]] for r in range(N_RANDOM + 1)] for i in range(len(members))], sizes


def test_engine_grow_and_table_equal_the_mirror(toy):
    net, names, sets, members = toy
    more = members + [net.node_set(set(g)) for g in ("IJKGH", "IK", "J", "EIK", "")]     # three steps with a tie, no gain, one gene, no gene
    eng = connectors.ConnectorEngine(net)
    try:
        got = eng.grow(more, n_add=MAX_ADD)
        want = mirrored(net, more, MAX_ADD)
        same_growth(got, want)
        assert got["steps"].tolist() == [1, 0, 1, 3, 0, 0, 1, 0] and [net.names[v] for v in got["node"][3, :3]] == ["B", "A", "C"]
        one = eng.grow(more, n_add=1)                                                     # n_add ends the fourth set's growth
        same_growth(one, mirrored(net, more, 1))
        res = eng.connector_table([sets[n] for n in names] + [{"J"}], 1, n_add=MAX_ADD, n_random=N_RANDOM, seed=SEED, min_bin_size=MIN_BIN)
        units, sizes = random_units(net, members + [net.node_set({"J"})], 1)
        assert np.array_equal(res["sizes"], sizes) and all(np.array_equal(units[i][0], m) for i, m in enumerate(members))
        flat = M.table(net.rowptr, net.col, [x for per_set in units for x in per_set], MAX_ADD)
        for f in ("steps", "final_lcc", "seeds_in"):
            assert np.array_equal(res[f], flat[f].reshape(4, N_RANDOM + 1)), f
        stats = connectors.table_stats([3, 2, 3, 1], sizes, *(flat[f].reshape(4, N_RANDOM + 1) for f in ("steps", "final_lcc", "seeds_in")))
        for key in ("joined_stats", "fraction_stats", "lcc_stats"):
            for f in set_modules.STAT_FIELDS:
                assert np.array_equal(res[key][f], stats[key][f], equal_nan=True), (key, f)
        assert np.isnan(res["joined_stats"]["p"][3]) and not np.isnan(res["joined_stats"]["q"][:3]).any()
        assert np.array_equal(res["connectors"], [1, 0, 1, 0]) and np.array_equal(res["connectors_null_mean"], stats["connectors_null_mean"], equal_nan=True)
        assert len({tuple(x.tolist()) for x in units[0][1:]}) > 1                        # the null is not one set repeated
        none = eng.connector_table([sets[n] for n in names], 0, n_add=MAX_ADD, n_random=0)
        assert "joined_stats" not in none and none["steps"].shape == (3, 1)
        same_growth(none["grow"], mirrored(net, members, MAX_ADD))
        old = connectors.CHUNK_BYTES
        connectors.CHUNK_BYTES = 16 * MAX_ADD * 5                                         # five units per call: same integers
        try:
            again = eng.connector_table([sets[n] for n in names] + [{"J"}], 1, n_add=MAX_ADD, n_random=N_RANDOM, seed=SEED, min_bin_size=MIN_BIN)
        finally:
            connectors.CHUNK_BYTES = old
        assert all(np.array_equal(again[f], res[f]) for f in ("steps", "final_lcc", "seeds_in", "sizes"))
        same_growth(again["grow"], res["grow"])
    finally:
        eng.close()
    with pytest.raises(P.ProximityError, match="the engine is closed"):
        eng.grow(members)


def program(tmp_path, script, *args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *args], cwd=str(tmp_path), capture_output=True, text=True, env=env,
                          timeout=600)


def test_seed_connectors_end_to_end(tmp_path, toy):
    net, names, sets, members = toy
    r = program(tmp_path, "seed_connectors.py", "--network", NET, "--seeds", SEEDS, "--max-add", str(MAX_ADD), "--n-random", str(N_RANDOM), "--seed",
                str(SEED), "--min-bin-size", str(MIN_BIN), "--out", "m.tsv", "--connectors", "c.tsv", "--summary", "s.tsv", "--genes", "g.tsv",
                "--null", "null.npy")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().split("\n")[-1].startswith(f"seed_connectors: 3 sets, max_add={MAX_ADD}, n_random={N_RANDOM}, LCC 11 nodes, 2 connectors, ")
    grown = mirrored(net, members, MAX_ADD)
    for name, writer in (("m.tsv", connectors_cli.write_modules), ("c.tsv", connectors_cli.write_connectors), ("g.tsv", connectors_cli.write_genes)):
        writer(tmp_path / ("want_" + name), names, net.names, grown)
        assert (tmp_path / name).read_text() == (tmp_path / ("want_" + name)).read_text(), name
    assert (tmp_path / "m.tsv").read_text().split("\n")[1] == "first set\t1\tA\t4\t3\t7"
    units, sizes = random_units(net, members, 1)                                          # --seeds draws the diseases' side
    flat = M.table(net.rowptr, net.col, [x for per_set in units for x in per_set], MAX_ADD)
    per = {f: flat[f].reshape(3, N_RANDOM + 1) for f in ("steps", "final_lcc", "seeds_in")}
    stats = connectors.table_stats([3, 2, 3], sizes, per["steps"], per["final_lcc"], per["seeds_in"])
    connectors_cli.write_summary(tmp_path / "want_s.tsv", names, dict(stats, n=np.array([3, 2, 3]), grow=grown))
    assert (tmp_path / "s.tsv").read_text() == (tmp_path / "want_s.tsv").read_text()
    null = np.load(tmp_path / "null.npy")
    assert null.dtype == np.int32 and np.array_equal(null, np.stack([per[f][:, 1:] for f in ("steps", "final_lcc", "seeds_in")], axis=1))
    # disease_modules.py takes the grown modules as a gene table
    r = program(tmp_path, "disease_modules.py", "--network", NET, "--diseases", "g.tsv", "--n-random", "8", "--min-bin-size", str(MIN_BIN), "--out", "dm.tsv")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [line.split("\t") for line in (tmp_path / "dm.tsv").read_text().split("\n")[1:-1]]
    assert [x[:3] for x in rows] == [["first.set", "4", "4"], ["second", "2", "2"], ["third", "4", "4"]]        # n and n.lcc: the modules are connected
    # without a null: the growth alone, NA in the summary
    r = program(tmp_path, "seed_connectors.py", "--network", NET, "--seeds", SEEDS, "--set", "third", "--max-add", "2", "--n-random", "0", "--out", "m0.tsv",
                "--summary", "s0.tsv")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "m0.tsv").read_text() == "set\trank\tgene\tlcc\tmerged\tdegree\nthird\t1\tA\t4\t3\t7\n"
    assert (tmp_path / "s0.tsv").read_text().split("\n")[1].split("\t") == ["third", "3", "1", "4", "3", "1"] + ["NA"] * 18


def test_seed_connectors_exit_statuses(tmp_path):
    r = program(tmp_path, "seed_connectors.py", "--network", NET, "--seeds", SEEDS, "--max-add", "0")
    assert r.returncode == 2 and "--max-add 0 must be >= 1" in r.stderr and r.stdout == ""
    r = program(tmp_path, "seed_connectors.py", "--network", NET, "--seeds", str(tmp_path / "missing.tsv"))
    assert r.returncode == 1 and r.stderr.startswith("seed_connectors: ") and r.stderr.count("\n") == 1, r.stderr
    r = program(tmp_path, "seed_connectors.py", "--network", NET, "--seeds", SEEDS, "--set", "fourth")
    assert r.returncode == 1 and "no set named 'fourth'" in r.stderr
    assert not os.path.exists(tmp_path / "modules.tsv")
