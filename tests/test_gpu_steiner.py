"""-m gpu: SteinerEngine (gcn-drug-repurposing_amd/steiner.py) and steiner.py as a fresh child process on the toy network
tests/golden/diamond_toy.sif with the three seed sets of tests/golden/diamond_toy_seeds.tsv, against the mirror
(tests/steiner_mirror.py): edges.tsv, nodes.tsv and the gene table are the mirror's trees through the same writers, summary.tsv is
table_stats over the mirror's trees of the very random sets the engine drew (read back through ModuleEngine.set_table, which draws
them bit for bit), and disease_modules.py reads the gene table that was written."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import steiner_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _sets_cli, proximity as P, set_modules, steiner, steiner_cli  # noqa: E402

pytestmark = pytest.mark.gpu
NET = os.path.join(HERE, "golden", "diamond_toy.sif")
SEEDS = os.path.join(HERE, "golden", "diamond_toy_seeds.tsv")
MAX_ADD, N_RANDOM, SEED, MIN_BIN = 4, 12, 7, 3
LISTS = ("steiner", "parent", "bridge")


@pytest.fixture(scope="module")
def toy():
    net = P.read_network(NET)
    sets = _sets_cli.load_seed_sets(SEEDS)
    names = sorted(sets)
    members = [net.node_set(sets[n]) for n in names]
    assert net.n == 11 and names == ["first set", "second", "third"] and [len(m) for m in members] == [3, 2, 3]      # Z is no node
    return net, names, sets, members


def mirrored(net, units, max_add):
    """the mirror's table of `units` in the shape of SteinerEngine.trees' return"""
    want = M.table(net.rowptr, net.col, units)
    out = {f: want[f] for f in M.COUNTS}
    out["terminals"] = [np.asarray(u, np.int32) for u in units]
    out["steiner"] = [x[:max_add].astype(np.int32) for x in want["steiner"]]
    out["parent"] = [x[:max_add].astype(np.int32) for x in want["parent"]]
    out["bridge"] = [x.astype(np.int32) for x in want["bridge"]]
    out["truncated"] = want["n_steiner"] > max_add
    out["edges"] = [steiner.tree_edges(s, p, b) for s, p, b in zip(out["steiner"], out["parent"], out["bridge"])]
    return out


def same_trees(got, want):
    for f in M.COUNTS:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), f
    assert np.array_equal(got["truncated"], want["truncated"]) and got["edges"] == want["edges"]
    for key in LISTS + ("terminals",):
        assert len(got[key]) == len(want[key]) and all(a.dtype == np.int32 and np.array_equal(a, b) for a, b in zip(got[key], want[key])), key


def random_units(net, members, side):
    """the engine's random sets, read back: a list over sets of lists over samples (sample 0 the set) of node arrays, and the sizes"""
    mod = set_modules.ModuleEngine(net)
    try:
        nodes, sizes = mod.set_table(members, side, N_RANDOM, SEED, P.degree_bins(net.degree, MIN_BIN))
    finally:
        mod.close()
    nodes, sizes = nodes.cpu().numpy(), sizes.cpu().numpy()
    return [[nodes[i, r, :sizes[i, r]] for r in range(N_RANDOM + 1)] for i in range(len(members))], sizes


def test_engine_trees_and_table_equal_the_mirror(toy):
    net, names, sets, members = toy
    more = members + [net.node_set(set(g)) for g in ("IJKGH", "IK", "J", "EIK", "")]     # three Steiner nodes, a chain of two, one gene, no gene
    eng = steiner.SteinerEngine(net)
    try:
        got = eng.trees(more, max_add=MAX_ADD)
        same_trees(got, mirrored(net, more, MAX_ADD))
        assert got["n_steiner"].tolist() == [1, 0, 1, 3, 2, 0, 3, 0] and got["length"].tolist() == [4, 1, 4, 10, 3, 0, 5, 0]
        assert [net.names[v] for v in got["steiner"][3]] == ["A", "B", "C"] and got["n_comp"].tolist() == [1, 1, 1, 1, 1, 1, 1, 0]
        one = eng.trees(more, max_add=1)                                                   # the lists are cut, the counts are not
        same_trees(one, mirrored(net, more, 1))
        assert one["truncated"].tolist() == [False, False, False, True, True, False, True, False] and np.array_equal(one["n_edges"], got["n_edges"])
        res = eng.tree_table([sets[n] for n in names] + [{"J"}], 1, n_random=N_RANDOM, seed=SEED, min_bin_size=MIN_BIN, max_add=MAX_ADD)
        units, sizes = random_units(net, members + [net.node_set({"J"})], 1)
        assert np.array_equal(res["sizes"], sizes) and all(np.array_equal(units[i][0], m) for i, m in enumerate(members))
        flat = M.table(net.rowptr, net.col, [x for per_set in units for x in per_set])
        for f in ("n_comp", "length", "n_steiner"):
            assert res[f].dtype == np.int32 and np.array_equal(res[f], flat[f].reshape(4, N_RANDOM + 1)), f
        stats = steiner.table_stats([3, 2, 3, 1], sizes, *(flat[f].reshape(4, N_RANDOM + 1) for f in ("n_steiner", "length")))
        for key in ("steiner_stats", "length_stats"):
            for f in set_modules.STAT_FIELDS:
                assert np.array_equal(res[key][f], stats[key][f], equal_nan=True), (key, f)
        assert np.isnan(res["steiner_stats"]["p"][3]) and not np.isnan(res["steiner_stats"]["q"][:3]).any()
        assert np.array_equal(res["short"], stats["short"])
        assert len({tuple(x.tolist()) for x in units[0][1:]}) > 1                        # the null is not one set repeated
        same_trees(res["trees"], mirrored(net, members + [net.node_set({"J"})], MAX_ADD))
        none = eng.tree_table([sets[n] for n in names], 0, n_random=0, max_add=MAX_ADD)
        assert "steiner_stats" not in none and none["n_steiner"].shape == (3, 1)
        same_trees(none["trees"], mirrored(net, members, MAX_ADD))
        old = steiner.CHUNK_BYTES
        steiner.CHUNK_BYTES = 20 * 5                                                      # five units per call of the null, one of the lists: same integers
        try:
            again = eng.tree_table([sets[n] for n in names] + [{"J"}], 1, n_random=N_RANDOM, seed=SEED, min_bin_size=MIN_BIN, max_add=MAX_ADD)
        finally:
            steiner.CHUNK_BYTES = old
        assert all(np.array_equal(again[f], res[f]) for f in ("n_comp", "length", "n_steiner", "sizes"))
        same_trees(again["trees"], res["trees"])
    finally:
        eng.close()
    with pytest.raises(P.ProximityError, match="the engine is closed"):
        eng.trees(members)


def program(tmp_path, script, *args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *args], cwd=str(tmp_path), capture_output=True, text=True, env=env,
                          timeout=600)


def test_steiner_end_to_end(tmp_path, toy):
    net, names, sets, members = toy
    r = program(tmp_path, "steiner.py", "--network", NET, "--seeds", SEEDS, "--max-add", str(MAX_ADD), "--n-random", str(N_RANDOM), "--seed",
                str(SEED), "--min-bin-size", str(MIN_BIN), "--out", "e.tsv", "--nodes", "n.tsv", "--summary", "s.tsv", "--genes", "g.tsv",
                "--null", "null.npy")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().split("\n")[-1].startswith(f"steiner: 3 sets, max_add={MAX_ADD}, n_random={N_RANDOM}, LCC 11 nodes, 2 Steiner nodes, ")
    trees = mirrored(net, members, MAX_ADD)
    for name, writer in (("e.tsv", steiner_cli.write_edges), ("n.tsv", steiner_cli.write_nodes), ("g.tsv", steiner_cli.write_genes)):
        writer(tmp_path / ("want_" + name), names, net.names, trees)
        assert (tmp_path / name).read_text() == (tmp_path / ("want_" + name)).read_text(), name
    assert (tmp_path / "e.tsv").read_text().split("\n")[1:4] == ["first set\tA\tB\tpath", "first set\tA\tE\tbridge", "first set\tA\tG\tbridge"]
    assert "first set\tA\tsteiner\tB\t3" in (tmp_path / "n.tsv").read_text().split("\n")
    units, sizes = random_units(net, members, 1)                                          # --seeds draws the diseases' side
    flat = M.table(net.rowptr, net.col, [x for per_set in units for x in per_set])
    per = {f: flat[f].reshape(3, N_RANDOM + 1) for f in ("n_steiner", "length")}
    stats = steiner.table_stats([3, 2, 3], sizes, per["n_steiner"], per["length"])
    steiner_cli.write_summary(tmp_path / "want_s.tsv", names, dict(stats, n=np.array([3, 2, 3]), trees=trees))
    assert (tmp_path / "s.tsv").read_text() == (tmp_path / "want_s.tsv").read_text()
    null = np.load(tmp_path / "null.npy")
    assert null.dtype == np.int32 and np.array_equal(null, np.stack([per[f][:, 1:] for f in ("n_steiner", "length")], axis=1))
    # disease_modules.py takes the trees' nodes as a gene table
    r = program(tmp_path, "disease_modules.py", "--network", NET, "--diseases", "g.tsv", "--n-random", "8", "--min-bin-size", str(MIN_BIN), "--out", "dm.tsv")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    rows = [line.split("\t") for line in (tmp_path / "dm.tsv").read_text().split("\n")[1:-1]]
    assert [x[:3] for x in rows] == [["first.set", "4", "4"], ["second", "2", "2"], ["third", "4", "4"]]        # n and n.lcc: the trees are connected
    # without a null: the trees alone, NA in the summary
    r = program(tmp_path, "steiner.py", "--network", NET, "--seeds", SEEDS, "--set", "third", "--n-random", "0", "--out", "e0.tsv", "--summary", "s0.tsv")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert (tmp_path / "e0.tsv").read_text() == "set\ta\tb\tkind\nthird\tA\tD\tpath\nthird\tA\tF\tbridge\nthird\tA\tH\tbridge\n"
    assert (tmp_path / "s0.tsv").read_text().split("\n")[1].split("\t") == ["third", "3", "1", "1", "4", "3", "2", "1"] + ["NA"] * 11


def test_steiner_exit_statuses(tmp_path):
    r = program(tmp_path, "steiner.py", "--network", NET, "--seeds", SEEDS, "--max-add", "0")
    assert r.returncode == 2 and "--max-add 0 must be >= 1" in r.stderr and r.stdout == ""
    r = program(tmp_path, "steiner.py", "--network", NET, "--seeds", str(tmp_path / "missing.tsv"))
    assert r.returncode == 1 and r.stderr.startswith("steiner: ") and r.stderr.count("\n") == 1, r.stderr
    r = program(tmp_path, "steiner.py", "--network", NET, "--seeds", SEEDS, "--set", "fourth")
    assert r.returncode == 1 and "no set named 'fourth'" in r.stderr
    assert not os.path.exists(tmp_path / "edges.tsv")
