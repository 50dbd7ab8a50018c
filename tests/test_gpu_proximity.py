"""GPU: network proximity (csrc/proximity.hip) against scipy's BFS, the numpy mirror and the reference's 2016 tables."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import proximity_mirror as M  # noqa: E402
from gcn_drug_repurposing_amd import proximity as P  # noqa: E402

pytestmark = pytest.mark.gpu

TOY = [("A", "B"), ("A", "C"), ("A", "D"), ("A", "E"), ("A", "F"), ("A", "G"), ("A", "H"), ("B", "C"), ("B", "D"), ("B", "I"), ("B", "J"),
       ("C", "K"), ("D", "E"), ("D", "I"), ("E", "F")]
# |z_device - z_table| percentiles allowed, as multiples of the mirror's seed-to-seed percentiles recorded in the fixture
P50_FACTOR, P99_FACTOR = 1.25, 1.5


def _net(edges):
    names, src, dst, idx = [], [], [], {}
    for u, v in edges:
        for g in (u, v):
            if g not in idx:
                idx[g] = len(names)
                names.append(g)
        src += [idx[u], idx[v]]
        dst += [idx[v], idx[u]]
    return P.Network(src, dst, names)


@pytest.fixture(scope="module")
def fx():
    return M.Fixture()


@pytest.fixture(scope="module")
def eng(fx):
    e = P.ProximityEngine(fx.net)
    yield e
    e.close()


@pytest.fixture(scope="module")
def D(eng):
    return eng.distances().cpu().numpy()


@pytest.fixture(scope="module")
def full(fx, eng):
    """all five measures on all 18,564 table pairs at n_random = 1000, pairs given explicitly"""
    pairs = np.stack([fx.pair_drug, fx.pair_disease], 1)
    return eng.score(fx.drugs, fx.diseases, pairs=pairs, measures=M.MEASURES, n_random=1000, seed=452456)


def test_apsp_toy_equals_bfs():
    net = _net(TOY)
    e = P.ProximityEngine(net)
    got = e.distances().cpu().numpy()
    assert np.array_equal(got, M.bfs_rows(net.rowptr, net.col, np.arange(net.n)))
    assert e.diameter == int(got.max()) == 3
    e.close()


def test_apsp_fixture_equals_bfs(fx, eng, D):
    want = np.concatenate([M.bfs_rows(fx.net.rowptr, fx.net.col, np.arange(c, min(c + 1024, fx.net.n))) for c in range(0, fx.net.n, 1024)])
    assert np.array_equal(D, want)
    assert eng.diameter == int(want.max()) == 13


def test_apsp_refusals():
    path = [(str(i), str(i + 1)) for i in range(300)]                  # a 301-node path: 300 hops do not fit in a byte
    from gcn_drug_repurposing_amd import GssError
    with pytest.raises(GssError, match="255 or more hops"):
        P.ProximityEngine(_net(path))
    with pytest.raises(GssError, match="above the budget"):
        P.ProximityEngine(_net(TOY), max_bytes=100)


def test_random_sets_equal_mirror(fx, eng):
    bl = P.degree_bins(fx.net.degree, 100)
    nb = M.bin_of(bl, fx.net.n)
    for side, sets, pick in ((0, fx.drugs, [0, 5, 17, 100, 237]), (1, fx.diseases, [0, 9, 40, 77])):
        node_sets = [fx.net.node_set(s) for s in sets]
        nodes, sizes = eng.set_table(node_sets, side, 1000, 452456, bl)
        nodes, sizes = nodes.cpu().numpy(), sizes.cpu().numpy()
        for i in pick:
            assert sizes[i, 0] == len(node_sets[i]) and np.array_equal(nodes[i, 0, :sizes[i, 0]], node_sets[i])
            want = M.random_sets(node_sets[i], nb, bl, 452456, side, i, 1000)
            for k, w in enumerate(want):
                assert sizes[i, k + 1] == len(w), (side, i, k)
                assert np.array_equal(nodes[i, k + 1, :len(w)], w), (side, i, k)


def test_d_of_all_measures_equals_tables(fx, full):
    for m in M.MEASURES:
        want = fx.column(m, "d")
        got = full[m]["d"]
        err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
        assert err.max() <= 1e-9, (m, int(err.argmax()), got[err.argmax()], want[err.argmax()])
        assert np.array_equal(full[m]["n_from"], fx.z["n_target"]) and np.array_equal(full[m]["n_to"], fx.z["n_disease"])


def test_statistics_equal_mirror(fx, full, D):
    dist = lambda T, S: D[np.ix_(np.asarray(T), np.asarray(S))]  # noqa: E731
    bl = M.bins(fx.net.degree, 100)
    nb = M.bin_of(bl, fx.net.n)
    rng = np.random.RandomState(3)
    for q in rng.choice(len(fx.pair_drug), 8, replace=False):
        i, j = int(fx.pair_drug[q]), int(fx.pair_disease[q])
        res = M.proximity(dist, fx.net.node_set(fx.drugs[i]), fx.net.node_set(fx.diseases[j]), nb, bl, 452456, i, j, 1000)
        for m in M.MEASURES:
            d, mm, s, z, p = res[m]
            got = full[m]
            assert got["d"][q] == pytest.approx(d, rel=1e-12, abs=1e-12)
            assert got["m"][q] == pytest.approx(mm, rel=1e-12, abs=1e-12), (m, q)
            assert got["s"][q] == pytest.approx(s, rel=1e-12, abs=1e-12), (m, q)
            assert got["z"][q] == pytest.approx(z, rel=1e-12, abs=1e-11), (m, q)
            assert got["pval"][q] == pytest.approx(p, rel=1e-12, abs=1e-12), (m, q)


def test_z_within_monte_carlo_spread(fx, full):
    for m in M.MEASURES:
        dz = np.abs(full[m]["z"] - fx.column(m, "z"))
        sp = fx.z[f"spread_{m}"]
        p50, p99 = np.percentile(dz, [50, 99])
        assert p50 <= P50_FACTOR * sp[0], (m, p50, sp)
        assert p99 <= P99_FACTOR * sp[2], (m, p99, sp)
        assert np.max(np.abs(full[m]["pval"] - 0.5 * np.vectorize(__import__("math").erfc)(-full[m]["z"] / np.sqrt(2)))) < 1e-14


def test_auc_of_z_equals_tables(fx, full):
    from gcn_drug_repurposing_amd.consumer import roc_auc
    for m in M.MEASURES:
        want = roc_auc(fx.flag, -fx.column(m, "z"))
        got = roc_auc(fx.flag, -full[m]["z"])
        assert abs(got - want) <= 0.01, (m, got, want)
    assert abs(roc_auc(fx.flag, -fx.column("closest", "z")) - 0.6569) < 5e-5


def test_all_vs_all_and_reproducible(fx, eng, full):
    """pairs=None scores every drug against every disease (q = i * 78 + j) with the same numbers, bit for bit"""
    res = eng.score(fx.drugs, fx.diseases, measures=M.MEASURES, n_random=1000, seed=452456)
    q = fx.pair_drug * len(fx.diseases) + fx.pair_disease
    for m in M.MEASURES:
        for f in P.FIELDS:
            assert np.array_equal(res[m][f][q], full[m][f]), (m, f)
    other = eng.score(fx.drugs[:3], fx.diseases[:4], measures=("closest",), n_random=1000, seed=7)
    assert not np.array_equal(other["closest"]["z"], res["closest"]["z"][[i * 78 + j for i in range(3) for j in range(4)]])


def test_empty_sets_give_nan(fx, eng):
    res = eng.score([{"not-a-gene"}, fx.drugs[0]], [fx.diseases[0]], measures=("closest", "separation"), n_random=10)
    for m in ("closest", "separation"):
        assert np.all(np.isnan([res[m][f][0] for f in P.FIELDS])) and np.isfinite(res[m]["z"][1])
    assert res["closest"]["n_from"][0] == 0


def test_cli_end_to_end(fx, tmp_path):
    """the CLI on the fixture's data files: every d of the five tables, z within the spread"""
    with open(tmp_path / "net.sif", "w") as f:
        f.writelines(f"{u} 1 {v}\n" for u, v in fx.z["edges"])
    with open(tmp_path / "targets.pcl", "wb") as f:
        pickle.dump({n: s for n, s in zip(fx.drug_names, fx.drugs)}, f, protocol=0)
    with open(tmp_path / "genes.tsv", "w") as f:
        f.writelines(f"\t{n}\t" + "\t".join(sorted(s)) + "\n" for n, s in zip(fx.disease_names, fx.diseases))
    with open(tmp_path / "closest.dat", "w") as f:
        f.write("group disease d\n")
        f.writelines(f"{fx.drug_names[i]} {fx.disease_names[j]} 0\n" for i, j in zip(fx.pair_drug, fx.pair_disease))
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "proximity.py"), "--network", str(tmp_path / "net.sif"), "--drugs",
                        str(tmp_path / "targets.pcl"), "--diseases", str(tmp_path / "genes.tsv"), "--pairs", str(tmp_path / "closest.dat"),
                        "--measure", "all", "--out", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for m in M.MEASURES:
        lines = open(out / f"{m}.dat").read().split("\n")
        assert lines[0] == "group disease n.target n.disease d z pval"
        rows = [ln.split() for ln in lines[1:] if ln]
        assert len(rows) == len(fx.pair_drug)
        d = np.array([float(x[4]) for x in rows])
        z = np.array([float(x[5]) for x in rows])
        assert np.max(np.abs(d - fx.column(m, "d")) / np.maximum(1.0, np.abs(fx.column(m, "d")))) <= 1e-9, m
        assert np.percentile(np.abs(z - fx.column(m, "z")), 50) <= P50_FACTOR * fx.z[f"spread_{m}"][0], m
