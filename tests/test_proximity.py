"""CPU: the network proximity host side (loaders, LCC, degree bins, CLI refusals) and its numpy mirror against the 2016 tables."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import proximity_mirror as M  # noqa: E402
from gcn_drug_repurposing_amd import proximity as P  # noqa: E402

TOY = [("A", "B"), ("A", "C"), ("A", "D"), ("A", "E"), ("A", "F"), ("A", "G"), ("A", "H"), ("B", "C"), ("B", "D"), ("B", "I"), ("B", "J"),
       ("C", "K"), ("D", "E"), ("D", "I"), ("E", "F")]


def toy_network(extra=()):
    names, src, dst = [], [], []
    idx = {}
    for u, v in list(TOY) + list(extra):
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


def test_disease_key_and_loaders(tmp_path, fx):
    assert P.disease_key("Kidney Diseases") == "kidney.diseases"
    assert P.disease_key("Lupus Erythematosus, Systemic") == "lupus.erythematosus.systemic"
    assert P.disease_key("Arthritis, Juvenile Rheumatoid") == "arthritis.juvenile.rheumatoid"
    tsv = tmp_path / "d.tsv"
    tsv.write_text("\tKidney Diseases\t10\t20\n\tHIV Infections\t30\n")
    assert P.load_disease_genes(str(tsv)) == {"kidney.diseases": {"10", "20"}, "hiv.infections": {"30"}}
    pcl = tmp_path / "t.pcl"
    with open(pcl, "wb") as f:
        pickle.dump({"DB1": {"1", "2"}, "DB2": {"3"}}, f, protocol=0)
    assert b"__builtin__\nset" in pcl.read_bytes()          # the reference's Python 2 form
    assert P.load_drug_targets(str(pcl)) == {"DB1": {"1", "2"}, "DB2": {"3"}}
    assert len(fx.disease_names) == 78 and len(fx.drug_names) == 238


def test_restricted_unpickler_rejects_other_globals(tmp_path):
    for payload in (b"cos\nsystem\n(S'true'\ntR.", b"cbuiltins\neval\n(S'1'\ntR.", b"c__builtin__\nfrozenset\n((lp0\nS'1'\natR."):
        p = tmp_path / "evil.pcl"
        p.write_bytes(payload)
        with pytest.raises(pickle.UnpicklingError, match="not allowed"):
            P.load_drug_targets(str(p))


def test_lcc_and_set_sizes(fx):
    assert fx.net.n_total == 13460 and fx.net.n == 13329
    assert np.all(np.diff(fx.net.rowptr) > 0)
    rowlen = np.diff(fx.net.rowptr)
    rows = np.repeat(np.arange(fx.net.n), rowlen)
    assert not np.any(rows == fx.net.col)                               # no self loops in the CSR
    nt = np.array([len(fx.net.node_set(s)) for s in fx.drugs])[fx.pair_drug]
    ns = np.array([len(fx.net.node_set(s)) for s in fx.diseases])[fx.pair_disease]
    assert np.array_equal(nt, fx.z["n_target"]) and np.array_equal(ns, fx.z["n_disease"])


def test_degree_bins_small_graph():
    net = toy_network(extra=[("K", "K")])                               # a self loop adds 2 to K's degree
    deg = dict(zip(net.names, net.degree))
    assert deg == {"A": 7, "B": 5, "C": 3, "D": 4, "E": 3, "F": 2, "G": 1, "H": 1, "I": 2, "J": 1, "K": 3}
    try:
        import networkx as nx
        g = nx.Graph()
        g.add_edges_from(list(TOY) + [("K", "K")])
        assert deg == dict(g.degree())
    except ImportError:
        pass
    name = lambda b: sorted(net.names[i] for i in b)  # noqa: E731
    # degrees 1:{G,H,J} 2:{F,I} 3:{C,E,K} 4:{D} 5:{B} 7:{A}
    assert [name(b) for b in P.degree_bins(net.degree, 3)] == [["G", "H", "J"], ["C", "E", "F", "I", "K"], ["A", "B", "D"]]
    assert [name(b) for b in P.degree_bins(net.degree, 4)] == [["F", "G", "H", "I", "J"], ["A", "B", "C", "D", "E", "K"]]
    assert [name(b) for b in P.degree_bins(net.degree, 100)] == [sorted(net.names)]
    for size in (1, 2, 3, 4, 5, 100):
        assert [list(b) for b in P.degree_bins(net.degree, size)] == [list(b) for b in M.bins(net.degree, size)]


def test_bins_on_the_2016_network(fx):
    bl = P.degree_bins(fx.net.degree, 100)
    assert [list(b) for b in bl] == [list(b) for b in M.bins(fx.net.degree, 100)]
    assert all(len(b) >= 100 for b in bl) and sum(len(b) for b in bl) == fx.net.n
    top = [int(fx.net.degree[b].min()) for b in bl]
    assert top == sorted(top)


def test_rng_keys_equal_counter_rng_h(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler is needed"
    src = tmp_path / "k.cpp"
    src.write_text('#define __host__\n#define __device__\n#define __forceinline__ inline\n#include "counter_rng.h"\n#include <stdio.h>\n'
                   "int main() { unsigned long long s[3] = {452456ull, 1ull, 0xFFFFFFFFFFFFFFFFull};\n"
                   "  for (int i = 0; i < 3; ++i) for (unsigned long long tag = 7; tag <= 8; ++tag) for (unsigned long long k = 0; k < 3; ++k)\n"
                   "    printf(\"%llu\\n\", (unsigned long long)gss::rng_key(s[i], tag, 17 + k, 999 - k, k * 32 + 20));\n}\n")
    exe = tmp_path / "k"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [int(M.rng_key(s, tag, 17 + k, 999 - k, k * 32 + 20)) for s in (452456, 1, 2 ** 64 - 1) for tag in (7, 8) for k in range(3)]
    assert got == want


def test_mirror_random_sets_properties(fx):
    bl = M.bins(fx.net.degree, 100)
    nb = M.bin_of(bl, fx.net.n)
    S = fx.net.node_set(fx.diseases[0])
    a = M.random_sets(S, nb, bl, 452456, 1, 0, 50)
    b = M.random_sets(S, nb, bl, 452456, 1, 0, 50)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(len(x) <= len(S) and np.all(np.diff(x) > 0) for x in a)
    assert any(len(x) == len(S) for x in a)
    c = M.random_sets(S, nb, bl, 452456, 0, 0, 50)                      # the other side's tag draws other sets
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    # every draw comes from the member's degree bin: the multiset of bins is kept when no draw collapsed
    full = [x for x in a if len(x) == len(S)]
    assert sorted(nb[S]) == sorted(nb[full[0]])


def test_mirror_d_equals_tables(fx):
    """d of all five measures on all 18,564 pairs from the mirror equals the tables' 12-digit text"""
    fs = [fx.net.node_set(s) for s in fx.drugs]
    ts = [fx.net.node_set(s) for s in fx.diseases]
    dist = M.RowCache(fx.net.rowptr, fx.net.col, rows=np.unique(np.concatenate(fs + ts)))
    got = {m: np.empty(len(fx.pair_drug)) for m in M.MEASURES}
    for q, (i, j) in enumerate(zip(fx.pair_drug, fx.pair_disease)):
        for m, v in M.measures(dist, fs[i], ts[j]).items():
            got[m][q] = v
    for m in M.MEASURES:
        want = fx.column(m, "d")
        assert np.all(np.isfinite(want))
        err = np.abs(got[m] - want) / np.maximum(1.0, np.abs(want))
        assert err.max() <= 1e-9, (m, int(err.argmax()), err.max())


def test_stats_toolbox_convention():
    m, s, z, p = M.stats(2.0, [1.0, 2.0, 3.0, 2.0])
    assert m == 2.0 and abs(s - np.sqrt(0.5)) < 1e-15 and z == 0.0 and p == 0.5
    assert M.stats(1.0, [2.0, 2.0])[2] == 0.0                          # s = 0 gives z = 0


def _cli(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "proximity.py")] + args, capture_output=True, text=True, cwd=ROOT)


def test_cli_refusals(tmp_path):
    sif = tmp_path / "n.sif"
    sif.write_text("".join(f"{u} 1 {v}\n" for u, v in TOY))
    pcl = tmp_path / "t.pcl"
    with open(pcl, "wb") as f:
        pickle.dump({"DB1": {"A", "B"}}, f, protocol=0)
    tsv = tmp_path / "d.tsv"
    tsv.write_text("\tSome Disease\tC\tD\n")
    base = ["--network", str(sif), "--drugs", str(pcl), "--diseases", str(tsv), "--out", str(tmp_path / "o")]
    r = _cli(base + ["--measure", "nearest"])
    assert r.returncode != 0 and "--measure nearest" in r.stderr
    r = _cli(base + ["--n-random", "1"])
    assert r.returncode != 0 and "--n-random 1" in r.stderr
    r = _cli(base + ["--min-bin-size", "0"])
    assert r.returncode != 0 and "--min-bin-size 0" in r.stderr
    dat = tmp_path / "pairs.dat"
    dat.write_text("group disease d\nDB9 some.disease 1\nDB1 other.disease 2\n")
    r = _cli(base + ["--pairs", str(dat)])
    assert r.returncode != 0 and "DB9" in r.stderr and "other.disease" in r.stderr
    assert P.read_table_pairs(str(dat)) == [("DB9", "some.disease"), ("DB1", "other.disease")]
