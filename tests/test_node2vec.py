"""CPU: node2vec input embeddings (csrc/walk.hip, csrc/sgns.hip, node2vec.py).  The numpy mirror of the walk kernel samples the
reference walker's transition distribution (tests/golden/node2vec_msi_small.npz, made from multiscale/openne/walker.py's own alias
tables by tests/golden/make_node2vec_fixture.py); the product's host setup agrees with the mirror; bad arguments are refused by name
-- in Python before anything reaches the GPU, and by the C entry points themselves."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import node2vec_mirror as M  # noqa: E402

ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "node2vec_msi_small.npz")


@pytest.fixture(scope="module")
def fix():
    z = np.load(FIX)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", [0, 1])
def test_mirror_walk_frequencies_match_the_reference_walker(fix, case):
    g, adj, names = M.msi_small_graph()
    assert list(fix["names"]) == names
    p, q = float(fix["p"][case]), float(fix["q"][case])
    walks, lengths = M.walks(adj, 400, 16, p, q, seed=11)
    pv, impossible = M.transition_chi2(walks, lengths, fix, case)
    assert impossible == 0
    assert len(pv) > 300, len(pv)
    # Bonferroni over the states: every p-value above 1e-3 / (number of states)
    assert pv.min() > 1e-3 / len(pv), (pv.min(), len(pv))
    # and the p-values look uniform (a biased sampler piles them up near 0)
    assert np.mean(pv < 0.01) < 0.03, np.mean(pv < 0.01)


def test_mirror_walks_follow_edges_and_stop_at_sinks():
    import scipy.sparse as sp
    rng = np.random.RandomState(3)
    a = sp.random(60, 60, density=0.08, random_state=rng, format="csr")
    a.data = rng.rand(a.nnz) + 0.1
    a = a.tolil()
    a[5, :] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    walks, lengths = M.walks(a, 3, 12, 0.5, 2.0, seed=1)
    dense = a.toarray() > 0
    for w, ln in zip(walks, lengths):
        assert (w[ln:] == -1).all() and (w[:ln] >= 0).all()
        for k in range(1, ln):
            assert dense[w[k - 1], w[k]]
        if ln < 12:
            assert not dense[w[ln - 1]].any()
    # each iteration starts one walk at every node
    for r in range(3):
        assert sorted(walks[r * 60:(r + 1) * 60, 0]) == list(range(60))


def test_host_setup_agrees_with_the_mirror():
    from gcn_drug_repurposing_amd import node2vec as N
    assert (N.start_nodes(97, 3, 5) == M.start_nodes(97, 3, 5)).all()
    keys = np.arange(1000, dtype=np.uint64)
    assert (N._rng_key(7, 3, 2, keys, 9) == M.rng_key(7, 3, 2, keys, 9)).all()
    counts = np.random.RandomState(0).randint(1, 5000, size=300)
    counts[:3] = [900000, 1, 64]
    c1, k1 = N.sgns_tables(counts, 1e-3)
    c2, k2 = M.tables(counts, 1e-3)
    assert (c1 == c2).all() and c1[-1] == 2 ** 31 - 1
    assert (k1 == k2).all() and k1.max() == 2 ** 32 and k1[0] < 2 ** 31


def test_node2vec_refuses_bad_arguments_by_name():
    import scipy.sparse as sp

    from gcn_drug_repurposing_amd.node2vec import Node2vec
    a = sp.csr_matrix(np.array([[0, 1.0], [2.0, 0]]))
    names = ["a", "b"]
    with pytest.raises(ValueError, match="dw=True"):
        Node2vec((a, names), 4, 1, 128, dw=True)
    for kw, what in (({"p": 0.0}, "p=0.0"), ({"p": -1.0}, "p=-1.0"), ({"q": 0.0}, "q=0.0"), ({"q": float("nan")}, "q=nan")):
        with pytest.raises(ValueError, match=what):
            Node2vec((a, names), 4, 1, 128, **kw)
    with pytest.raises(ValueError, match="walk_length=0"):
        Node2vec((a, names), 0, 1, 128)
    with pytest.raises(ValueError, match="dim=100"):
        Node2vec((a, names), 4, 1, 100)
    for bad in (-1.0, float("inf"), float("nan")):
        b = sp.csr_matrix(np.array([[0, bad], [2.0, 0]]))
        with pytest.raises(ValueError, match="edge weight"):
            Node2vec((b, names), 4, 1, 128)


def test_cli_refuses_other_methods_by_name(tmp_path, capsys):
    from gcn_drug_repurposing_amd import node2vec_cli
    f = tmp_path / "g.edgelist"
    f.write_text("a b 1.0\nb a 2.0\n")
    for argv, what in ((["--method", "line"], "--method line"), (["--method", "deepWalk"], "--method deepWalk"),
                       (["--graph-format", "adjlist"], "--graph-format adjlist")):
        with pytest.raises(SystemExit):
            node2vec_cli.main(["--input", str(f), "--output", str(tmp_path / "o.txt")] + argv)
        assert what in capsys.readouterr().err
    with pytest.raises(ValueError, match="p=0.0"):
        node2vec_cli.main(["--input", str(f), "--output", str(tmp_path / "o.txt"), "--p", "0"])
    f.write_text("a b -1.0\nb a 2.0\n")
    with pytest.raises(ValueError, match="edge weight"):
        node2vec_cli.main(["--input", str(f), "--output", str(tmp_path / "o.txt"), "--weighted", "--directed"])


def test_cli_reads_the_edgelist_as_openne_does(tmp_path):
    """OpenNE Graph.read_edgelist: nodes in order of first appearance, weight 1.0 without --weighted, both directions without
    --directed, a repeated edge keeps its last weight"""
    from gcn_drug_repurposing_amd.node2vec_cli import read_graph
    f = tmp_path / "g.edgelist"
    f.write_text("x y 2.0\nz x 3.0\nx y 5.0\n")
    adj, names = read_graph(str(f), weighted=True, directed=True)
    assert names == ["x", "y", "z"]
    assert adj.toarray().tolist() == [[0, 5.0, 0], [0, 0, 0], [3.0, 0, 0]]
    adj, _ = read_graph(str(f), weighted=False, directed=False)
    assert adj.toarray().tolist() == [[0, 1.0, 1.0], [1.0, 0, 0], [1.0, 0, 0]]


def test_c_entry_points_refuse_bad_arguments_by_name():
    """the checks run before any device work, so they are testable without a GPU"""
    import ctypes as C

    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    lib = pkg.load()
    one = C.c_int32(0)
    P = C.addressof(one)
    for p, q, L, what in ((0.0, 1.0, 4, "p=0"), (1.0, -2.0, 4, "q=-2"), (1.0, float("inf"), 4, "q=inf"), (1.0, 1.0, 0, "walk_length=0")):
        rc = lib.gss_node2vec_walks(2, P, P, P, P, 2, P, L, p, q, 1, P, P, None)
        assert rc == -22
        assert what in lib.gss_last_error().decode()
    desc = pkg._lib.SgnsDesc(n=4, d=100, walk_length=8, window=5, negative=5, epochs=1, n_walks=4, walks=P, lengths=P, cum_table=P,
                             sample_int=P, cum_last=1, alpha=0.025, min_alpha=1e-4, seed=0, concurrency=1)
    assert lib.gss_sgns_epoch(desc, 0, P, P, None) == -22 and "dim=100" in lib.gss_last_error().decode()
    desc.d, desc.negative = 128, 0
    assert lib.gss_sgns_epoch(desc, 0, P, P, None) == -22 and "negative=0" in lib.gss_last_error().decode()
