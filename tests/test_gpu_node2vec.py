"""GPU: node2vec input embeddings.  The walk kernel reproduces the numpy mirror bit for bit and the reference walker's transition
distribution; serial SGNS (concurrency 1) matches the serial mirror; Hogwild SGNS (default concurrency) keeps the serial quality on a
planted partition; MSI graph -> node2vec -> train.py -> graph_embs.txt runs end to end and the embeddings rank drugs for indications."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import node2vec_mirror as M  # noqa: E402
from conftest import record_measured  # noqa: E402
from node2vec_cases import sinks_graph  # noqa: E402

PQ = [(1.0, 1.0), (0.25, 0.25), (4.0, 0.5)]
TOY_SIF = "A 1 B\nA 1 C\nA 1 D\nA 1 E\nA 1 F\nA 1 G\nA 1 H\nB 1 C\nB 1 D\nB 1 I\nB 1 J\nC 1 K\nD 1 E\nD 1 I\nE 1 F\n"
# SGNS, concurrency 1 vs the serial mirror after one epoch: both are fp32 with the same update order; only the dot products' summation
# order (a 64-lane xor reduction vs numpy) and fma contraction differ, a few ulp per update that the following updates carry along
SGNS_SERIAL_ABS = 2e-5


def toy_graph(tmp_path):
    import scipy.sparse as sp

    from gcn_drug_repurposing_amd.embio import read_edgelist
    f = tmp_path / "toy.sif"
    f.write_text(TOY_SIF)
    src, dst, w, names = read_edgelist(str(f))
    return sp.csr_matrix((w, (src, dst)), shape=(len(names), len(names)))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", ["toy_sif", "msi_small", "sinks"])
@pytest.mark.parametrize("pq", PQ)
def test_gpu_walks_equal_the_mirror_bit_for_bit(tmp_path, graph, pq):
    from gcn_drug_repurposing_amd.node2vec import random_walks
    adj = {"toy_sif": lambda: toy_graph(tmp_path), "msi_small": lambda: M.msi_small_graph()[1], "sinks": sinks_graph}[graph]()
    nw, L = 20, 16
    w, ln = random_walks(adj, nw, L, pq[0], pq[1], seed=123)
    w, ln = w.cpu().numpy(), ln.cpu().numpy()
    mw, ml = M.walks(adj, nw, L, pq[0], pq[1], seed=123)
    assert (ln == ml).all()
    assert (w == mw).all()
    w2, ln2 = random_walks(adj, nw, L, pq[0], pq[1], seed=123)
    assert (w2.cpu().numpy() == w).all() and (ln2.cpu().numpy() == ln).all()
    if graph == "sinks":
        assert (ln < L).any() and (ln == 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", [0, 1])
def test_gpu_walk_frequencies_match_the_reference_walker(case):
    from gcn_drug_repurposing_amd.node2vec import random_walks
    z = np.load(os.path.join(HERE, "golden", "node2vec_msi_small.npz"))
    fix = {k: z[k] for k in z.files}
    _, adj, _ = M.msi_small_graph()
    w, ln = random_walks(adj, 2000, 16, float(fix["p"][case]), float(fix["q"][case]), seed=5)
    pv, impossible = M.transition_chi2(w.cpu().numpy(), ln.cpu().numpy(), fix, case)
    assert impossible == 0
    assert len(pv) > 700, len(pv)          # of the 672 + 111 states of the graph
    assert pv.min() > 1e-3 / len(pv), (pv.min(), len(pv))
    assert np.mean(pv < 0.01) < 0.03, np.mean(pv < 0.01)


@pytest.mark.gpu
def test_gpu_sgns_serial_matches_the_mirror():
    import torch

    from gcn_drug_repurposing_amd.node2vec import random_walks, train_sgns
    _, adj, _ = M.msi_small_graph()
    n = adj.shape[0]
    w, ln = random_walks(adj, 4, 16, 0.25, 0.25, seed=3)
    # initialisation alone is bitwise the mirror's
    syn0, syn1 = train_sgns(w, ln, n, dim=128, epochs=1, seed=9, concurrency=1, window=0 + 10)
    torch.cuda.synchronize()
    i0, _ = M.init_vectors(n, 128, 9)
    ms0, ms1 = M.sgns(w.cpu().numpy(), ln.cpu().numpy(), n, 128, window=10, epochs=1, seed=9)
    err0 = np.abs(syn0.cpu().numpy() - ms0).max()
    err1 = np.abs(syn1.cpu().numpy() - ms1).max()
    moved = np.abs(ms0 - i0).max()
    record_measured("sgns_serial_vs_mirror", syn0_abs=err0, syn1_abs=err1, moved=moved)
    print(f"serial SGNS vs mirror: max|syn0 diff| {err0:.3e}, max|syn1neg diff| {err1:.3e}, max|update| {moved:.3e}")
    assert moved > 5e-3                                   # training did move the vectors
    assert np.abs(ms1).max() > 5e-3
    assert err0 < SGNS_SERIAL_ABS and err1 < SGNS_SERIAL_ABS
    # the same with the syn0 initialisation checked on its own (one value of an untouched row would do; compare all of them)
    from gcn_drug_repurposing_amd import _lib
    lib = _lib.load()
    a0 = torch.empty((n, 128), device="cuda")
    a1 = torch.empty((n, 128), device="cuda")
    _lib.check(lib.gss_sgns_init(n, 128, 9, _lib.ptr(a0), _lib.ptr(a1), _lib.current_stream()))
    assert (a0.cpu().numpy() == i0).all() and (a1.cpu().numpy() == 0).all()


def planted_partition(k=8, size=500, deg_in=12, deg_out=1, seed=0):
    import scipy.sparse as sp
    rng = np.random.RandomState(seed)
    n = k * size
    comm = np.repeat(np.arange(k), size)
    src = np.repeat(np.arange(n), deg_in + deg_out)
    dst = np.empty_like(src)
    for i in range(n):
        base = comm[i] * size
        inside = base + rng.choice(size, deg_in, replace=False)
        outside = rng.choice(np.flatnonzero(comm != comm[i]), deg_out, replace=False)
        dst[i * (deg_in + deg_out):(i + 1) * (deg_in + deg_out)] = np.concatenate([inside, outside])
    keep = src != dst
    a = sp.csr_matrix((np.ones(keep.sum()), (src[keep], dst[keep])), shape=(n, n))
    a = ((a + a.T) > 0).astype(np.float64)
    return a.tocsr(), comm


def knn_purity(emb, comm, k=10):
    e = emb / np.linalg.norm(emb, axis=1, keepdims=True)
    s = e @ e.T
    np.fill_diagonal(s, -np.inf)
    nn = np.argpartition(-s, k, axis=1)[:, :k]
    return float((comm[nn] == comm[:, None]).mean())


@pytest.mark.gpu
def test_gpu_hogwild_sgns_keeps_the_serial_quality():
    """default concurrency vs concurrency 1 on the same walks (the serial kernel is the mirror's order, checked above): the fraction of
    each node's 10 cosine-nearest neighbours in its own community"""
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd.node2vec import random_walks, train_sgns
    adj, comm = planted_partition()
    n = adj.shape[0]
    w, ln = random_walks(adj, 4, 16, 1.0, 1.0, seed=2)
    serial, _ = train_sgns(w, ln, n, dim=128, epochs=2, seed=4, concurrency=1)
    hog, _ = train_sgns(w, ln, n, dim=128, epochs=2, seed=4)
    ps, ph = knn_purity(serial.cpu().numpy(), comm), knn_purity(hog.cpu().numpy(), comm)
    conc = _lib.load().gss_sgns_default_concurrency()
    record_measured("sgns_hogwild_quality", serial=ps, hogwild=ph, concurrency=conc)
    print(f"planted partition 10-NN purity: serial {ps:.4f}, Hogwild ({conc} waves) {ph:.4f}")
    assert ps >= 0.9 and ph >= 0.9
    assert ph >= ps - 0.02


@pytest.mark.gpu
def test_gpu_msi_small_node2vec_to_train_py(tmp_path):
    from gcn_drug_repurposing_amd import embio, node2vec_cli, trainer
    from gcn_drug_repurposing_amd.node2vec import Node2vec
    g, adj, names = M.msi_small_graph()
    model = Node2vec(g, path_length=16, num_paths=64, dim=128, p=0.25, q=0.25, window=10, seed=1)
    emb_file = tmp_path / "msi_small.embs.txt"
    model.save_embeddings(str(emb_file))
    got_names, x = embio.read_embs(str(emb_file))
    assert got_names == names == list(model.vectors)
    assert x.shape == (len(names), 128) and open(emb_file).readline() == f"{len(names)} 128\n"
    assert np.array_equal(x.astype(np.float32), model.embeddings)
    out = tmp_path / "graph_embs.txt"
    trainer.main(["--emb-file", str(emb_file), "--num-layers", "2", "--hidden-units", "128", "--k", "5", "--epochs", "3",
                  "--lr", "0.0003", "--beta-percentile", "98", "--batch-size", "0", "--seed", "1", "--out", str(out)])
    ge = np.loadtxt(str(out))
    assert ge.shape == (len(names), 128)
    np.testing.assert_allclose(np.linalg.norm(ge, axis=1), 1.0, atol=1e-6)
    # the command line on the graph's weighted edgelist: rows in order of first appearance, as OpenNE's reader numbers them
    edges = tmp_path / "msi_small.edgelist"
    g.write_weighted_edgelist(str(edges))
    cli_out = tmp_path / "cli.embs.txt"
    node2vec_cli.main(["--input", str(edges), "--output", str(cli_out), "--graph-format", "edgelist", "--weighted", "--directed",
                       "--number-walks", "8", "--walk-length", "16", "--representation-size", "128", "--window-size", "10",
                       "--p", "0.25", "--q", "0.25", "--workers", "8", "--seed", "3"])
    cli_names, cx = embio.read_embs(str(cli_out))
    assert cli_names == embio.read_edgelist(str(edges))[3] and sorted(cli_names) == sorted(names)
    assert np.isfinite(cx).all()


@pytest.mark.gpu
def test_gpu_standin_node2vec_ranks_indications():
    """reference settings (predict_drug.py:40-46) on the real-layer stand-in: the mean drug-indication AUC of the node2vec embeddings
    is above 0.5 by at least 10 standard errors (standard deviation across indications / sqrt(count))"""
    from gcn_drug_repurposing_amd import consumer, synth
    from gcn_drug_repurposing_amd.node2vec import Node2vec
    adj, ntype, names = synth.whole_graph_standin()
    model = Node2vec((adj, names), path_length=16, num_paths=64, dim=128, p=0.25, q=0.25, window=10, seed=0)
    pos = synth.standin_drug_indications()
    drugs = [names[i] for i in np.flatnonzero(ntype == 0)]
    inds = [names[i] for i in np.flatnonzero(ntype == 1)]
    aucs, used = consumer.indication_aucs(model.embeddings, names, drugs, inds, pos)
    se = aucs.std() / np.sqrt(len(aucs))
    record_measured("node2vec_standin_auc", mean=aucs.mean(), median=np.median(aucs), se=se, count=len(aucs),
                    walks_s=model.timings["walks_s"], sgns_s=model.timings["sgns_s"])
    print(f"stand-in node2vec AUC over {len(aucs)} indications: mean {aucs.mean():.4f}, median {np.median(aucs):.4f}, se {se:.4f}; "
          f"walks {model.timings['walks_s']:.2f} s, SGNS {model.timings['sgns_s']:.2f} s")
    assert len(aucs) > 500
    assert aucs.mean() - 0.5 >= 10 * se
