"""CPU: the predict_drug.py pieces that need no GPU -- the shortest-path mirror against networkx, node names, the config refusals, and
the table writer against the reference's own tables (tests/golden/predict_msi_small), with the mirror standing in for the device paths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import paths_mirror as M  # noqa: E402
import predict_fixture as F  # noqa: E402


def mirror_source(g, queries):
    from gcn_drug_repurposing_amd.predict import PathSource
    adj, names, _ = g.to_csr()
    t = np.array([names.index(q) for q in queries])
    dist, nxt = M.mirror_trees(adj, t)
    return PathSource(names, dist, nxt, t)


@pytest.mark.parametrize("pathway", [False, True])
def test_mirror_lengths_equal_networkx(pathway):
    nx = pytest.importorskip("networkx")
    g = F.msi_graph(pathway)
    adj, names, _ = g.to_csr()
    G = nx.DiGraph()
    G.add_nodes_from(names)
    G.add_edges_from((u, v) for u, s in g.adj.items() for v in s)
    targets = [names.index("NodeCovid"), names.index("C0000003"), 0]
    dist, nxt = M.mirror_trees(adj, targets)
    for qi, t in enumerate(targets):
        want = nx.single_target_shortest_path_length(G, names[t])
        want = dict(want)
        for v in range(len(names)):
            assert dist[qi, v] == want.get(names[v], 255)
            p = M.follow(dist[qi], nxt[qi], t, v)
            if p is not None:
                assert len(p) - 1 == dist[qi, v] and all(adj[a, b] != 0 for a, b in zip(p, p[1:]))
                succ = adj.indices[adj.indptr[v]:adj.indptr[v + 1]]
                if v != t:   # the tie rule: the smallest successor one hop closer
                    assert p[1] == min(u for u in succ if dist[qi, u] == dist[qi, v] - 1)


def test_node2name_equals_the_reference_map():
    g = F.msi_graph(False)
    exp = json.load(open(os.path.join(F.D, "node2name.json")))
    assert g.node2name == exp
    assert sum(v is None for v in exp.values()) >= 3     # blank cells of drug, protein and pathway rows stay missing
    # additive: names, node order and the CSR are those of the tables without the name columns
    assert len(g.names) == 111


def _cli(tmp_path, cfg=None, args=()):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = "-1"      # a refusal comes before anything touches the GPU
    cmd = [sys.executable, os.path.join(ROOT, "predict_drug.py")] + (["-c", cfg] if cfg else []) + list(args)
    return subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, env=env, timeout=300)


def _refused(tmp_path, message, method="gcn", args=(), **over):
    cfg = F.config(tmp_path, method, **over)
    path = tmp_path / "bad.json"
    path.write_text(json.dumps(cfg))
    r = _cli(tmp_path, str(path), args)
    assert r.returncode == 2, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert "Traceback" not in r.stderr
    assert not (tmp_path / "drugs.tsv").exists()


def test_refusals_by_name(tmp_path):
    covid = F.config(tmp_path, "gcn")["covid"]
    _refused(tmp_path, "add_permutation", covid=dict(covid, add_permutation=True))
    _refused(tmp_path, "covid.save_dir", covid=dict(covid, save_dir=str(tmp_path / "nope.tsv")))
    _refused(tmp_path, "method 'word2vec' is unknown", method="word2vec")
    _refused(tmp_path, "gcn.embs = 'sif'", gcn={"embs": "sif", "emb_file": "x"})
    _refused(tmp_path, "train.py --emb-file", gcn={"embs": "node2vec", "emb_file": str(tmp_path / "missing.embs.txt")})
    _refused(tmp_path, "--query 'NoSuchNode' is not a node", args=("--query", "NoSuchNode"))
    _refused(tmp_path, "no diffusion profile", method="diffusion", args=("--query", "117"))
    r = _cli(tmp_path, str(tmp_path / "absent.json"))
    assert r.returncode == 2 and "absent.json" in r.stderr


def test_config_keys_are_read(tmp_path):
    from gcn_drug_repurposing_amd.predict import Settings, load_config, parse_args
    a = parse_args(["-c", "x.json", "-s", "ignored", "-r", "r", "-d", "0", "--query", "A", "--query", "B"])
    assert a.config == "x.json" and a.query == ["A", "B"]
    s = Settings(load_config(F.stage(tmp_path, "gcn")))
    assert s.method == "gcn" and s.topk == F.TOPK and s.queries == ["NodeCovid"] and s.add_pathway
    assert s.n2v_file == os.path.join(str(tmp_path), "n2v_num_64_len_16.embs.txt")
    assert s.tables()["indication_to_protein"].endswith("indication_to_protein.tsv")


@pytest.mark.parametrize("case", ["node2vec", "gcn", "diffusion"])
def test_writer_reproduces_the_reference_tables(tmp_path, case, monkeypatch):
    from gcn_drug_repurposing_amd import predict
    monkeypatch.chdir(tmp_path)
    cfg = F.stage(tmp_path, case)
    if case == "diffusion":
        F.stage_reference_profile(tmp_path)
    s = predict.Settings(predict.load_config(cfg))
    out = predict.run(s, "proteins.tsv" if case == "gcn" else None, path_source=mirror_source)
    F.check_drug_table(tmp_path / "drugs.tsv", case)
    if case == "gcn":
        F.check_protein_table(tmp_path / "proteins.tsv")
        assert out["NodeCovid"] == ("drugs.tsv", "proteins.tsv")
    assert (tmp_path / "whole_graph.weighted.edgelist").exists()


def test_two_queries_name_their_outputs(tmp_path, monkeypatch):
    from gcn_drug_repurposing_amd import predict
    monkeypatch.chdir(tmp_path)
    s = predict.Settings(predict.load_config(F.stage(tmp_path, "gcn")), ["NodeCovid", "C0000003"])
    out = predict.run(s, "proteins.tsv", path_source=mirror_source)
    assert out == {"NodeCovid": ("drugs.NodeCovid.tsv", "proteins.NodeCovid.tsv"), "C0000003": ("drugs.C0000003.tsv", "proteins.C0000003.tsv")}
    F.check_drug_table(tmp_path / "drugs.NodeCovid.tsv", "gcn")
    assert (tmp_path / "drugs.C0000003.tsv").read_text().splitlines()[0] == "\t".join(predict.DRUG_HEADER)
