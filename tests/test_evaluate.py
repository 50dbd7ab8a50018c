"""CPU: the evaluate_auc.py pieces that need no GPU -- the unweighted eval graph, the config refusals, score and label assembly with the
host mirror of the ROC-AUC kernel against the reference's recorded AUCs (tests/golden/evaluate_msi_small), the skip rules and the stdout
line."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_fixture as F  # noqa: E402


def _run(tmp_path, method, **kw):
    from gcn_drug_repurposing_amd import evaluate
    s = evaluate.Settings(evaluate.load_config(F.stage(tmp_path, method, **{k: v for k, v in kw.items() if k == "labels"})))
    err = io.StringIO()
    res = evaluate.run(s, auc_source=F.mirror_aucs, err=err, per_indication=kw.get("per_indication"))
    return res, err.getvalue()


def test_eval_graph_is_the_references_unweighted_edgelist(tmp_path):
    _run(tmp_path, "node2vec")
    got = (tmp_path / "eval.weighted.edgelist").read_bytes()
    assert got == open(os.path.join(F.D, "eval.weighted.edgelist"), "rb").read()
    assert all(len(line.split()) == 2 for line in got.decode().splitlines())
    from gcn_drug_repurposing_amd.msi import MsiGraph
    g = MsiGraph()
    g._add_edge("a", "b")
    g.write_unweighted_edgelist(str(tmp_path / "one.edgelist"))
    assert (tmp_path / "one.edgelist").read_bytes() == b"a b\nb a\n"      # networkx 3.4 on one undirected edge without a weight


@pytest.mark.parametrize("case", ["diffusion", "node2vec", "gcn"])
def test_mirror_reproduces_the_reference_aucs(tmp_path, case):
    if case == "diffusion":
        F.stage_reference_profiles(tmp_path)
    res, err = _run(tmp_path, case, per_indication=str(tmp_path / "per.tsv"))
    assert not any(res.skipped.values()) and res.unknown_pairs == 0 and "evaluate_auc:" not in err
    F.check_aucs(res.indications, res.auc, case)
    F.check_line(res.line, case)
    inds, aucs, rows = F.read_per_indication(tmp_path / "per.tsv")
    F.check_aucs(inds, aucs, case)
    assert all(r[1] == f"n_{r[0]}" for r in rows)                                 # the MSI's node names
    assert [int(r[2]) + int(r[3]) for r in rows] == [12] * len(rows)             # every drug node is a candidate


def test_stdout_line_has_the_reference_format():
    from gcn_drug_repurposing_amd.evaluate import format_line
    assert format_line([0.5, 0.75, 1.0]) == "median auc: 0.75, mean auc: 0.75"
    a = np.array([0.1, 0.2, 0.4])
    assert format_line(a) == f"median auc: {np.median(a)}, mean auc: {a.mean()}" == "median auc: 0.2, mean auc: 0.23333333333333336"


def test_skip_rules_and_their_report(tmp_path):
    from gcn_drug_repurposing_amd import consumer
    from gcn_drug_repurposing_amd.msi import MsiGraph
    g = MsiGraph().load({t: os.path.join(F.TABLES_DIR, t + ".tsv") for t in ("drug_to_protein", "indication_to_protein", "protein_to_protein",
                                                                           "protein_to_functional_pathway",
                                                                           "functional_pathway_to_functional_pathway")})
    drugs = [n for n in g.names if g.type[n] == "drug"]
    inds = [n for n in g.names if g.type[n] == "indication"]
    rows = [(drugs[0], inds[1]), ("DB99999", inds[2]), (drugs[1], inds[4]), ("DB99998", inds[4]), (drugs[2], inds[5])]
    rows += [(d, inds[3]) for d in drugs]                                          # every drug listed: one class
    labels = tmp_path / "labels.tsv"
    labels.write_text("drug\tdrug_name\tindication\tindication_name\n" + "".join(f"{d}\tx\t{i}\ty\n" for d, i in rows))
    res, err = _run(tmp_path, "gcn", labels=str(labels))
    assert res.skipped == {"no_row": [inds[0]] + inds[6:], "no_known_drug": [inds[2]], "all_positive": [inds[3]]}
    kept = [res.indications[k] for k in res.kept]
    assert kept == [inds[1], inds[4], inds[5]]
    k4 = res.indications.index(inds[4])
    assert (res.n_pos[k4], res.n_neg[k4]) == (1, len(drugs) - 1)                  # the unknown drug is left out
    n_skip = len(inds) - 3
    assert f"skipped {n_skip} of {len(inds)} indications: {len(inds) - 5} without a row" in err, err
    assert "1 whose listed drugs are not drug nodes of the graph, 1 with every drug listed" in err, err
    assert "2 listed (drug, indication) pairs name a drug that is not a drug node" in err, err
    from gcn_drug_repurposing_amd.embio import read_embs
    names, _ = read_embs(os.path.join(F.D, "n2v.embs.txt"))
    _, used = consumer.indication_aucs(np.loadtxt(os.path.join(F.D, "gcn.embs.txt")), names, drugs, inds,
                                       consumer.read_drug_indication_tsv(str(labels)))
    assert used == kept                                                            # consumer.indication_aucs' skip rules


def _cli(tmp_path, cfg):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = "-1"      # a refusal comes before anything touches the GPU
    return subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_auc.py"), "-c", cfg, "-s", "x", "-d", "0"], cwd=str(tmp_path),
                          capture_output=True, text=True, env=env, timeout=300)


def _refused(tmp_path, message, method="gcn", **over):
    cfg = F.config(tmp_path, method, **over)
    path = tmp_path / "bad.json"
    path.write_text(json.dumps(cfg))
    r = _cli(tmp_path, str(path))
    assert r.returncode == 2, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert "Traceback" not in r.stderr and r.stdout == ""


def test_refusals_by_name(tmp_path):
    _refused(tmp_path, "method 'word2vec' is unknown", method="word2vec")
    _refused(tmp_path, "gcn.embs = 'sif' is not supported", gcn={"embs": "sif", "emb_file": "x"})
    _refused(tmp_path, "config: missing key gcn.emb_file", gcn={"embs": "node2vec"})
    _refused(tmp_path, "train.py --emb-file", gcn={"embs": "node2vec", "emb_file": str(tmp_path / "missing.embs.txt")})
    _refused(tmp_path, "networks.drug_to_indication", labels=str(tmp_path / "absent.tsv"))
    short = tmp_path / "short_gcn.txt"
    np.savetxt(short, np.loadtxt(os.path.join(F.D, "gcn.embs.txt"))[:-3])
    F.stage(tmp_path, "gcn")
    _refused(tmp_path, "108 rows, but the node2vec file has 111 nodes", gcn={"embs": "node2vec", "emb_file": str(short)})
    r = _cli(tmp_path, str(tmp_path / "absent.json"))
    assert r.returncode == 2 and "absent.json" in r.stderr
