"""CPU: what the trainer's --eval-config needs without a GPU -- the numpy mirror of csrc/scores.hip (embedding_scores_mirror.py) against
sklearn's arithmetic and the reference's recorded AUCs on tests/golden/evaluate_msi_small, the condition that makes that comparison
fair, the new train.py flags and their refusals (all before the GPU check), and evaluate.DeviceEvaluator's host-side checks with a stub
in place of the device calls.  The device side is in test_gpu_train_eval.py."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import embedding_scores_mirror as M  # noqa: E402
import evaluate_fixture as F  # noqa: E402

GAP = 1e-9      # a listed / unlisted pair of host scores closer than this, and not equal, could rank differently under another summation order


def fixture_lists(names):
    """the evaluator's lists on the fixture: (indications, drugs, rows, cols, pos_ptr, pos_col)"""
    from gcn_drug_repurposing_amd import consumer, evaluate
    from gcn_drug_repurposing_amd.msi import COMPONENTS, DRUG, INDICATION, MsiGraph
    g = MsiGraph().load({name: os.path.join(F.TABLES_DIR, name + ".tsv") for name, _, _ in COMPONENTS})
    drugs = [n for n in g.names if g.type[n] == DRUG]
    inds = [n for n in g.names if g.type[n] == INDICATION]
    idx = {n: i for i, n in enumerate(names)}
    ptr, col, _, _ = evaluate.label_rows(inds, drugs, consumer.read_drug_indication_tsv(os.path.join(F.D, "drug_indication_df.tsv")))
    return inds, drugs, [idx[i] for i in inds], [idx[d] for d in drugs], ptr, col


def fixture_embeddings(case):
    """-> (names, fp32 [111, 8]): the fixture's GCN embeddings (what a plan's tensor would hold) or its node2vec input"""
    from gcn_drug_repurposing_amd.embio import read_embs
    names, x = read_embs(os.path.join(F.D, "n2v.embs.txt"))
    if case == "gcn":
        x = np.loadtxt(os.path.join(F.D, "gcn.embs.txt"), ndmin=2)
    return names, np.asarray(x, dtype=np.float32)


def host_scores(x32, rows, cols, normalize):
    """evaluate.score_rows' arithmetic on the fp32 values: sklearn's normalisation, np.matmul per indication"""
    from gcn_drug_repurposing_amd.predict import normalize_like_sklearn
    x = x32.astype(np.float64)
    if normalize:
        x = normalize_like_sklearn(x)
    xd = x[cols]
    return np.asarray([np.matmul(xd, np.array(x[r])) for r in rows])


def close_pairs(scores, ptr, col):
    """per row: the number of (listed, unlisted) pairs of scores that are closer than GAP without being equal"""
    out = []
    for r in range(scores.shape[0]):
        mask = np.zeros(scores.shape[1], bool)
        mask[col[ptr[r]:ptr[r + 1]]] = True
        gap = np.abs(scores[r][mask][:, None] - scores[r][~mask][None, :])
        out.append(int(((gap != 0) & (gap <= GAP)).sum()))
    return out


@pytest.mark.parametrize("case, normalize", [("gcn", 1), ("node2vec", 0)])
def test_mirror_against_sklearn_and_the_recorded_aucs(case, normalize):
    names, x32 = fixture_embeddings(case)
    assert x32.shape == (111, 8)
    inds, drugs, rows, cols, ptr, col = fixture_lists(names)
    d = x32.shape[1]
    got = M.scores(x32, d, rows, cols, normalize)
    want = host_scores(x32, rows, cols, normalize)
    # the comparison is fair: no listed / unlisted pair is near enough for a correct summation order to swap it (an exact 0 is a true tie,
    # which both sides rank alike), so no indication needs exempting
    assert sum(close_pairs(want, ptr, col)) == 0
    # (d + 3) 2^-52 relative to the product of the two norms: d products and d - 1 sums of the dot, and the rounding of each operand's
    # normalisation (norm, square root, division).  Normalised rows have norm 1; the raw node2vec rows are compared by their own norms.
    v = x32.astype(np.float64)
    nr = np.sqrt((v * v).sum(axis=1))
    scale = np.ones_like(want) if normalize else nr[rows][:, None] * nr[cols][None, :]
    assert np.all(np.abs(got - want) <= (d + 3) * 2.0 ** -52 * scale), np.max(np.abs(got - want) / scale)
    auc, n_pos, n_neg = F.mirror_aucs(got, ptr, col)
    kept = [k for k in range(len(inds)) if n_pos[k] > 0 and n_neg[k] > 0]
    F.check_aucs([inds[k] for k in kept], auc[kept], case)


def test_mirror_properties():
    """what the kernel promises, on the mirror: sub-lists, swapped lists and padding change no bit; a zero row normalises to zero"""
    rng = np.random.RandomState(3)
    x = rng.randn(40, 80).astype(np.float32)
    x[5] = 0
    rows, cols = [3, 5, 3, 39, 0], [7, 5, 2, 2, 11, 38]
    for normalize in (0, 1):
        full = M.scores(x, 70, rows, cols, normalize)
        assert np.array_equal(M.scores(x, 70, cols, rows, normalize), full.T)
        assert np.array_equal(M.scores(x, 70, rows[1:3], cols[2:], normalize), full[1:3, 2:])
        assert np.all(full[1] == 0) and np.all(full[:, 1] == 0)
        padded = np.concatenate([x[:, :70], np.zeros((40, 10), np.float32)], axis=1)
        assert np.array_equal(M.scores(padded, 80, rows, cols, normalize), full)      # the plan's zero padding up to a multiple of 16
    assert abs(M.scores(x, 70, [4], [4], 1)[0, 0] - 1.0) <= 73 * 2.0 ** -52


# ---- the trainer's flags ---------------------------------------------------------------------------------------------------------------

BASE = ["--beta-percentile", "98", "--hidden-units", "8", "--num-layers", "2"]


def test_new_flags_parse():
    from gcn_drug_repurposing_amd import trainer
    a = trainer.parse_args(BASE + ["--emb-file", "x", "--eval-config", "c.json", "--eval-every", "3", "--eval-log", "log.tsv", "--keep-best",
                                   "best.txt", "--patience", "2"])
    assert (a.eval_config, a.eval_every, a.eval_log, a.keep_best, a.patience) == ("c.json", 3, "log.tsv", "best.txt", 2)
    a = trainer.parse_args(BASE + ["--emb-file", "x"])
    assert (a.eval_config, a.eval_every, a.eval_log, a.keep_best, a.patience) == (None, 1, None, None, None)


@pytest.mark.parametrize("extra, text", [
    (["--eval-config", "c.json", "--eval-every", "0"], "--eval-every 0 must be >= 1"),
    (["--eval-config", "c.json", "--patience", "-1"], "--patience -1 must be >= 1"),
    (["--eval-config", "c.json", "--patience", "0"], "--patience 0 must be >= 1"),
    (["--keep-best", "best.txt"], "--keep-best needs --eval-config"),
    (["--eval-log", "log.tsv"], "--eval-log needs --eval-config"),
    (["--patience", "2"], "--patience needs --eval-config"),
])
def test_flag_refusals(extra, text, capsys):
    from gcn_drug_repurposing_amd import trainer
    with pytest.raises(SystemExit) as e:
        trainer.main(BASE + ["--emb-file", "x"] + extra)
    assert e.value.code == 2 and text in capsys.readouterr().err


def _config(tmp_path, **networks):
    cfg = {"networks": {"protein_to_protein": os.path.join(F.TABLES_DIR, "protein_to_protein.tsv"),
                        "drug_to_indication": os.path.join(F.D, "drug_indication_df.tsv")}}
    cfg["networks"].update(networks)
    cfg["networks"] = {k: v for k, v in cfg["networks"].items() if v is not None}
    path = tmp_path / "eval.json"
    path.write_text(json.dumps(cfg))
    return str(path)


def _train(args):
    from gcn_drug_repurposing_amd import trainer
    return trainer.main(BASE + ["--adj-file", os.path.join(F.D, "eval.weighted.edgelist")] + args)


def _refused(args, capsys, monkeypatch):
    """the run ends with exit code 2 and a message, and it ends BEFORE the GPU check: looking for a GPU is an error here"""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU check ran before the refusal"))
    with pytest.raises(SystemExit) as e:
        _train(args)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_eval_config_refusals_come_before_the_gpu_check(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("GSS_FORCE_SHARDED", raising=False)
    emb = os.path.join(F.D, "n2v.embs.txt")
    err = _refused(["--emb-file", emb, "--eval-config", _config(tmp_path, drug_to_indication=None)], capsys, monkeypatch)
    assert "missing key networks.drug_to_indication" in err
    err = _refused(["--emb-file", emb, "--eval-config", _config(tmp_path, protein_to_protein=str(tmp_path / "protein_to_protein.tsv"))],
                   capsys, monkeypatch)
    assert "MSI table" in err and str(tmp_path) in err and "does not exist" in err
    err = _refused(["--emb-file", emb, "--eval-config", _config(tmp_path, drug_to_indication=str(tmp_path / "nope.tsv"))], capsys, monkeypatch)
    assert "networks.drug_to_indication" in err and "nope.tsv" in err
    # an --emb-file without one of the drug nodes
    inds, drugs, *_ = fixture_lists(fixture_embeddings("node2vec")[0])
    lines = open(emb).read().split("\n")
    short = tmp_path / "short.embs.txt"
    body = [l for l in lines[1:] if l and l.split(" ")[0] not in (drugs[2], inds[1])]
    short.write_text("\n".join([f"{len(body)} 8"] + body) + "\n")
    err = _refused(["--emb-file", str(short), "--eval-config", _config(tmp_path)], capsys, monkeypatch)
    assert f"node {drugs[2]!r} has no row (2 drug / indication nodes are missing)" in err and "short.embs.txt" in err
    monkeypatch.setenv("GSS_FORCE_SHARDED", "1")
    err = _refused(["--emb-file", emb, "--eval-config", _config(tmp_path)], capsys, monkeypatch)
    assert "--eval-config is not supported on sharded runs" in err and "GSS_FORCE_SHARDED=1" in err


def test_a_run_without_eval_config_prints_no_new_key(capsys):
    """the argument dump of a run without --eval-config is what it was before the flags existed"""
    from gcn_drug_repurposing_amd import trainer
    with pytest.raises(Exception, match="At least one of beta"):
        trainer.main(["--emb-file", "x"])
    out = capsys.readouterr().out
    assert "ngpus:None" in out and "eval" not in out and "keep_best" not in out and "patience" not in out


# ---- DeviceEvaluator on the host ---------------------------------------------------------------------------------------------------------

def _evaluator(monkeypatch, names, **kw):
    from gcn_drug_repurposing_amd import evaluate
    calls = []
    monkeypatch.setattr(evaluate.DeviceEvaluator, "upload", lambda self, device=None: calls.append(device))
    ev = evaluate.DeviceEvaluator(kw.pop("ppi", os.path.join(F.TABLES_DIR, "protein_to_protein.tsv")),
                                  kw.pop("labels", os.path.join(F.D, "drug_indication_df.tsv")), names, **kw)
    return ev, calls


def test_device_evaluator_lists_and_refusals(tmp_path, monkeypatch):
    from gcn_drug_repurposing_amd import evaluate
    from gcn_drug_repurposing_amd.predict import PredictError
    names, _ = fixture_embeddings("gcn")
    ev, calls = _evaluator(monkeypatch, names)
    inds, drugs, rows, cols, ptr, col = fixture_lists(names)
    assert calls == [None]                                                     # the upload comes last, once
    assert (ev.indications, ev.drugs) == (inds, drugs)
    assert ev.rows.tolist() == rows and ev.cols.tolist() == cols and ev.rows.dtype == ev.cols.dtype == np.int32
    assert np.array_equal(ev.pos_ptr, ptr) and np.array_equal(ev.pos_col, col) and ev.unknown_pairs == 0
    # every refusal comes before the device is touched
    for kw, text in [({"labels": str(tmp_path / "nope.tsv")}, "networks.drug_to_indication"),
                     ({"ppi": str(tmp_path / "protein_to_protein.tsv")}, "MSI table")]:
        with pytest.raises(PredictError, match=text):
            _evaluator(monkeypatch, names, **kw)
    gone = [n for n in names if n not in (drugs[0], drugs[3], inds[2])]
    with pytest.raises(PredictError) as e:
        _evaluator(monkeypatch, gone, source="some.embs.txt")
    first = [n for n in drugs + inds if n not in gone][0]
    assert str(e.value) == f"some.embs.txt: node {first!r} has no row (3 drug / indication nodes are missing)"
    empty = tmp_path / "labels.tsv"
    empty.write_text("drug\tdrug_name\tindication\tindication_name\n")
    with pytest.raises(PredictError, match="no indication has both a listed drug and an unlisted one"):
        _evaluator(monkeypatch, names, labels=str(empty))
    assert len(calls) == 1
    # tensors score() cannot take are refused by name, on the host
    import torch
    lib_calls = []
    monkeypatch.setattr(evaluate, "time", type("T", (), {"perf_counter": staticmethod(lambda: lib_calls.append(1) or 0.0)}))
    for emb, text in [(np.zeros((len(names), 8), np.float32), "not a torch tensor"),
                      (torch.zeros(len(names), 8, dtype=torch.float64), "dtype torch.float64"),
                      (torch.zeros(len(names) - 1, 8), f"the name list has {len(names)} rows"),
                      (torch.zeros(8), "shape"),
                      (torch.zeros(len(names), 8), "emb is on device cpu, not on the GPU")]:
        with pytest.raises(PredictError, match=text):
            ev.score(emb)
    assert lib_calls == []                                                     # score() stopped before its first device call
