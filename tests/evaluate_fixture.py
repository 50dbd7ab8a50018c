"""Shared by test_evaluate.py (CPU) and test_gpu_evaluate.py: the evaluate_msi_small fixture staged as an evaluate_auc.py config, the host
mirror of the device ROC-AUC (the kernel's own arithmetic in numpy), and the checks against the reference's recorded AUCs
(tests/golden/make_evaluate_fixture.py)."""
import json
import os
import pickle
import re
import shutil

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
D = os.path.join(HERE, "golden", "evaluate_msi_small")
TABLES_DIR = os.path.join(HERE, "golden", "msi_small")
LINE = re.compile(r"^median auc: (\S+), mean auc: (\S+)$")


def expected():
    return json.load(open(os.path.join(D, "expected.json")))


def mirror_aucs(scores, pos_ptr, pos_col):
    """csrc/auc.hip on the host: per row, the negatives' scores sorted (-0.0 folded into +0.0), 2U = sum over positives of
    searchsorted left + right, AUC = 2U / (2 P N); NaN and the counts where a row has one class"""
    scores = np.asarray(scores, dtype=np.float64)
    R, C = scores.shape
    auc = np.full(R, np.nan)
    n_pos = np.zeros(R, np.int32)
    n_neg = np.zeros(R, np.int32)
    for r in range(R):
        mask = np.zeros(C, bool)
        mask[pos_col[pos_ptr[r]:pos_ptr[r + 1]]] = True
        s = scores[r] + 0.0
        neg = np.sort(s[~mask])
        pos = s[mask]
        n_pos[r], n_neg[r] = len(pos), len(neg)
        if len(pos) and len(neg):
            twice = int(np.searchsorted(neg, pos, "left").sum()) + int(np.searchsorted(neg, pos, "right").sum())
            auc[r] = twice / (2.0 * len(pos) * len(neg))
    return auc, n_pos, n_neg


def config(tmp, method, labels=None, walk_length=16, number_walk=64, **over):
    cfg = {
        "name": "Drug Repurposing", "method": method,
        "eval": {"graph": os.path.join(str(tmp), "eval.weighted.edgelist")},
        "networks": {"protein_to_protein": os.path.join(TABLES_DIR, "protein_to_protein.tsv"),
                     "drug_to_indication": labels or os.path.join(D, "drug_indication_df.tsv")},
        "diffusion": {"eval_diffusion_embs_dir": os.path.join(str(tmp), "dp")},
        "node2vec": {"eval_emb_file_prefix": os.path.join(str(tmp), "eval_n2v"), "walk_length": walk_length, "number_walk": number_walk},
        "gcn": {"embs": "node2vec", "emb_file": os.path.join(D, "gcn.embs.txt")},
    }
    for k, v in over.items():
        cfg[k] = v
    return cfg


def stage(tmp, method, with_embs=True, walk_length=16, number_walk=64, name="config.json", **over):
    """config.json in tmp, the node2vec file staged under the config's eval prefix -> its path"""
    if with_embs:
        shutil.copy(os.path.join(D, "n2v.embs.txt"), os.path.join(str(tmp), f"eval_n2v_num_{number_walk}_len_{walk_length}.embs.txt"))
    path = os.path.join(str(tmp), name)
    with open(path, "w") as f:
        json.dump(config(tmp, method, walk_length=walk_length, number_walk=number_walk, **over), f)
    return path


def stage_reference_profiles(tmp):
    """an eval_diffusion_embs_dir with the reference's node order and the indications' profiles (drugs have none: the CPU test's
    stand-in for the device's profiles)"""
    z = np.load(os.path.join(D, "diffusion_profiles.npz"))
    d = os.path.join(str(tmp), "dp")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "node2idx.pkl"), "wb") as f:
        pickle.dump({str(n): i for i, n in enumerate(z["nodelist"])}, f)
    for i, p in zip(z["indications"], z["profiles"]):
        np.save(os.path.join(d, f"{i}_p_visit_array.npy"), p)


def check_aucs(indications, aucs, case):
    exp = expected()[case]
    assert list(indications) == exp["indications"]
    assert np.max(np.abs(np.asarray(aucs, np.float64) - np.asarray(exp["auc"]))) <= 1e-12, (list(aucs), exp["auc"])


def check_line(line, case):
    got, want = LINE.match(line), LINE.match(expected()[case]["line"])
    assert got and want, line
    for a, b in zip(got.groups(), want.groups()):
        assert abs(float(a) - float(b)) <= 1e-12, (line, expected()[case]["line"])


def read_per_indication(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "indication\tname\tpositives\tnegatives\tauc" and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    return [r[0] for r in rows], [float(r[4]) for r in rows], rows
