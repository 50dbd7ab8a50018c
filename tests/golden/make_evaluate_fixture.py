#!/usr/bin/env python3
"""Golden fixture for evaluate_auc.py on the msi_small tables: a drug -> indication label table, the REFERENCE's own outputs, and seeded
embedding files.  evaluate_auc.py is imported with sys.modules stubs for multiscale_interactome.* (pointed at the reference's multiscale/
packages), utils stubbed, and np.float = float.

* diffusion: the reference's evaluate_auc.main as written, in a temporary working directory holding the tables as data/*.tsv.  Its
  DiffusionProfiles pickles the graph into the profile directory before creating it, so calculate_diffusion_profiles is wrapped to
  create the directory first; roc_auc_score is wrapped to record each indication's AUC.  Recorded: the eval graph's text, the
  per-indication AUCs, the printed line, and the indications' profiles (for the CPU test's staged profile directory).
* node2vec / gcn: the reference's graph_embedding arithmetic per indication (its raw rows, or sklearn-normalised GCN rows, in
  embedding-file order; np.matmul with the indication's row), sklearn's roc_auc_score against DrugToIndication's drugs.  The main
  function's embedding branches end in a NameError, so this is the evident intent.  Every row's distinct scores are asserted to lie
  more than 1e-9 apart, so rounding cannot reorder a pair.
The label table is the reference's data/drug_indication_df.tsv restricted to msi_small's nodes plus seeded pairs, so every indication
node has a listed drug and the reference does not crash.  Run in the build container only:  python tests/golden/make_evaluate_fixture.py"""
import csv
import io
import json
import multiprocessing
import os
import shutil
import sys
import tempfile
import types
from contextlib import redirect_stdout

import numpy as np

REF = os.environ.get("GSS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msi_small")
OUT = os.path.join(HERE, "evaluate_msi_small")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "multiscale"))
sys.path.insert(0, REF)

TABLES = ("drug_to_protein", "indication_to_protein", "protein_to_protein", "protein_to_functional_pathway",
          "functional_pathway_to_functional_pathway")
DIM = 8
WALK, NUM = 16, 64


def compat():
    """the reference targets networkx 2.x / scipy < 1.8 (as in make_diffusion_fixture.py)"""
    import networkx as nx
    import scipy
    import scipy.sparse as sp
    if not hasattr(nx, "to_scipy_sparse_matrix"):
        nx.to_scipy_sparse_matrix = lambda g, nodelist=None, weight="weight", dtype=None: sp.csr_matrix(
            nx.to_scipy_sparse_array(g, nodelist=nodelist, weight=weight, dtype=dtype, format="csr"))
    for name in ("array", "repeat", "where", "absolute"):
        if not hasattr(scipy, name):
            setattr(scipy, name, getattr(np, name))


def stub_modules():
    compat()
    from msi import msi as ref_msi
    from msi import node_to_node as ref_n2n
    from diff_prof import diffusion_profiles as ref_dp
    np.float = float
    mods = {"multiscale_interactome": types.ModuleType("multiscale_interactome"),
            "multiscale_interactome.openne": types.ModuleType("multiscale_interactome.openne"),
            "multiscale_interactome.openne.node2vec": types.ModuleType("n2v"),
            "multiscale_interactome.openne.graph": types.ModuleType("graph"),
            "multiscale_interactome.msi": types.ModuleType("multiscale_interactome.msi"),
            "multiscale_interactome.msi.msi": ref_msi,
            "multiscale_interactome.msi.node_to_node": ref_n2n,
            "multiscale_interactome.diff_prof": types.ModuleType("multiscale_interactome.diff_prof"),
            "multiscale_interactome.diff_prof.diffusion_profiles": ref_dp,
            "utils": types.ModuleType("utils")}
    mods["multiscale_interactome.openne.node2vec"].Node2vec = None
    mods["multiscale_interactome.openne.graph"].Graph = None
    for k in ("query_uniprot2data", "make_SARSCOV2_PPI"):
        setattr(mods["utils"], k, None)
    sys.modules.update(mods)
    import evaluate_auc
    return evaluate_auc, ref_msi, ref_n2n, ref_dp


def label_table(drugs, inds):
    """the reference's pairs among msi_small's nodes, plus 1-3 seeded drugs for every indication without one"""
    with open(os.path.join(REF, "data", "drug_indication_df.tsv"), newline="") as f:
        rows = list(csv.DictReader(f, delimiter="\t"))
    keep = [r for r in rows if r["drug"] in drugs and r["indication"] in inds]
    dname = {r["drug"]: r["drug_name"] for r in rows if r["drug"] in drugs}
    iname = {r["indication"]: r["indication_name"] for r in rows if r["indication"] in inds}
    out = [(r["drug"], r["drug_name"], r["indication"], r["indication_name"]) for r in keep]
    have = {r[2] for r in out}
    rng = np.random.RandomState(11)
    for i in sorted(inds):
        if i in have:
            continue
        for d in sorted(rng.choice(sorted(drugs), rng.randint(1, 4), replace=False)):
            out.append((d, dname.get(d, f"n_{d}"), i, iname.get(i, f"n_{i}")))
    with open(os.path.join(OUT, "drug_indication_df.tsv"), "w") as f:
        f.write("drug\tdrug_name\tindication\tindication_name\n")
        f.writelines("\t".join(r) + "\n" for r in out)
    return len(keep), len(out)


def min_gap(v):
    u = np.unique(v)
    return float(np.min(np.diff(u))) if len(u) > 1 else np.inf


def main():
    from sklearn.metrics import roc_auc_score
    from sklearn.preprocessing import normalize
    os.makedirs(OUT, exist_ok=True)
    ev, ref_msi, ref_n2n, ref_dp = stub_modules()
    calc = ref_dp.DiffusionProfiles.calculate_diffusion_profiles

    def calc_in_dir(self, msi):
        os.makedirs(self.save_load_file_path, exist_ok=True)
        return calc(self, msi)
    ref_dp.DiffusionProfiles.calculate_diffusion_profiles = calc_in_dir
    multiprocessing.cpu_count = lambda: 4        # num_cores = 2 worker processes
    recorded = []

    def recording_auc(y, s):
        recorded.append(float(roc_auc_score(y, s)))
        return recorded[-1]
    ev.roc_auc_score = recording_auc
    expected = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "data"))
        for t in TABLES:
            shutil.copy(os.path.join(SRC, t + ".tsv"), os.path.join(tmp, "data", t + ".tsv"))
        os.chdir(tmp)
        try:
            msi = ref_msi.MSI()
            msi.load()
            drugs = [n for n in msi.nodelist if msi.graph.nodes[n]["type"] == "drug"]
            inds = [n for n in msi.nodelist if msi.graph.nodes[n]["type"] == "indication"]
            n_ref, n_all = label_table(set(drugs), set(inds))
            shutil.copy(os.path.join(OUT, "drug_indication_df.tsv"), os.path.join(tmp, "data", "drug_indication_df.tsv"))
            cfg = {"method": "diffusion", "eval": {"graph": "eval.weighted.edgelist"},
                   "diffusion": {"eval_diffusion_embs_dir": "results/"},
                   "networks": {"drug_to_indication": "data/drug_indication_df.tsv"},
                   "node2vec": {"eval_emb_file_prefix": "eval_n2v", "walk_length": WALK, "number_walk": NUM},
                   "gcn": {"embs": "node2vec", "emb_file": "gcn.embs.txt"}}
            buf = io.StringIO()
            with redirect_stdout(buf):
                m = ev.main(cfg)
            line = buf.getvalue().strip().split("\n")[-1]
            order = [n for n in m.nodelist if m.graph.nodes[n]["type"] == "indication"]
            assert len(recorded) == len(order)
            expected["diffusion"] = {"indications": order, "auc": recorded[:], "line": line}
            shutil.copy("eval.weighted.edgelist", os.path.join(OUT, "eval.weighted.edgelist"))
            dp = ref_dp.DiffusionProfiles(alpha=None, max_iter=None, tol=None, weights=None, num_cores=None, save_load_file_path="results/")
            dp.load_diffusion_profiles(order)
            prof = np.stack([dp.drug_or_indication2diffusion_profile[i] for i in order])
            didx = [m.nodelist.index(d) for d in m.nodelist if m.graph.nodes[d]["type"] == "drug"]
            gaps = [min_gap(p[didx]) for p in prof]
            np.savez(os.path.join(OUT, "diffusion_profiles.npz"), nodelist=np.asarray(m.nodelist), indications=np.asarray(order),
                     profiles=prof)
            label_graph = ref_n2n.DrugToIndication(False, "data/drug_indication_df.tsv").graph
        finally:
            os.chdir(cwd)
    # seeded embedding files: node2vec rows in a permuted node order, GCN rows in that order
    rng = np.random.RandomState(7)
    nodes = list(msi.graph.nodes)
    perm = [nodes[i] for i in rng.permutation(len(nodes))]
    with open(os.path.join(OUT, "n2v.embs.txt"), "w") as f:
        f.write(f"{len(perm)} {DIM}\n")
        for n in perm:
            f.write(n + " " + " ".join(repr(float(v)) for v in np.round(rng.randn(DIM), 6)) + "\n")
    np.savetxt(os.path.join(OUT, "gcn.embs.txt"), np.round(rng.randn(len(perm), DIM), 6), fmt="%.6f")
    node_vecs = np.loadtxt(os.path.join(OUT, "n2v.embs.txt"), skiprows=1, dtype=object)
    names = list(node_vecs[:, 0])
    for case, embs in (("node2vec", node_vecs[:, 1:].astype(np.float64)),
                       ("gcn", normalize(np.loadtxt(os.path.join(OUT, "gcn.embs.txt")), axis=1))):
        drug_names = [n for n in names if msi.graph.nodes[n]["type"] == "drug"]      # graph_embedding's loop
        drug_embs = np.array([embs[names.index(n)] for n in drug_names])
        aucs = []
        for i in order:
            prox = np.matmul(drug_embs, np.array(embs[names.index(i)]))
            assert min_gap(prox) > 1e-9, (case, i, min_gap(prox))
            ref = np.zeros(len(drug_names), dtype=int)
            for d in label_graph[i]:
                ref[drug_names.index(d)] = 1
            aucs.append(float(roc_auc_score(ref, prox)))
        a = np.array(aucs)
        expected[case] = {"indications": order, "auc": aucs, "line": f"median auc: {np.median(a)}, mean auc: {a.mean()}"}
    with open(os.path.join(OUT, "expected.json"), "w") as f:
        json.dump(expected, f, indent=1)
    print(f"labels: {n_ref} reference pairs + {n_all - n_ref} seeded; {len(order)} indications, {len(drugs)} drugs")
    print("diffusion drug-score gaps per indication (min):", min(gaps))
    for k, v in expected.items():
        print(k, v["line"])


if __name__ == "__main__":
    main()
