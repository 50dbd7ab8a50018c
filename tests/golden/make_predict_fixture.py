#!/usr/bin/env python3
"""Golden fixture for predict_drug.py: the msi_small tables with a few blank name cells, a seeded node2vec file and a seeded GCN
file, and the REFERENCE's own outputs on them.  predict_drug.py is imported with sys.modules stubs for multiscale_interactome.*
(pointed at the reference's multiscale/ packages) and np.float = float; graph_embedding + output_drugs write the node2vec and GCN drug
tables, the reference's DiffusionProfiles (with only the return line's indexing fixed) the diffusion table, and run_covid.py:294-319
is restated with networkx for the protein table.  Per row it records whether networkx's path is the only shortest path.
Run in the build container only:  python tests/golden/make_predict_fixture.py"""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get("GSS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "msi_small")
OUT = os.path.join(HERE, "predict_msi_small")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "multiscale"))
sys.path.insert(0, REF)

TABLES = ("drug_to_protein", "indication_to_protein", "protein_to_protein", "protein_to_functional_pathway",
          "functional_pathway_to_functional_pathway")
BLANK = {("drug_to_protein", "DB00004"), ("protein_to_protein", "117"), ("protein_to_functional_pathway", "GO:0000011"),
         ("functional_pathway_to_functional_pathway", "GO:0000011"), ("drug_to_protein", "117"), ("protein_to_functional_pathway", "117")}
TOPK = 10
DIM = 8


def copy_tables():
    for t in TABLES:
        lines = open(os.path.join(SRC, t + ".tsv")).read().splitlines()
        out = [lines[0]]
        for line in lines[1:]:
            p = line.split("\t")
            for col, name_col in ((0, 4), (1, 5)):
                if (t, p[col]) in BLANK:
                    p[name_col] = ""
            out.append("\t".join(p))
        open(os.path.join(OUT, t + ".tsv"), "w").write("\n".join(out) + "\n")
    ids = [l.strip() for l in open(os.path.join(SRC, "pathway_ids.txt")) if l.strip()]
    open(os.path.join(OUT, "pathways.tsv"), "w").write("Pathway_ID\tname\n" + "".join(f"{i}\tp\n" for i in ids))


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
    from diff_prof import diffusion_profiles as ref_dp
    np.float = float
    mods = {"multiscale_interactome": types.ModuleType("multiscale_interactome"),
            "multiscale_interactome.openne": types.ModuleType("multiscale_interactome.openne"),
            "multiscale_interactome.openne.node2vec": types.ModuleType("n2v"),
            "multiscale_interactome.openne.graph": types.ModuleType("graph"),
            "multiscale_interactome.msi": types.ModuleType("multiscale_interactome.msi"),
            "multiscale_interactome.msi.msi": ref_msi,
            "multiscale_interactome.diff_prof": types.ModuleType("multiscale_interactome.diff_prof"),
            "multiscale_interactome.diff_prof.diffusion_profiles": ref_dp,
            "utils": types.ModuleType("utils")}
    mods["multiscale_interactome.openne.node2vec"].Node2vec = None
    mods["multiscale_interactome.openne.graph"].Graph = None
    for k in ("query_uniprot2data", "make_SARSCOV2_PPI", "convert_name_list"):
        setattr(mods["utils"], k, None)
    sys.modules.update(mods)
    import predict_drug
    return predict_drug, ref_msi, ref_dp


def ref_msi_graph(ref_msi, pathway):
    p = lambda n: os.path.join(OUT, n + ".tsv")  # noqa: E731
    msi = ref_msi.MSI(drug2protein_file_path=p("drug_to_protein"), indication2protein_file_path=p("indication_to_protein"),
                      protein2protein_file_path=p("protein_to_protein"), protein2functional_pathway_file_path=p("protein_to_functional_pathway"),
                      functional_pathway2functional_pathway_file_path=p("functional_pathway_to_functional_pathway"),
                      indication2protein_directed=False)
    msi.load()
    weights = {'down_functional_pathway': 4.4863053901688685, 'indication': 3.541889556309463,
               'functional_pathway': 6.583155399238509, 'up_functional_pathway': 2.09685000906964,
               'protein': 4.396695660380823, 'drug': 3.2071696595616364}
    msi.weight_graph(weights)
    if pathway:   # predict_drug.py:182-196
        import pandas as pd
        ids = list(set(pd.read_csv(os.path.join(OUT, "pathways.tsv"), sep="\t")["Pathway_ID"]))
        for pw in ids:
            if pw in msi.graph.nodes:
                msi.graph.add_edge('NodeCovid', pw, weight=3.0 / len(ids))
                msi.graph.add_edge(pw, 'NodeCovid', weight=3.0 / len(ids))
    return msi


def unique_flags(msi, sources, target="NodeCovid"):
    import networkx as nx
    out = []
    for s in sources:
        out.append(sum(1 for _ in zip(range(2), nx.all_shortest_paths(msi.graph, s, target))) == 1)
    return out


def main():
    import networkx as nx
    import pandas as pd
    os.makedirs(OUT, exist_ok=True)
    copy_tables()
    pd_, ref_msi, ref_dp = stub_modules()
    msi = ref_msi_graph(ref_msi, pathway=True)
    rng = np.random.RandomState(5)
    nodes = list(msi.graph.nodes)
    order = [nodes[i] for i in rng.permutation(len(nodes))]     # embedding-file order differs from graph order
    with open(os.path.join(OUT, "n2v.embs.txt"), "w") as f:
        f.write(f"{len(order)} {DIM}\n")
        for n in order:
            f.write(n + " " + " ".join(repr(float(v)) for v in np.round(rng.randn(DIM), 6)) + "\n")
    np.savetxt(os.path.join(OUT, "gcn.embs.txt"), np.round(rng.randn(len(order), DIM), 6), fmt="%.6f")
    name2map = {k: (None if (isinstance(v, float) and np.isnan(v)) else v) for k, v in msi.node2name.items()}
    json.dump(name2map, open(os.path.join(OUT, "node2name.json"), "w"), indent=0, sort_keys=True)
    flags = {}
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for case, gcn, pathway in (("node2vec", False, False), ("gcn", True, True)):
                m = ref_msi_graph(ref_msi, pathway)
                cfg = {"node2vec": {"emb_file_prefix": None, "walk_length": 16, "number_walk": 64},
                       "gcn": {"emb_file": os.path.join(OUT, "gcn.embs.txt")}}
                shutil.copy(os.path.join(OUT, "n2v.embs.txt"), os.path.join(tmp, "n2v_num_64_len_16.embs.txt"))
                cfg["node2vec"]["emb_file_prefix"] = os.path.join(tmp, "n2v")
                names, ranked, prox = pd_.graph_embedding(cfg, m, gcn=gcn)
                pd_.output_drugs(names, ranked, prox, TOPK, os.path.join(OUT, f"expected_{case}.tsv"), m)
                flags[case] = unique_flags(m, ranked[:TOPK])
            # diffusion: the reference's DiffusionProfiles; predict_drug.diffusion_method with its return indexing fixed
            m = ref_msi_graph(ref_msi, pathway=False)
            ddir = os.path.join(tmp, "dp")
            dp = ref_dp.DiffusionProfiles(alpha=0.8595436247434408, max_iter=1000, tol=1e-06,
                                          weights={'down_functional_pathway': 4.4863053901688685, 'indication': 3.541889556309463,
                                                   'functional_pathway': 6.583155399238509, 'up_functional_pathway': 2.09685000906964,
                                                   'protein': 4.396695660380823, 'drug': 3.2071696595616364},
                                          num_cores=1, save_load_file_path=ddir)
            os.makedirs(ddir)
            dp.calculate_diffusion_profiles(m)
            dps = ref_dp.DiffusionProfiles(alpha=None, max_iter=None, tol=None, weights=None, num_cores=None, save_load_file_path=ddir)
            m.load_saved_node_idx_mapping_and_nodelist(ddir)
            dps.load_diffusion_profiles(m.drugs_in_graph + m.indications_in_graph)
            res = dps.drug_or_indication2diffusion_profile["NodeCovid"]
            drugs, prox = [], []
            for i, node in enumerate(m.nodelist):
                if m.graph.nodes[node]['type'] == 'drug':
                    drugs.append(node)
                    prox.append(res[i])
            rid = np.argsort(np.array(prox))[::-1]
            ranked = [drugs[i] for i in rid]
            names = [d if m.node2name[d] is np.nan else m.node2name[d] for d in ranked]
            pd_.output_drugs(names, ranked, np.asarray(prox)[rid], TOPK, os.path.join(OUT, "expected_diffusion.tsv"), m)
            flags["diffusion"] = unique_flags(m, ranked[:TOPK])
            np.save(os.path.join(OUT, "diffusion_NodeCovid.npy"), np.asarray(res))
            json.dump(m.nodelist, open(os.path.join(OUT, "diffusion_nodelist.json"), "w"))
        finally:
            os.chdir(cwd)
    # run_covid.py:294-319 on the pathway graph with the GCN file
    from sklearn.preprocessing import normalize
    m = ref_msi_graph(ref_msi, pathway=True)
    gcn_embs = normalize(np.loadtxt(os.path.join(OUT, "gcn.embs.txt")), axis=1)
    nodes = list(np.loadtxt(os.path.join(OUT, "n2v.embs.txt"), skiprows=1, dtype=object)[:, 0])
    covid_emb = gcn_embs[nodes.index('NodeCovid')]
    mask = [m.graph.nodes[n]['type'] == 'protein' and m.node2name[n] is not np.nan for n in nodes]
    pnodes = list(np.array(nodes)[mask])
    pnames = [m.node2name[n] for n in pnodes]
    prox = list(np.matmul(gcn_embs[mask], covid_emb))
    paths, lengths = [], []
    for n in pnodes:
        p = nx.shortest_path(m.graph, source=n, target='NodeCovid')
        paths.append(', '.join(x if m.node2name[x] is np.nan else m.node2name[x] for x in p))
        lengths.append(len(p) - 1)
    pd.DataFrame({'protein name': pnames, 'proximity to Covid-19': prox, 'shortest path to Covid-19': paths, 'path length': lengths}) \
        .to_csv(os.path.join(OUT, "expected_proteins.tsv"), sep='\t', na_rep='NA', index=False)
    flags["proteins"] = unique_flags(m, pnodes)
    json.dump(flags, open(os.path.join(OUT, "unique_paths.json"), "w"))
    print({k: f"{sum(v)}/{len(v)} unique" for k, v in flags.items()})


if __name__ == "__main__":
    main()
