#!/usr/bin/env python3
"""Golden fixture for gene knock-outs of diffusion profiles: run the REFERENCE on the small MSI tables of tests/golden/msi_small/ --
MSI.load, msi.graph.remove_edges_from(in_edges(g) + out_edges(g)), MSI.weight_graph, then DiffusionProfiles' matrix surgery and
power_iteration (multiscale/diff_prof/diffusion_profiles.py:30-90) -- for a few (start, gene) columns and their baselines (gene = ''),
and record the converged vectors.  Run in the build container only:

    python tests/golden/make_knockout_fixture.py

The library aliases the reference needs on current networkx / scipy are those of make_diffusion_fixture.py.  No reference code is changed
or copied; the output is data only."""
import os
import sys

import numpy as np

REF = os.environ.get("GSS_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = os.path.join(HERE, "msi_small")
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REF, "multiscale"))
sys.path.insert(0, REF)

ALPHA, MAX_ITER, TOL = 0.8595436247434408, 1000, 1e-06                     # evaluate_auc.py:80-83
WEIGHTS = {'down_functional_pathway': 4.4863053901688685, 'indication': 3.541889556309463,
           'functional_pathway': 6.583155399238509, 'up_functional_pathway': 2.09685000906964,
           'protein': 4.396695660380823, 'drug': 3.2071696595616364}        # evaluate_auc.py:84-91


def main():
    import networkx as nx
    import scipy
    import scipy.sparse as sp
    if not hasattr(nx, "to_scipy_sparse_matrix"):
        nx.to_scipy_sparse_matrix = lambda g, nodelist=None, weight="weight", dtype=None: sp.csr_matrix(
            nx.to_scipy_sparse_array(g, nodelist=nodelist, weight=weight, dtype=dtype, format="csr"))
    for name in ("array", "repeat", "where", "absolute"):
        if not hasattr(scipy, name):
            setattr(scipy, name, getattr(np, name))
    from msi.msi import MSI                                      # the reference
    from diff_prof.diffusion_profiles import DiffusionProfiles   # the reference

    p = lambda n: os.path.join(SMALL, n + ".tsv")  # noqa: E731

    def fresh():
        msi = MSI(drug2protein_file_path=p("drug_to_protein"), indication2protein_file_path=p("indication_to_protein"),
                  protein2protein_file_path=p("protein_to_protein"), protein2functional_pathway_file_path=p("protein_to_functional_pathway"),
                  functional_pathway2functional_pathway_file_path=p("functional_pathway_to_functional_pathway"))
        msi.load()
        return msi

    msi = fresh()
    starts = sorted(msi.drugs_in_graph + msi.indications_in_graph)
    proteins = sorted(n for n in msi.nodelist if msi.node2type[n] == "protein")
    hub = sorted(proteins, key=lambda n: (-msi.graph.degree(n), n))
    columns = []
    for s in (starts[0], starts[4], starts[11], starts[-1]):
        mine = sorted(msi.drug_or_indication2proteins[s])
        far = [g for g in hub if g not in mine]
        columns += [(s, ""), (s, mine[0]), (s, far[0]), (s, far[len(far) // 2])]
    prof, iters = [], []
    for s, g in columns:
        msi = fresh()
        if g:
            msi.graph.remove_edges_from(list(msi.graph.in_edges(g)) + list(msi.graph.out_edges(g)))
        msi.weight_graph(WEIGHTS)
        dp = DiffusionProfiles(alpha=ALPHA, max_iter=MAX_ITER, tol=TOL, weights=WEIGHTS, num_cores=1, save_load_file_path=None)
        dp.get_initial_M(msi)
        m, sv = dp.refine_M_S(dp.convert_M_to_make_all_drugs_indications_sinks_except_selected(msi, [s]))
        prof.append(dp.power_iteration(m, sv, msi.nodelist, dp.get_personalization_dictionary([s], msi.nodelist)))
    out = os.path.join(HERE, "knockout_msi_small.npz")
    np.savez_compressed(out, nodelist=np.array(msi.nodelist), starts=np.array([s for s, _ in columns]), genes=np.array([g for _, g in columns]),
                        profiles=np.stack(prof), alpha=ALPHA, tol=TOL, max_iter=MAX_ITER)
    print("columns", columns, "profile sums", np.stack(prof).sum(1).min(), np.stack(prof).sum(1).max(), "->", out)


if __name__ == "__main__":
    main()
