#!/usr/bin/env python3
"""Gene knock-outs on the 29,960-node whole-graph stand-in: a screen of --genes proteins (evenly spaced through the protein list; one chunk
of 2 + 2 * genes columns) for one drug-indication pair.  Reports the host's list construction in seconds, the device-event time of the
batched run per knocked-out column (median of --reps runs after one warm-up) beside a plain batch of the same kpad in the same process,
the list sizes per column (overrides, correction entries: mean, max), the paired-distance launch against gss_profile_dist on the same
T = 256 pairs (whose diagonal is all a screen uses), and the route the engine offered before knock-outs were columns: one weighted graph,
one PprProblem and one PprEngine per gene, timed on 16 genes.
Writes profiles/knockout_bench.json.   python tools/knockout_bench.py [--genes 2047] [--reps 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 1:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=2047)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from gcn_drug_repurposing_amd import _lib, msi, synth
    from gcn_drug_repurposing_amd import knockout as K
    from gcn_drug_repurposing_amd.diffusion import PprEngine, PprProblem, compare_profile_pairs, compare_profiles
    from gcn_drug_repurposing_amd.predict import DIFFUSION
    w, alpha, max_iter, tol = DIFFUSION["weights"], DIFFUSION["alpha"], DIFFUSION["max_iter"], DIFFUSION["tol"]
    hashes = _lib.source_hashes()
    out = {"graph": "synth.standin_tables(seed=1)", "source_hash": {k: hashes[k] for k in ("ppr.hip", "profile_dist.hip", "*")}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, rows in synth.standin_tables(seed=1).items():
            with open(os.path.join(tmp, name + ".tsv"), "w") as f:
                f.write("node_1\tnode_2\n")
                f.writelines(f"{u}\t{v}\n" for u, v in rows)
        g = msi.MsiGraph().load({name: os.path.join(tmp, name + ".tsv") for name, _, _ in msi.COMPONENTS})
    proteins = [n for n in g.names if g.type[n] == msi.PROTEIN]
    genes = [proteins[i] for i in np.linspace(0, len(proteins) - 1, min(a.genes, len(proteins))).astype(int)]
    genes = list(dict.fromkeys(genes))
    drug, ind = g.drugs_in_graph[0], g.indications_in_graph[0]
    (cols, pairs, rows), = K.plan_chunks([(drug, ind, x) for x in genes], max_columns=2 * len(genes) + 4)
    t0 = time.perf_counter()
    kg = K.KnockoutGraph(g, w)                                     # once per graph and weights, shared by every chunk
    t1 = time.perf_counter()
    prob = K.KnockoutProblem(kg, w, cols)
    t2 = time.perf_counter()
    out["host_graph_s"], out["host_lists_s"], out["host_list_construction_s"] = t1 - t0, t2 - t1, t2 - t0
    out["host_lists_ms_per_column"] = (t2 - t1) * 1e3 / len(cols)
    n_ovr, n_corr = np.diff(prob.ovr_ptr), np.bincount(prob.corr_grp_col, weights=np.diff(prob.corr_ptr), minlength=prob.k)
    ko = prob.dead >= 0
    out.update(nodes=prob.n, nnz=int(prob.mt.nnz), proteins=len(proteins), genes=len(genes), columns=prob.k, kpad=prob.kpad,
               overrides_per_knockout_column={"mean": float(n_ovr[ko].mean()), "max": int(n_ovr[ko].max())},
               correction_entries_per_knockout_column={"mean": float(n_corr[ko].mean()), "max": int(n_corr[ko].max())},
               correction_groups=int(len(prob.corr_grp_row)))
    eng = K._engine(prob)
    run = timed(lambda: eng.run(alpha, tol, max_iter), a.reps)
    x, its = eng.run(alpha, tol, max_iter)
    run["ms_per_column"] = run["ms_median"] / prob.k
    run["iterations_max"] = int(its.max())
    out["knockout_batch"] = run
    idx = {n: i for i, n in enumerate(prob.names)}
    plain = PprEngine(PprProblem(prob.m0, [idx[s] for s, _ in cols], prob.proteins_of))
    base = timed(lambda: plain.run(alpha, tol, max_iter), a.reps)
    base["ms_per_column"] = base["ms_median"] / prob.k
    base["iterations_max"] = int(plain.run(alpha, tol, max_iter)[1].max())
    out["plain_batch_same_kpad"] = base
    out["knockout_over_plain"] = run["ms_median"] / base["ms_median"]
    del plain
    ca, cb = [p[0] for p in pairs[:256]], [p[1] for p in pairs[:256]]
    out["distances_T256"] = {}
    for m in ("correlation", "cityblock"):
        paired = timed(lambda: compare_profile_pairs(x, ca, cb, m), a.reps)
        matrix = timed(lambda: compare_profiles(x, ca, cb, m), a.reps)
        out["distances_T256"][m] = {"pairs": paired, "matrix_of_which_the_diagonal_is_used": matrix,
                                    "matrix_over_pairs": matrix["ms_median"] / paired["ms_median"],
                                    "note": "device events around the Python entry points: list upload, column check, workspace, kernels"}
    del eng
    sample = genes[:: max(1, len(genes) // 16)][:16]
    t0 = time.perf_counter()
    for x_ in sample:                                              # the route before knock-outs were columns: one graph per gene
        m0 = K.weighted_csr(g, w, without=x_)[0]
        e = PprEngine(PprProblem(m0, [idx[drug], idx[ind]], prob.proteins_of))
        e.run(alpha, tol, max_iter)
        torch.cuda.synchronize()
        del e
    per_gene = (time.perf_counter() - t0) / len(sample)
    out["one_engine_per_gene"] = {"genes": len(sample), "s_per_gene": per_gene, "note": "wall clock: weighting, PprProblem, PprEngine, run"}
    batched = (out["host_list_construction_s"] + run["ms_median"] * 1e-3) / len(genes)
    out["batched_s_per_gene"] = batched
    out["one_engine_per_gene_over_batched"] = per_gene / batched
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "knockout_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
