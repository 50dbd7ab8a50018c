#!/usr/bin/env python3
"""gss_profile_dist on the diffusion profiles of the 29,960-node whole-graph stand-in (1,661 drugs, 841 indications incl. NodeCovid: 2,502
columns, left on the device by PprEngine.run): per metric the device-event time of the indications x drugs and the drugs x drugs comparison
(median of --reps calls after two warm-up calls), element pairs per second, the share of the fp64 peak (78.6 TFLOP/s, vector and matrix alike: the
public MI355X figure) on the operations the metric needs, and scipy's cdist on a stated sub-block with the extrapolation to the full block
labelled as such; and of compare_profile_pairs (gss_profile_dist_pairs) on 256 drug-indication pairs, knockout.py's chunk.  --auc adds
evaluate_auc.py's median / mean AUC on the stand-in for 'visit' and the five metrics.
Writes profiles/profile_dist_bench.json.   python tools/profile_dist_bench.py [--reps 10] [--auc]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP64 = 78.6e12
# fp64 operations per element pair: |a - b| and the add; the difference, the multiply-add; |a|, |b|, their sum, |a - b|, a division, an add
# (the division counted as one); one multiply-add on the matrix cores plus the centring subtraction of both operands amortised over a tile
OPS = {"cityblock": 2, "euclidean": 2, "canberra": 6, "cosine": 2, "correlation": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--auc", action="store_true")
    a = ap.parse_args()
    import scipy.sparse as sp
    import torch
    from scipy.spatial.distance import cdist
    from gcn_drug_repurposing_amd import _lib, synth
    from gcn_drug_repurposing_amd.diffusion import METRICS, PprEngine, PprProblem, compare_profile_pairs, compare_profiles
    hashes = _lib.source_hashes()
    out = {"graph": "synth.whole_graph_standin(seed=1)", "source_hash": {k: hashes[k] for k in ("profile_dist.hip", "profile_front.h", "rank_keys.h", "*")},
           "reps": a.reps, "peak_fp64_flops": PEAK_FP64, "ops_per_pair": OPS}
    adj, ntype, _ = synth.whole_graph_standin(seed=1)
    m0 = sp.csr_matrix(adj, dtype=np.float64)
    starts = np.flatnonzero(ntype <= 1)
    prot = {int(s): m0.indices[m0.indptr[s]:m0.indptr[s + 1]].tolist() for s in starts}
    eng = PprEngine(PprProblem(m0, starts, prot))
    x, _ = eng.run(0.8595436247434408, 1e-6, 1000)
    torch.cuda.synchronize()
    drugs = np.flatnonzero(ntype[starts] == 0)
    inds = np.flatnonzero(ntype[starts] == 1)
    n = x.shape[0]
    out.update(nodes=int(n), drugs=len(drugs), indications=len(inds), ld=int(x.stride(0)),
               drug_columns_contiguous=bool(np.array_equal(drugs, np.arange(drugs[0], drugs[0] + len(drugs)))),
               indication_columns_contiguous=bool(np.array_equal(inds, np.arange(inds[0], inds[0] + len(inds)))))
    host = x[:, :len(starts)].t().contiguous().cpu().numpy()
    sub = 64
    pair_a, pair_b = drugs[np.arange(256) % len(drugs)], inds[np.arange(256) % len(inds)]
    out["metrics"] = {}
    for m in METRICS:
        rec = {}
        for label, rows, cols in (("indications_x_drugs", inds, drugs), ("drugs_x_drugs", drugs, drugs)):
            ms = []
            for r in range(a.reps + 2):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                d = compare_profiles(x, rows, cols, m)
                e1.record()
                torch.cuda.synchronize()
                if r >= 2:
                    ms.append(e0.elapsed_time(e1))
            pairs = float(len(rows)) * len(cols) * n
            t = float(np.median(ms)) * 1e-3
            rec[label] = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "element_pairs": pairs, "element_pairs_per_s": pairs / t,
                          "share_of_fp64_peak": pairs * OPS[m] / t / PEAK_FP64,
                          "note": "device events around the entry point: list upload, column check, scratch allocation, statistics pass and kernel"}
        t0 = time.perf_counter()
        want = cdist(host[inds[:sub]], host[drugs[:sub]], m)
        t_host = time.perf_counter() - t0
        got = compare_profiles(x, inds[:sub], drugs[:sub], m).cpu().numpy()
        rec["scipy_cdist"] = {"block": f"{sub} x {sub} x {n}", "s": t_host, "element_pairs_per_s": sub * sub * n / t_host,
                              "extrapolated_s_indications_x_drugs": t_host * len(inds) * len(drugs) / (sub * sub),
                              "note": "one host core; the full-block figure is an extrapolation, not timed",
                              "max_abs_difference_to_device_on_block": float(np.nanmax(np.abs(got - want)))}
        ms = []                                                        # gss_profile_dist_pairs at knockout.py's size: 256 listed pairs
        for r in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            compare_profile_pairs(x, pair_a, pair_b, m)
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ms.append(e0.elapsed_time(e1))
        rec["pairs_T256"] = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                             "note": "device events around compare_profile_pairs: list upload, column check, workspace and kernels"}
        out["metrics"][m] = rec
        print(m, json.dumps(rec["indications_x_drugs"]), json.dumps(rec["pairs_T256"]), flush=True)
    del eng, x
    if a.auc:
        from gcn_drug_repurposing_amd import evaluate
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, "data")
            os.makedirs(d)
            for name, rows in synth.standin_tables(seed=1).items():
                with open(os.path.join(d, name + ".tsv"), "w") as f:
                    f.write("node_1\tnode_2\n")
                    f.writelines(f"{u}\t{v}\n" for u, v in rows)
            labels = os.path.join(d, "drug_indication_df.tsv")
            with open(labels, "w") as f:
                f.write("drug\tdrug_name\tindication\tindication_name\n")
                f.writelines(f"{dr}\tx\t{i}\ty\n" for i, ds in synth.standin_drug_indications().items() for dr in sorted(ds))
            out["auc"] = {}
            for m in ("visit",) + METRICS:
                cfg = {"method": "diffusion", "eval": {"graph": os.path.join(tmp, "eval.edgelist")},
                       "networks": {"protein_to_protein": os.path.join(d, "protein_to_protein.tsv"), "drug_to_indication": labels},
                       "diffusion": {"eval_diffusion_embs_dir": os.path.join(tmp, "dp"), "compare": m}}
                t = {}
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    res = evaluate.run(evaluate.Settings(cfg), timings=t, err=open(os.devnull, "w"))
                a_ = res.auc[res.kept]
                out["auc"][m] = {"median": float(np.median(a_)), "mean": float(a_.mean()), "indications": len(res.kept), "scores_s": t["scores_s"],
                                 "auc_s": t["auc_s"]}
                print(m, out["auc"][m], flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "profile_dist_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
