#!/usr/bin/env python3
"""gss_profile_rank and the "spearman" comparison on the diffusion profiles of the 29,960-node whole-graph stand-in (1,661 drugs, 841
indications incl. NodeCovid: 2,502 columns, left on the device by PprEngine.run): the device-event time of the rank transform alone (all
2,502 columns, null list, caller's workspace) and of the whole compare_profiles(..., "spearman") call for indications x drugs and drugs x
drugs (median of --reps calls after two warm-up calls), next to "correlation" on the same blocks, and scipy.stats.rankdata on one core for
64 columns with the extrapolation to 2,502 labelled as such.  --auc adds evaluate_auc.py's median / mean AUC on the stand-in for
'correlation' and 'spearman'; --fixture the largest difference between the Spearman distances of device-made and of reference-made profiles
on the msi_small fixture (a rank is discontinuous: DESIGN.md section 9.10).
Writes profiles/profile_rank_bench.json.   python tools/profile_rank_bench.py [--reps 10] [--auc] [--fixture]"""
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
    for r in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            ms.append(e0.elapsed_time(e1))
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def fixture_swaps():
    """device-made against reference-made profiles of tests/golden/diffusion_msi_small.npz under "spearman" """
    import scipy.sparse as sp
    from gcn_drug_repurposing_amd.diffusion import PprEngine, PprProblem, compare_profiles, rank_profiles
    z = np.load(os.path.join(ROOT, "tests", "golden", "diffusion_msi_small.npz"))
    nodes = [str(v) for v in z["nodelist"]]
    idx = {n: i for i, n in enumerate(nodes)}
    m0 = sp.csr_matrix((z["m_data"], z["m_indices"], z["m_indptr"]), shape=(len(nodes),) * 2)
    starts = np.array([idx[str(s)] for s in z["starts"]])
    prot = {idx[str(s)]: [idx[p] for p in str(ps).split()] for s, ps in zip(z["starts"], z["proteins_of"])}
    eng = PprEngine(PprProblem(m0, starts, prot))
    x, _ = eng.run(float(z["alpha"]), float(z["tol"]), int(z["max_iter"]))
    k = len(starts)
    ref = np.asarray(z["profiles"], np.float64)
    dev = compare_profiles(x, range(k), range(k), "spearman").cpu().numpy()
    want = compare_profiles(ref, None, None, "spearman").cpu().numpy()
    r_dev, r_ref = rank_profiles(x, range(k)).cpu().numpy(), rank_profiles(ref).cpu().numpy()
    return {"profiles": k, "nodes": len(nodes), "max_abs_profile_difference": float(np.abs(x[:, :k].t().cpu().numpy() - ref).max()),
            "rank_entries_that_differ": int((r_dev != r_ref).sum()), "rank_entries": int(r_ref.size),
            "max_abs_spearman_distance_difference": float(np.nanmax(np.abs(dev - want)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--auc", action="store_true")
    ap.add_argument("--fixture", action="store_true")
    a = ap.parse_args()
    import scipy.sparse as sp
    import torch
    from scipy.stats import rankdata
    from gcn_drug_repurposing_amd import _lib, synth
    from gcn_drug_repurposing_amd.diffusion import PprEngine, PprProblem, compare_profiles
    hashes = _lib.source_hashes()
    lib = _lib.load()
    assert lib.gss_source_hash(b"profile_rank.hip").decode() == hashes["profile_rank.hip"], "the library was not built from this tree"
    out = {"graph": "synth.whole_graph_standin(seed=1)", "source_hash": {k: hashes[k] for k in ("profile_rank.hip", "profile_front.h", "rank_keys.h", "*")},
           "reps": a.reps}
    adj, ntype, _ = synth.whole_graph_standin(seed=1)
    m0 = sp.csr_matrix(adj, dtype=np.float64)
    starts = np.flatnonzero(ntype <= 1)
    prot = {int(s): m0.indices[m0.indptr[s]:m0.indptr[s + 1]].tolist() for s in starts}
    eng = PprEngine(PprProblem(m0, starts, prot))
    x, _ = eng.run(0.8595436247434408, 1e-6, 1000)
    torch.cuda.synchronize()
    drugs = np.flatnonzero(ntype[starts] == 0)
    inds = np.flatnonzero(ntype[starts] == 1)
    n, k, ld = x.shape[0], len(starts), int(x.stride(0))
    need = int(lib.gss_profile_rank_workspace_bytes(n, k))
    out.update(nodes=int(n), columns=int(k), drugs=len(drugs), indications=len(inds), ld=ld, workspace_bytes=need)
    r = torch.empty(n, k, dtype=torch.float64, device="cuda")
    ws = torch.empty((need + 7) // 8, dtype=torch.float64, device="cuda")

    def rank_all():
        _lib.check(lib.gss_profile_rank(n, x.data_ptr(), ld, k, None, r.data_ptr(), k, ws.data_ptr(), need, _lib.current_stream()),
                   "gss_profile_rank")
    out["gss_profile_rank"] = dict(timed(rank_all, a.reps), columns=int(k),
                                   note="device events around the entry point alone: null list (no check, no synchronisation), "
                                        "the caller's workspace and output; five panels of at most 512 columns, three launches each")
    print("gss_profile_rank", json.dumps(out["gss_profile_rank"]), flush=True)
    sub = 64
    host = x[:, :sub].t().contiguous().cpu().numpy()
    t0 = time.perf_counter()
    want = rankdata(host, axis=1)
    t_host = time.perf_counter() - t0
    out["scipy_rankdata"] = {"columns": sub, "s": t_host, "extrapolated_s_all_columns": t_host * k / sub,
                             "note": "one host core; the figure for all columns is an extrapolation, not timed",
                             "equal_to_device_on_these_columns": bool(np.array_equal(r[:, :sub].t().cpu().numpy(), want))}
    out["profile_shape"] = {"share_of_exact_zeros": float((host == 0).mean()), "distinct_values_per_profile_median":
                            float(np.median([len(np.unique(v)) for v in host]))}
    out["compare"] = {}
    for m in ("correlation", "spearman"):
        out["compare"][m] = {}
        for label, rows, cols in (("indications_x_drugs", inds, drugs), ("drugs_x_drugs", drugs, drugs)):
            out["compare"][m][label] = dict(timed(lambda: compare_profiles(x, rows, cols, m), a.reps),
                                            note="device events around compare_profiles: list upload, (spearman: workspace and rank matrix "
                                                 "allocation, the unique columns ranked once,) column check, statistics pass and kernel")
        print(m, json.dumps(out["compare"][m]), flush=True)
    del eng, x, r, ws
    if a.fixture:
        out["msi_small_device_vs_reference_profiles"] = fixture_swaps()
        print(json.dumps(out["msi_small_device_vs_reference_profiles"]), flush=True)
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
            for m in ("correlation", "spearman"):
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
    with open(os.path.join(ROOT, "profiles", "profile_rank_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
