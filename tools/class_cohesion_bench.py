#!/usr/bin/env python3
"""The null of the ATC class coherence (gss_pair_sums_random, csrc/class_cohesion.hip) at the size a user runs it, and the stand-in's result table.

The matrix: the drug x drug correlation distances (diffusion.compare_profiles) of the diffusion profiles of the 29,960-node whole-graph
stand-in, restricted to the pool -- the 1,328 of its 1,661 drugs that the reference's drug-class table (tests/golden/atc_classes.npz)
names.  The sizes: the distinct class sizes of the four ATC levels on that pool (58 of them, up to 266).
  1. gss_pair_sums_random at P = 10^4 and 10^5: device events around the entry point (its read-back of the sizes and that synchronisation
     included), median of --reps calls after 2; the same without the gathers' share (sizes = [2]: keys, sort and one entry), as the model's split;
  2. the numpy route on one core for --host-samples samples, EXTRAPOLATED linearly to P and labelled so: per sample the permutation (the
     mirror's keys, np.lexsort), one np.ix_ gather at the largest size and prefix sums -- and the plain form, one np.ix_ gather per size;
  3. three samples of the device's null against the numpy route (relative difference; the tests hold every bit);
  4. the result table: per metric and level, the classes (of at least 2 pool drugs) with Benjamini-Hochberg q < 0.05 among all of the level,
     P = --samples random sets per size.  The stand-in's PPI layer is synthetic: the table says what the program computes, not what the
     multiscale interactome finds.
Writes profiles/class_cohesion_bench.json (or --out).   python tools/class_cohesion_bench.py [--reps 10] [--samples 10000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--host-samples", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_cohesion_bench.json"))
    a = ap.parse_args()
    import scipy.sparse as sp
    import torch
    import class_cohesion_mirror as M
    from gcn_drug_repurposing_amd import _lib, synth
    from gcn_drug_repurposing_amd import classes as K
    from gcn_drug_repurposing_amd.diffusion import ALL_METRICS, PprEngine, PprProblem, compare_profiles
    hashes = _lib.source_hashes()
    lib = _lib.load()
    assert lib.gss_source_hash(b"class_cohesion.hip").decode() == hashes["class_cohesion.hip"], "the library was not built from this tree"
    out = {"graph": "synth.whole_graph_standin(seed=1)", "table": "tests/golden/atc_classes.npz",
           "source_hash": {k: hashes[k] for k in ("class_cohesion.hip", "counter_rng.h", "profile_front.h", "rank_keys.h", "*")}, "reps": a.reps}
    adj, ntype, names = synth.whole_graph_standin(seed=1)
    m0 = sp.csr_matrix(adj, dtype=np.float64)
    starts = np.flatnonzero(ntype <= 1)
    prot = {int(s): m0.indices[m0.indptr[s]:m0.indptr[s + 1]].tolist() for s in starts}
    eng = PprEngine(PprProblem(m0, starts, prot))
    x, _ = eng.run(0.8595436247434408, 1e-6, 1000)
    torch.cuda.synchronize()
    column = {names[int(s)]: c for c, s in enumerate(starts) if ntype[s] == 0}      # drug id -> its profile's column of x
    levels = [1, 2, 3, 4]
    _, ids, table = M.atc_fixture()
    coded = {n for by_code in table.values() for _, members in by_code.values() for n in members}
    pool = sorted((n for n in ids if n in column and n in coded), key=column.__getitem__)
    row = {n: i for i, n in enumerate(pool)}
    cols = [column[n] for n in pool]
    classes = [(k, code, sorted(row[n] for n in table[k][code][1] if n in row)) for k in levels for code in sorted(table[k])]
    classes = [c for c in classes if len(c[2]) >= 2]
    sizes = sorted({len(c[2]) for c in classes})
    n = len(pool)
    out.update(drugs=len(column), table_drugs=len(ids), pool=n, classes_per_level={k: sum(1 for c in classes if c[0] == k) for k in levels},
               distinct_sizes_per_level={k: len({len(c[2]) for c in classes if c[0] == k}) for k in levels}, sizes=sizes,
               pairs_at_largest_size=sizes[-1] * (sizes[-1] - 1) // 2)
    print(json.dumps({k: out[k] for k in ("pool", "classes_per_level", "distinct_sizes_per_level")}), flush=True)

    d = compare_profiles(x, cols, cols, "correlation")
    assert torch.equal(d, d.t()), "the distance matrix is not bitwise symmetric"
    d_sizes = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    d_two = torch.tensor([2], dtype=torch.int32, device="cuda")
    for P in (10000, 100000):
        sums = torch.empty(P, len(sizes), dtype=torch.float64, device="cuda")
        one = torch.empty(P, 1, dtype=torch.float64, device="cuda")

        def null():
            _lib.check(lib.gss_pair_sums_random(n, d.data_ptr(), n, 0, 0, P, len(sizes), d_sizes.data_ptr(), sums.data_ptr(), None,
                                                _lib.current_stream()), "gss_pair_sums_random")

        def sort_only():
            _lib.check(lib.gss_pair_sums_random(n, d.data_ptr(), n, 0, 0, P, 1, d_two.data_ptr(), one.data_ptr(), None, _lib.current_stream()),
                       "gss_pair_sums_random")
        out[f"1_null_P{P}"] = dict(timed(null, a.reps), gathered_entries=P * out["pairs_at_largest_size"],
                                   note="device events around the entry point: the sizes' read-back and its synchronisation, one launch of P workgroups")
        out[f"1_keys_and_sort_P{P}"] = dict(timed(sort_only, a.reps), note="the same call with sizes = [2]: keys, sort and one matrix entry per sample")
        print(P, json.dumps(out[f"1_null_P{P}"]), json.dumps(out[f"1_keys_and_sort_P{P}"]), flush=True)
        if P == 10000:
            head = sums[:3].cpu().numpy()

    h = d.cpu().numpy()
    at = np.asarray(sizes) - 2      # T(m) = r_1 + ... + r_{m-1} = cumsum(r[1:])[m - 2]
    t0 = time.perf_counter()
    host = []
    for s in range(a.host_samples):
        p = M.permutation(0, s, n)[:sizes[-1]]
        r = np.tril(h[np.ix_(p, p)], -1).sum(axis=1)
        host.append(np.cumsum(r[1:])[at])
    t_prefix = (time.perf_counter() - t0) / a.host_samples
    t0 = time.perf_counter()
    for s in range(a.host_samples):
        p = M.permutation(0, s, n)
        [np.tril(h[np.ix_(p[:m], p[:m])], -1).sum() for m in sizes]
    t_plain = (time.perf_counter() - t0) / a.host_samples
    out["2_numpy_one_core"] = {"samples_timed": a.host_samples, "ms_per_sample_one_gather_and_prefix_sums": t_prefix * 1e3,
                               "ms_per_sample_one_gather_per_size": t_plain * 1e3,
                               "EXTRAPOLATED_s_P10000": {"prefix_sums": t_prefix * 1e4, "per_size": t_plain * 1e4},
                               "EXTRAPOLATED_s_P100000": {"prefix_sums": t_prefix * 1e5, "per_size": t_plain * 1e5},
                               "note": "linear extrapolation from samples_timed samples, not a run of P samples"}
    print("2 numpy", json.dumps(out["2_numpy_one_core"]), flush=True)
    out["3_device_vs_numpy_max_relative_difference"] = float(np.max(np.abs(head - np.asarray(host[:3])) / np.asarray(host[:3])))
    print("3 max relative difference", out["3_device_vs_numpy_max_relative_difference"], flush=True)

    lists = [c[2] for c in classes]
    result = {}
    for metric in ALL_METRICS:
        dm = compare_profiles(x, cols, cols, metric)
        try:
            t0 = time.perf_counter()
            rec = K.class_cohesion(dm, lists, a.samples, seed=0, labels=pool)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        except ValueError as e:
            result[metric] = {"refused": str(e)}
            continue
        per_level = {}
        for k in levels:
            of_level = [r for r, c in zip(rec, classes) if c[0] == k]
            q = K.benjamini_hochberg([r["p"] for r in of_level])
            per_level[k] = {"classes": len(of_level), "q_below_0.05": int((q < 0.05).sum()), "z_below_0": sum(1 for r in of_level if r["z"] < 0),
                            "median_z": float(np.median([r["z"] for r in of_level]))}
        result[metric] = {"levels": per_level, "class_cohesion_wall_s": wall}
        print("4", metric, json.dumps(result[metric]), flush=True)
    out["4_standin_result"] = {"samples": a.samples, "seed": 0, "by_metric": result,
                               "note": "the stand-in's PPI layer is synthetic; wall clock = observed sums + null + its download + host statistics"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    import re
    flat = re.sub(r"[\[{][^\[\]{}]*[\]}]", lambda m: re.sub(r"\s*\n\s*", " ", m.group(0)), json.dumps(out, indent=1))     # innermost lists and dicts on one line
    with open(a.out, "w") as f:
        f.write(flat + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
