#!/usr/bin/env python3
"""Network proximity at the reference's size (the 2016 network's LCC, 13,329 nodes; 238 drugs x 78 diseases = 18,564 pairs; all five
measures; 1,000 random samples per set) from tests/golden/proximity_2016.npz.  Prints one JSON line: the all-pairs BFS, random-set,
set-statistics and scoring milliseconds (device events), the end-to-end seconds with host preparation (LCC, bins, set tables), the
byte model of DESIGN.md section 9.2 for each kernel with its achieved rate, and the numpy mirror's seconds per pair on this host's
cores extrapolated to the table.  networkx / toolbox are not measured (neither is part of this project); no speedup is quoted.
usage: proximity_bench.py [--reps R] [--mirror-pairs P]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import proximity_mirror as M  # noqa: E402
from gcn_drug_repurposing_amd import proximity as P  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mirror-pairs", type=int, default=4)
    args = ap.parse_args()
    fx = M.Fixture()
    net = fx.net
    n, nnz = net.n, len(net.col)
    n_random = 1000
    R = n_random + 1
    best = {}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        eng, apsp = timed(lambda: P.ProximityEngine(net))
        bins = P.degree_bins(net.degree, 100)
        fs = [net.node_set(s) for s in fx.drugs]
        ts = [net.node_set(s) for s in fx.diseases]
        (fn, fsz), rs_f = timed(lambda: eng.set_table(fs, 0, n_random, 452456, bins))
        (tn, tsz), rs_t = timed(lambda: eng.set_table(ts, 1, n_random, 452456, bins))
        (f_inner, _, _), st_f = timed(lambda: eng.set_stats(fn, fsz, centres=False))
        (t_inner, tc, tnc), st_t = timed(lambda: eng.set_stats(tn, tsz, centres=True))
        _, score = timed(lambda: eng.score(fx.drugs, fx.diseases, measures=P.MEASURES, n_random=n_random, seed=452456))
        e2e = time.perf_counter() - t0
        eng.close()
        cur = {"apsp_ms": apsp, "random_sets_ms": rs_f + rs_t, "set_stats_ms": st_f + st_t, "score_call_ms": score, "e2e_s": e2e}
        best = {k: min(v, best.get(k, v)) for k, v in cur.items()}
    # the score() call repeats random sets and set statistics; the scoring kernels alone are the difference
    score_only = best["score_call_ms"] - best["random_sets_ms"] - best["set_stats_ms"]
    nt = fsz.cpu().numpy().astype(np.int64)
    ns = tsz.cpu().numpy().astype(np.int64)
    lookups = int(np.einsum("ir,jr->", nt, ns))                     # sum over pairs and samples of |T'| |S'|
    ncen = tnc.cpu().numpy().astype(np.int64)
    lookups_c = int(np.einsum("ir,jr->", nt, ncen))
    set_lookups = int((ns ** 2).sum() * 2 + (nt ** 2).sum())
    apsp_bytes = n * nnz * 4.0 + n * (n + 1) * 4.0 + n * n         # every row read once per source, rowptr, the matrix written
    peak_hbm = 8.0e12
    out = {
        "n": n, "nnz": nnz, "pairs": len(fx.drugs) * len(fx.diseases), "measures": len(P.MEASURES), "n_random": n_random,
        "apsp_ms": round(best["apsp_ms"], 3),
        "apsp_model_bytes": apsp_bytes, "apsp_gbps": round(apsp_bytes / best["apsp_ms"] / 1e6, 1),
        "apsp_frac_of_8tbps": round(apsp_bytes / best["apsp_ms"] / 1e-3 / peak_hbm, 4),
        "random_sets_ms": round(best["random_sets_ms"], 3),
        "set_stats_ms": round(best["set_stats_ms"], 3), "set_stats_lookups": set_lookups,
        "score_ms": round(score_only, 3), "score_lookups": lookups + lookups_c,
        "score_lookups_per_s": (lookups + lookups_c) / score_only * 1e3,
        "score_line_model_bytes": (lookups + lookups_c) * 128.0,
        "score_line_frac_of_8tbps": round((lookups + lookups_c) * 128.0 / score_only / 1e-3 / peak_hbm, 4),
        "e2e_s": round(best["e2e_s"], 3),
    }
    # the mirror on this host: full statistics (5 measures, 1,000 samples) of a few pairs, extrapolated
    eng = P.ProximityEngine(net)
    D = eng.distances().cpu().numpy()
    eng.close()
    dist = lambda T, S: D[np.ix_(np.asarray(T), np.asarray(S))]  # noqa: E731
    bl = M.bins(net.degree, 100)
    nb = M.bin_of(bl, n)
    rng = np.random.RandomState(0)
    t0 = time.perf_counter()
    for q in rng.choice(len(fx.pair_drug), args.mirror_pairs, replace=False):
        i, j = int(fx.pair_drug[q]), int(fx.pair_disease[q])
        M.proximity(dist, net.node_set(fx.drugs[i]), net.node_set(fx.diseases[j]), nb, bl, 452456, i, j, n_random)
    per = (time.perf_counter() - t0) / args.mirror_pairs
    out["mirror_s_per_pair_one_core"] = round(per, 3)
    out["mirror_table_s_one_core_extrapolated"] = round(per * out["pairs"], 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
