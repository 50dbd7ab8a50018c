#!/usr/bin/env python3
"""The permutation null of Mantel's test (gss_matrix_cross_sums, csrc/matrix_mantel.hip) at the sizes a user runs it: n = 63 (the drugs of
the Connectivity Map table), 1,661 (the drugs of the multiscale interactome) and 4,096 (the kernel's limit), S = --permutations each.

The matrices: two seeded symmetric matrices per n, standardised as mantel() standardises them (Spearman: the average-tie ranks of the pair
values, centred, unit norm), so the kernel reads what it reads in use; the values do not change what it costs.
  1. gss_matrix_cross_sums, mode 1, S replicates in one call: device events around the entry point, median of --reps calls after 2; the
     gathered products per second that follow from it (n (n - 1) / 2 * S over the median);
  2. mantel() end to end per method (symmetry and NaN checks, both standardisations, r, the null, its download, host statistics): wall
     clock behind a device synchronise, median of min(--reps, 2) calls after 1; and the ranking of one matrix's pair values alone, which
     is what Spearman adds (gss_profile_rank gives a column to one workgroup, and here the column is n (n - 1) / 2 long);
  3. the numpy route on this machine's host cores for --host-permutations relabellings (fewer at the larger sizes), EXTRAPOLATED linearly to
     S and labelled so: per relabelling the mirror's keys, np.lexsort, one np.ix_ gather of b and one product-sum over the lower triangle;
  4. three replicates of the device's null against that numpy route (absolute difference of correlations; the tests hold every bit).
Writes profiles/mantel_bench.json (or --out).   python tools/time_mantel.py [--reps 5] [--permutations 10000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = (63, 1661, 4096)


def device_ms(fn, reps):
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


def wall_ms(fn, reps):
    import torch
    ms = []
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if r >= 1:
            ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--permutations", type=int, default=10000)
    ap.add_argument("--host-permutations", type=int, default=200, help="at n = 63; scaled down by (63 / n)^2 above, at least 3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mantel_bench.json"))
    a = ap.parse_args()
    import torch
    import mantel_mirror as M
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd import mantel as MT
    if not torch.cuda.is_available():
        raise SystemExit("time_mantel: no GPU; nothing is measured without one")
    hashes = _lib.source_hashes()
    lib = _lib.load()
    assert lib.gss_source_hash(b"matrix_mantel.hip").decode() == hashes["matrix_mantel.hip"], "the library was not built from this tree"
    S = a.permutations
    out = {"source_hash": {k: hashes[k] for k in ("matrix_mantel.hip", "counter_rng.h", "rank_keys.h", "*")}, "reps": a.reps, "permutations": S,
           "device": torch.cuda.get_device_name(0), "host_cores": os.cpu_count(), "sizes": {}}
    for n in SIZES:
        K = n * (n - 1) // 2
        rng = np.random.RandomState(n)
        raw = []
        for _ in range(2):
            h = np.triu(rng.rand(n, n), 1)
            raw.append(torch.from_numpy(h + h.T).cuda())
        sa, sb = (MT.standardise_pairs(m, "spearman") for m in raw)
        sums = torch.empty(S, dtype=torch.float64, device="cuda")

        def null():
            _lib.check(lib.gss_matrix_cross_sums(n, sa.data_ptr(), n, sb.data_ptr(), n, 1, 0, 0, S, sums.data_ptr(), None, _lib.current_stream()),
                       "gss_matrix_cross_sums")
        rec = {"pairs": K, "gathered_products": K * S, "matrix_bytes": 8 * n * n, "1_null": device_ms(null, a.reps)}
        rec["1_null"]["products_per_s"] = K * S / (rec["1_null"]["ms_median"] * 1e-3)
        head = sums[:3].cpu().numpy()
        for method in MT.METHODS:
            rec[f"2_mantel_end_to_end_{method}"] = wall_ms(lambda: MT.mantel(raw[0], raw[1], method, S, 0), min(a.reps, 2))
        pairs = MT.pair_values(raw[0])[1]
        rec["2_rank_of_the_pair_values"] = dict(device_ms(lambda: MT.pair_ranks(pairs), min(a.reps, 2)),
                                                note="diffusion.rank_profiles on one column of n (n - 1) / 2 values: one workgroup; twice per spearman call")

        ha, hb = sa.cpu().numpy(), sb.cpu().numpy()
        low = np.tril(ha, -1)
        hs = max(3, int(a.host_permutations * (63.0 / n) ** 2))
        t0 = time.perf_counter()
        host = []
        for s in range(hs):
            p = M.permutation(0, s, n)
            host.append(float(np.sum(low * hb[np.ix_(p, p)])))
        dt = time.perf_counter() - t0
        rec["3_numpy"] = {"permutations_timed": hs, "s_timed": dt, "ms_extrapolated_to_S": dt / hs * S * 1e3,
                          "note": "numpy on the host cores of the machine the GPU is in; linear extrapolation from permutations_timed, not a measurement at S"}
        rec["3_numpy"]["device_speedup_extrapolated"] = rec["3_numpy"]["ms_extrapolated_to_S"] / rec["1_null"]["ms_median"]
        rec["4_max_abs_diff_of_3"] = float(np.max(np.abs(head - np.asarray(host[:3]))))
        out["sizes"][str(n)] = rec
        print(n, json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
