#!/usr/bin/env python3
"""The gene-set enrichment of diffusion profiles (csrc/enrich.hip) at the size a user runs it, and the numpy mirror at the CLI test's size.

The real-sized call: a universe of M = 17,660 proteins scattered over 29,960 nodes, 2 profiles (seeded, heavy-tailed), the sets with the
sizes of the reference's biological functions at enrich.py's default bounds (tests/golden/function_set_sizes.json: 5 .. 500 proteins; the
members are seeded random places -- the time of a set depends on its size, not on which proteins it holds), 10,000 samples per distinct
size.
  1. device events around gss_profile_order, gss_enrich_lists and gss_enrich_random, each entry point's own read-backs and
     synchronisations included, and around the three in a row: the median of --reps calls after 2 warm-ups;
  2. the numpy mirror (tests/enrich_mirror.py) on one core at the CLI test's size -- 60 places, 2 profiles, 24 sets of 2 .. 5 places, 200
     samples: a host clock around the order, the scores, the null and the statistics;
  3. three samples of the device's null against the mirror (equality; the tests hold every bit).
Writes profiles/enrich_bench.json (or --out).   python tools/enrich_bench.py [--reps 5] [--samples 10000]"""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enrich_bench.json"))
    a = ap.parse_args()
    import torch
    import enrich_mirror as M
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd import enrich as E
    hashes = _lib.source_hashes()
    lib = _lib.load()
    assert lib.gss_source_hash(b"enrich.hip").decode() == hashes["enrich.hip"], "the library was not built from this tree"
    hist = json.load(open(os.path.join(ROOT, "tests", "golden", "function_set_sizes.json")))["proteins_per_function_histogram"]
    set_sizes = [int(m) for m, count in hist.items() for _ in range(count) if 5 <= int(m) <= 500]
    sizes = sorted(set(set_sizes))
    n, m_places, nc, P = 29960, 17660, 2, a.samples
    rng = np.random.RandomState(0)
    universe = np.sort(rng.permutation(n)[:m_places]).astype(np.int32)
    x = torch.from_numpy(np.exp(3 * rng.randn(n, nc))).cuda()
    sets = [rng.permutation(m_places)[:m] for m in set_sizes]
    out = {"source_hash": {k: hashes[k] for k in ("enrich.hip", "counter_rng.h", "profile_front.h", "rank_keys.h", "*")}, "reps": a.reps, "n": n,
           "M": m_places, "profiles": nc, "sets": len(sets), "distinct_sizes": len(sizes), "largest_set": sizes[-1], "members": int(sum(set_sizes)),
           "samples": P}
    print(json.dumps({k: out[k] for k in ("M", "profiles", "sets", "distinct_sizes", "largest_set", "samples")}), flush=True)
    keep = {}

    def order():
        keep["order"] = E.profile_order(x, [0, 1], universe)

    def lists():
        keep["es"] = E.enrichment_scores(keep["order"], sets)

    def null():
        keep["null"] = E.random_enrichment_scores(keep["order"], sizes, P, seed=0)

    def whole():
        order()
        lists()
        null()

    note = "device events around the Python call: uploads of the lists, the entry point's read-backs and synchronisations, its launches"
    for name, fn in (("1_profile_order", order), ("1_enrich_lists", lists), ("1_enrich_random", null), ("1_all_three", whole)):
        out[name] = dict(timed(fn, a.reps), note=note)
        print(name, json.dumps(out[name]), flush=True)

    pos, w = keep["order"].pos.cpu().numpy(), keep["order"].w.cpu().numpy()
    head = keep["null"][:, :3].cpu().numpy()
    same = all(np.array_equal(M.random_scores(pos[j], w[j], sizes, 0, 0, 3)[0].view(np.int64), head[j].view(np.int64)) for j in range(nc))
    out["3_first_three_samples_equal_the_mirror"] = bool(same)
    print("3 equal", same, flush=True)

    small_rng = np.random.RandomState(1)
    small_x = small_rng.rand(2, 86)
    small_universe = np.arange(60)
    small_sets = [small_rng.permutation(60)[:2 + k % 4] for k in range(24)]
    small_sizes = sorted({len(s) for s in small_sets})
    t0 = time.perf_counter()
    for j in range(2):
        p, ww = M.order(small_x[j], small_universe)
        scored = [M.es_peak(p, ww, s) for s in small_sets]
        small_null, _ = M.random_scores(p, ww, small_sizes, 0, 0, 200)
        M.stats([e for e, _ in scored], [k for _, k in scored], small_sets, p, small_sizes, small_null)
    out["2_numpy_mirror_cli_test_size"] = {"seconds": time.perf_counter() - t0, "M": 60, "profiles": 2, "sets": 24, "samples": 200,
                                           "note": "one core, a host clock; the mirror is written for clarity, one Python statement per operation"}
    print("2 mirror", json.dumps(out["2_numpy_mirror_cli_test_size"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
