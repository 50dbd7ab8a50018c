#!/usr/bin/env python3
"""The Steiner trees at the reference's size, from --fixture (default tests/golden/proximity_2016.npz): the disease gene sets of the
2016 network (LCC 13,329 nodes) with at least --min-genes genes on the LCC, alone and with --n-random degree-matched random sets each.
Writes one JSON file (default profiles/steiner_bench.json) and prints it:
  * device-event milliseconds, every one of --reps after one warm-up call, of gss_steiner_trees alone (device tables in place: the
    observed sets with and without the lists, and the whole random-set table in one call without them) and of the whole
    SteinerEngine.trees / .tree_table;
  * the seconds the numpy mirror (tests/steiner_mirror.py) takes on one host core, a host clock: the baseline.  For the observed sets
    the same call; of the null its first --mirror-units units, scaled to the whole table (said so in the file);
  * whether the device's integers equal the mirror's on everything the mirror ran;
  * the quantities of DESIGN.md section 9.20's cost model on this very call: levels, bridges, Steiner nodes per unit.
No pass / fail threshold: the times are recorded.
usage: steiner_bench.py [--fixture FILE] [--reps R] [--n-random R] [--min-genes G] [--mirror-units M] [--out FILE]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import proximity_mirror as PM  # noqa: E402
import steiner_mirror as M  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.proximity import degree_bins  # noqa: E402
from gcn_drug_repurposing_amd.steiner import COUNT_FIELDS, SteinerEngine  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def all_of(fn, reps):
    out, _ = timed(fn)                                            # warm-up: code objects, allocator
    times = []
    for _ in range(reps):
        out, ms = timed(fn)
        times.append(ms)
    return out, times


def spread(times):
    return {"ms": [round(x, 3) for x in times], "median_ms": round(float(np.median(times)), 3),
            "spread": round((max(times) - min(times)) / float(np.median(times)), 3)}


def entry_point(eng, seeds, sizes, max_add=0, lists=False):
    """a closure that calls gss_steiner_trees once on a device seed table, and the buffers it writes"""
    U, width = seeds.shape
    counts = [torch.empty(U, dtype=torch.int32, device="cuda") for _ in COUNT_FIELDS]
    extra = [torch.empty((U, max_add), dtype=torch.int32, device="cuda"), torch.empty((U, max_add), dtype=torch.int32, device="cuda"),
             torch.empty((U, width - 1, 2), dtype=torch.int32, device="cuda")] if lists else [None, None, None]

    def call():
        _lib.check(eng.lib.gss_steiner_trees(eng.net.n, _lib.ptr(eng._rowptr), _lib.ptr(eng._col), eng.max_deg, U, width, _lib.ptr(seeds),
                                             _lib.ptr(sizes), max_add, *(_lib.ptr(x) for x in counts), *(_lib.ptr(x) for x in extra),
                                             _lib.current_stream()), "gss_steiner_trees")

    return call, dict(zip(COUNT_FIELDS, counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default=PM.FIXTURE)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-add", type=int, default=4096)
    ap.add_argument("--n-random", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=452456)
    ap.add_argument("--min-genes", type=int, default=20)
    ap.add_argument("--mirror-units", type=int, default=100, help="units of the null the mirror is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "steiner_bench.json"))
    args = ap.parse_args()
    fx = PM.Fixture(args.fixture)
    net = fx.net
    genes = [s for s in fx.diseases if len(net.node_set(s)) >= args.min_genes]
    sets = [net.node_set(s) for s in genes]
    eng = SteinerEngine(net)
    out = {"n": net.n, "nnz": len(net.col), "max_degree": eng.max_deg, "sets": len(sets), "largest_set": max(len(s) for s in sets),
           "max_add": args.max_add, "n_random": args.n_random, "reps": args.reps, "input": os.path.basename(args.fixture),
           "lds_bytes_observed": 4 * net.n + 16 * max(len(s) for s in sets)}
    # the observed sets
    grown, whole = all_of(lambda: eng.trees(sets, max_add=args.max_add), args.reps)
    seeds, sizes, _ = eng.pack(sets)
    call, bufs = entry_point(eng, seeds, sizes, args.max_add, lists=True)
    _, alone = all_of(call, args.reps)
    bare, _ = entry_point(eng, seeds, sizes)
    _, counts_only = all_of(bare, args.reps)
    assert all(np.array_equal(bufs[f].cpu().numpy(), grown[f]) for f in COUNT_FIELDS)
    t0 = time.perf_counter()
    want = M.table(net.rowptr, net.col, sets)
    seconds = time.perf_counter() - t0
    levels = [int(M.tree(net.rowptr, net.col, s)["dist"].max()) for s in sets]
    n_bridges = [len(M.bridges(net.rowptr, net.col, *M.nearest(net.rowptr, net.col, s)[:2])[0]) for s in sets]
    out["observed"] = {"steiner_trees_with_lists": spread(alone), "steiner_trees_counts_only": spread(counts_only), "engine_trees": spread(whole),
                       "numpy_mirror_seconds": round(seconds, 2), "speedup_engine_over_mirror": round(seconds * 1e3 / float(np.median(whole)), 1),
                       "equal_to_the_mirror": bool(all(np.array_equal(grown[f], want[f]) for f in COUNT_FIELDS)
                                                   and all(np.array_equal(a, b) for f in ("steiner", "parent", "bridge")
                                                           for a, b in zip(grown[f], want[f]))),
                       "steiner_nodes": {"total": int(want["n_steiner"].sum()), "max_unit": int(want["n_steiner"].max()),
                                         "mean_unit": round(float(want["n_steiner"].mean()), 1)},
                       "length": {"total": int(want["length"].sum()), "max_unit": int(want["length"].max())},
                       "trees_per_set_max": int(want["n_comp"].max()),
                       "units_where_the_src_rule_decided": int((want["src_decided"] > 0).sum()),
                       "units_where_the_bridge_order_decided": int((want["order_decided"] > 0).sum())}
    out["cost_model"] = {"levels_max": max(levels), "levels_mean": round(float(np.mean(levels)), 1),
                         "bridges_mean": round(float(np.mean(n_bridges)), 0), "bridges_max": max(n_bridges),
                         "edges": len(net.col) // 2, "longest_bridge": int(want["max_w"].max()),
                         "ms_per_unit_slowest_counts_only": round(float(np.median(counts_only)), 4)}
    # the null: every set and its random sets
    if args.n_random:
        table, whole = all_of(lambda: eng.tree_table(genes, 1, n_random=args.n_random, seed=args.seed, max_add=args.max_add), args.reps)
        nodes, sizes = eng.set_table(sets, 1, args.n_random, args.seed, degree_bins(net.degree, 100))
        flat_nodes, flat_sizes = nodes.reshape(-1, nodes.shape[2]).contiguous(), sizes.reshape(-1).contiguous()
        call, bufs = entry_point(eng, flat_nodes, flat_sizes)
        _, alone = all_of(call, args.reps)
        R = args.n_random + 1
        same = all(np.array_equal(bufs[f].cpu().numpy().reshape(len(sets), R), table[f]) for f in ("n_comp", "length", "n_steiner"))
        units = min(args.mirror_units, flat_nodes.shape[0])
        h_nodes, h_sizes = flat_nodes[:units].cpu().numpy(), flat_sizes[:units].cpu().numpy()
        t0 = time.perf_counter()
        part = M.table(net.rowptr, net.col, [h_nodes[i, :h_sizes[i]] for i in range(units)])
        seconds = time.perf_counter() - t0
        n_steiner = bufs["n_steiner"].cpu().numpy()
        U = int(flat_nodes.shape[0])
        out["null"] = {"units": U, "steiner_trees": spread(alone), "tree_table": spread(whole),
                       "us_per_unit_and_cu": round(float(np.median(alone)) * 1e3 / (U / 256.0), 1),
                       "one_call_equals_the_chunked_table": bool(same),
                       "numpy_mirror": {"units": units, "seconds": round(seconds, 2), "seconds_scaled_to_all_units": round(seconds * U / units, 1),
                                        "note": "one host core, a host clock; the first units of the table (the first sets' samples), scaled by the unit count"},
                       "equal_to_the_mirror_on_those_units": bool(all(np.array_equal(bufs[f][:units].cpu().numpy(), part[f]) for f in COUNT_FIELDS)),
                       "steiner_nodes": {"max_unit": int(n_steiner.max()), "mean_unit": round(float(n_steiner.mean()), 2)},
                       "sets_with_steiner_q_below_0.05": int(np.sum(table["steiner_stats"]["q"] <= 0.05)),
                       "sets_with_length_q_below_0.05": int(np.sum(table["length_stats"]["q"] <= 0.05)),
                       "steiner_observed_mean": round(float(table["n_steiner"][:, 0].mean()), 2),
                       "steiner_null_mean": round(float(np.nanmean(table["steiner_stats"]["mean"])), 2)}
    eng.close()
    out["device"] = torch.cuda.get_device_name(0)
    out["source_hashes"] = {k: v for k, v in _lib.source_hashes().items()
                            if k in ("steiner.hip", "seed_units.h", "lds_union_find.h", "proximity.hip", "device_scope.h", "common.h", "*")}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
