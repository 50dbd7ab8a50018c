#!/usr/bin/env python3
"""The seed connector algorithm at the reference's size, from --fixture (default tests/golden/proximity_2016.npz): the disease gene
sets of the 2016 network (LCC 13,329 nodes) with at least --min-genes genes on the LCC, up to --n-add connectors each, alone and with
--n-random degree-matched random sets each.  Writes one JSON file (default profiles/connectors_bench.json) and prints it:
  * device-event milliseconds, every one of --reps after one warm-up call, of gss_seed_connectors alone (device tables in place: the
    observed sets, and the whole random-set table in one call) and of the whole ConnectorEngine.grow / .connector_table;
  * the seconds the numpy mirror (tests/connectors_mirror.py) takes on one host core, a host clock: the baseline.  For the observed sets
    the same call; of the null its first --mirror-units units, scaled to the whole table (said so in the file);
  * whether the device's integers equal the mirror's on everything the mirror ran;
  * the quantities of DESIGN.md section 9.19's cost model on this very call: per step the candidates, the CSR entries of their rows and
    the most components next to one candidate, and the steps per unit.
No pass / fail threshold: the times are recorded.
usage: connectors_bench.py [--fixture FILE] [--reps R] [--n-add K] [--n-random R] [--min-genes G] [--mirror-units M] [--out FILE]"""
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

import connectors_mirror as M  # noqa: E402
import proximity_mirror as PM  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.connectors import STEP_FIELDS, UNIT_FIELDS, ConnectorEngine  # noqa: E402
from gcn_drug_repurposing_amd.proximity import degree_bins  # noqa: E402


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


def entry_point(eng, seeds, sizes, n_add):
    """a closure that calls gss_seed_connectors once on a device seed table, and the buffers it writes"""
    U, width = seeds.shape
    step = [torch.empty((U, n_add), dtype=torch.int32, device="cuda") for _ in STEP_FIELDS]
    unit = [torch.empty(U, dtype=torch.int32, device="cuda") for _ in UNIT_FIELDS]

    def call():
        _lib.check(eng.lib.gss_seed_connectors(eng.net.n, _lib.ptr(eng._rowptr), _lib.ptr(eng._col), eng.max_deg, U, width, _lib.ptr(seeds),
                                               _lib.ptr(sizes), n_add, *(_lib.ptr(x) for x in step), *(_lib.ptr(x) for x in unit), None,
                                               _lib.current_stream()), "gss_seed_connectors")

    return call, dict(zip(STEP_FIELDS + UNIT_FIELDS, step + unit))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fixture", default=PM.FIXTURE)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-add", type=int, default=500)
    ap.add_argument("--n-random", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=452456)
    ap.add_argument("--min-genes", type=int, default=20)
    ap.add_argument("--mirror-units", type=int, default=300, help="units of the null the mirror is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connectors_bench.json"))
    args = ap.parse_args()
    fx = PM.Fixture(args.fixture)
    net = fx.net
    genes = [s for s in fx.diseases if len(net.node_set(s)) >= args.min_genes]
    sets = [net.node_set(s) for s in genes]
    eng = ConnectorEngine(net)
    out = {"n": net.n, "nnz": len(net.col), "max_degree": eng.max_deg, "sets": len(sets), "largest_set": max(len(s) for s in sets),
           "n_add": args.n_add, "n_random": args.n_random, "reps": args.reps, "input": os.path.basename(args.fixture)}
    # the observed sets
    grown, whole = all_of(lambda: eng.grow(sets, n_add=args.n_add), args.reps)
    seeds, sizes, _ = eng.seed_table(sets)
    call, bufs = entry_point(eng, seeds, sizes, args.n_add)
    _, alone = all_of(call, args.reps)
    assert all(np.array_equal(bufs[f].cpu().numpy(), grown[f]) for f in STEP_FIELDS + UNIT_FIELDS)
    t0 = time.perf_counter()
    want = M.table(net.rowptr, net.col, sets, args.n_add)
    seconds = time.perf_counter() - t0
    live = want["node"] >= 0
    out["observed"] = {"seed_connectors": spread(alone), "engine_grow": spread(whole),
                       "numpy_mirror_seconds": round(seconds, 2), "speedup_engine_over_mirror": round(seconds * 1e3 / float(np.median(whole)), 1),
                       "equal_to_the_mirror": bool(all(np.array_equal(grown[f], want[f]) for f in STEP_FIELDS + UNIT_FIELDS)
                                                   and all(np.array_equal(a, b) for a, b in zip(grown["label"], want["label"]))),
                       "steps": {"total": int(live.sum()), "max_unit": int(want["steps"].max()), "mean_unit": round(float(want["steps"].mean()), 1)},
                       "seeds_joined_of_genes": [int(grown["seeds_in"].sum()), int(sum(len(s) for s in sets))],
                       "steps_decided_by_degree": int((live & (want["ties_lcc"] > want["ties_deg"]) & (want["ties_deg"] == 1)).sum()),
                       "steps_decided_by_node_index": int((live & (want["ties_deg"] > 1)).sum())}
    out["cost_model"] = {"scanned_words_per_step": net.n, "candidates_per_step_max": int(want["candidates"].max()),
                         "row_entries_per_step_max": int(want["entries"].max()),
                         "row_entries_per_step_mean": round(float(want["entries"][live].mean()), 1) if live.any() else 0.0,
                         "row_entries_summed_over_steps_max_unit": int(want["entries"].sum(axis=1).max()),
                         "most_components_next_to_one_candidate": int(want["most_merged"].max()),
                         "ms_per_step_slowest_unit": round(float(np.median(alone)) / max(int(want["steps"].max()) + 1, 1), 4)}
    # the null: every set and its random sets
    if args.n_random:
        table, whole = all_of(lambda: eng.connector_table(genes, 1, n_add=args.n_add, n_random=args.n_random, seed=args.seed), args.reps)
        nodes, sizes = eng.set_table(sets, 1, args.n_random, args.seed, degree_bins(net.degree, 100))
        flat_nodes, flat_sizes = nodes.reshape(-1, nodes.shape[2]).contiguous(), sizes.reshape(-1).contiguous()
        call, bufs = entry_point(eng, flat_nodes, flat_sizes, args.n_add)
        _, alone = all_of(call, args.reps)
        R = args.n_random + 1
        same = all(np.array_equal(bufs[f].cpu().numpy().reshape(len(sets), R), table[f]) for f in ("steps", "final_lcc", "seeds_in"))
        units = min(args.mirror_units, flat_nodes.shape[0])
        h_nodes, h_sizes = flat_nodes[:units].cpu().numpy(), flat_sizes[:units].cpu().numpy()
        t0 = time.perf_counter()
        part = M.table(net.rowptr, net.col, [h_nodes[i, :h_sizes[i]] for i in range(units)], args.n_add)
        seconds = time.perf_counter() - t0
        steps = bufs["steps"].cpu().numpy()
        out["null"] = {"units": int(flat_nodes.shape[0]), "seed_connectors": spread(alone), "connector_table": spread(whole),
                       "one_call_equals_the_chunked_table": bool(same),
                       "numpy_mirror": {"units": units, "seconds": round(seconds, 2),
                                        "seconds_scaled_to_all_units": round(seconds * flat_nodes.shape[0] / units, 1),
                                        "note": "one host core, a host clock; the first units of the table (the first sets' samples), scaled by the unit count"},
                       "equal_to_the_mirror_on_those_units": bool(all(np.array_equal(bufs[f][:units].cpu().numpy(), part[f])
                                                                      for f in STEP_FIELDS + UNIT_FIELDS)),
                       "steps": {"total": int(steps.sum()), "max_unit": int(steps.max()), "mean_unit": round(float(steps.mean()), 2)},
                       "sets_with_joined_q_below_0.05": int(np.sum(table["joined_stats"]["q"] <= 0.05)),
                       "connectors_observed_mean": round(float(table["connectors"].mean()), 2),
                       "connectors_null_mean": round(float(np.nanmean(table["connectors_null_mean"])), 2)}
    eng.close()
    out["device"] = torch.cuda.get_device_name(0)
    out["source_hashes"] = {k: v for k, v in _lib.source_hashes().items()
                            if k in ("seed_connect.hip", "seed_units.h", "lds_union_find.h", "proximity.hip", "device_scope.h", "common.h", "*")}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
