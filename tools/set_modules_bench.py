#!/usr/bin/env python3
"""The module check at the reference's size, from tests/golden/proximity_2016.npz: the 78 disease gene sets and the 238 drug target sets
of the 2016 network (LCC 13,329 nodes), each with 1,000 degree-matched random sets (78,078 and 238,238 units).  Writes one JSON file
(default profiles/set_modules_bench.json) and prints it: device-event milliseconds, best of --reps after one warm-up call of every
shape, of gss_random_sets, gss_set_components and the whole ModuleEngine.module_table (which ends in its copies to the host, so the
events bracket everything), with the cost model of DESIGN.md section 9.17 evaluated on the very tables that were timed: probes = sum
over units of sum over members of min(deg * log2 m, m * log2 deg) (the logarithms rounded up as the kernel rounds them), the CSR entries
the walked rows hold, and the rates they give.  The numpy / scipy version of the disease job took 31 s on one host core (not measured
here).  usage: set_modules_bench.py [--reps R] [--out FILE]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import proximity_mirror as PM  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd import proximity as P  # noqa: E402
from gcn_drug_repurposing_amd.set_modules import ModuleEngine  # noqa: E402

SEED, N_RANDOM, MIN_BIN = 452456, 1000, 100


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def best_of(fn, reps):
    out, _ = timed(fn)                                            # warm-up: code objects, allocator
    times = []
    for _ in range(reps):
        out, ms = timed(fn)
        times.append(ms)
    return out, min(times), times


def lg(x):
    """ceil(log2 x), at least 1: the kernel's ilog2_ceil"""
    x = np.maximum(np.asarray(x, np.int64), 1)
    return np.maximum(1, np.ceil(np.log2(x)).astype(np.int64))


def cost_model(net, nodes, sizes):
    """probes and walked CSR entries of a set table (host arrays), by the kernel's own choice of direction per member"""
    deg_of = np.diff(net.rowptr).astype(np.int64)
    m = np.repeat(sizes.reshape(-1), sizes.reshape(-1))          # per member: its unit's size
    flat = nodes.reshape(-1, nodes.shape[-1])
    keep = np.arange(nodes.shape[-1])[None, :] < sizes.reshape(-1, 1)
    deg = deg_of[flat[keep]]
    walk, search = deg * lg(m), m * lg(deg)
    by_row = (walk <= search) & (deg > 0)
    return {"units": int(sizes.size), "members": int(m.size), "probes": int(np.where(deg > 0, np.minimum(walk, search), 0).sum()),
            "members_walking_their_row": int(by_row.sum()), "row_entries_walked": int(deg[by_row].sum()),
            "row_entries_of_all_members": int(deg.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_modules_bench.json"))
    args = ap.parse_args()
    fx = PM.Fixture()
    net = fx.net
    eng = ModuleEngine(net)
    bins = P.degree_bins(net.degree, MIN_BIN)
    out = {"n": net.n, "nnz": len(net.col), "max_degree": int(np.diff(net.rowptr).max()), "n_random": N_RANDOM, "seed": SEED, "reps": args.reps,
           "host_numpy_scipy_s_one_core_diseases": 31.0}
    for what, side, gene_sets in (("diseases", 1, fx.diseases), ("drugs", 0, fx.drugs)):
        sets = [net.node_set(s) for s in gene_sets]
        (nodes, sizes), rs, rs_all = best_of(lambda: eng.set_table(sets, side, N_RANDOM, SEED, bins), args.reps)
        _, comp, comp_all = best_of(lambda: eng.components(nodes, sizes), args.reps)
        _, lab, _ = best_of(lambda: eng.components(nodes, sizes, labels=True), args.reps)
        _, whole, whole_all = best_of(lambda: eng.module_table(gene_sets, side, n_random=N_RANDOM, seed=SEED, min_bin_size=MIN_BIN), args.reps)
        model = cost_model(net, nodes.cpu().numpy(), sizes.cpu().numpy())
        out[what] = dict(model, sets=len(sets), max_size=int(nodes.shape[2]), random_sets_ms=round(rs, 3), random_sets_ms_all=[round(x, 3) for x in rs_all],
                         set_components_ms=round(comp, 3), set_components_ms_all=[round(x, 3) for x in comp_all],
                         set_components_with_labels_ms=round(lab, 3), module_table_ms=round(whole, 3),
                         module_table_ms_all=[round(x, 3) for x in whole_all],
                         probes_per_s=model["probes"] / comp * 1e3, units_per_s=model["units"] / comp * 1e3)
    eng.close()
    out["device"] = torch.cuda.get_device_name(0)
    out["source_hashes"] = {k: v for k, v in _lib.source_hashes().items() if k in ("set_modules.hip", "seed_units.h", "lds_union_find.h", "proximity.hip", "*")}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
