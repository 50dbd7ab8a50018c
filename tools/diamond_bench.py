#!/usr/bin/env python3
"""DIAMOnD at the reference's size, from tests/golden/proximity_2016.npz: the 78 disease gene sets of the 2016 network (LCC 13,329
nodes), 200 nodes added to each in one call.  Writes one JSON file (default profiles/diamond_bench.json) and prints it:
  * device-event milliseconds, every one of --reps after one warm-up call, of gss_diamond_grow alone (device tables in place) and of the
    whole DiamondEngine.grow (uploads of the seed table, the launch, the copies back, p on the host);
  * the seconds the numpy mirror (tests/diamond_mirror.py) takes for the same call on one host core, a host clock: the baseline.  The
    mirror is written for clarity, one Python statement per operation of the tail sum;
  * whether the device's nodes equal the mirror's, and how many steps have a runner-up closer than 1e-9 (there the winner is
    implementation-defined, include/gssgcn.h);
  * the quantities of DESIGN.md section 9.18's cost model on this very call: per unit the sum over its steps of the step's longest tail
    sum (the chain one lane walks while the workgroup waits), and the rows walked.
No pass / fail threshold: the times are recorded.  usage: diamond_bench.py [--reps R] [--n-add K] [--alpha A] [--mirror-sets M] [--out FILE]"""
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

import diamond_mirror as M  # noqa: E402
import proximity_mirror as PM  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diamond import DiamondEngine  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-add", type=int, default=200)
    ap.add_argument("--alpha", type=int, default=1)
    ap.add_argument("--mirror-sets", type=int, default=None, help="time the mirror on the first M sets only (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diamond_bench.json"))
    args = ap.parse_args()
    fx = PM.Fixture()
    net = fx.net
    sets = [net.node_set(s) for s in fx.diseases]
    eng = DiamondEngine(net)
    U, width = len(sets), max(len(s) for s in sets)
    out = {"n": net.n, "nnz": len(net.col), "max_degree": eng.max_deg, "sets": U, "largest_set": width, "n_add": args.n_add, "alpha": args.alpha,
           "reps": args.reps}
    res, whole = all_of(lambda: eng.grow(sets, n_add=args.n_add, alpha=args.alpha), args.reps)
    # the entry point alone, on device tables built once
    d_seeds, d_sizes, _ = eng.pack(sets)
    lg = eng._table(net.n + (args.alpha - 1) * width + 2)
    ints = [torch.empty((U, args.n_add), dtype=torch.int32, device="cuda") for _ in range(3)]
    reals = [torch.empty((U, args.n_add), dtype=torch.float64, device="cuda") for _ in range(3)]

    def call():
        _lib.check(eng.lib.gss_diamond_grow(net.n, _lib.ptr(eng._rowptr), _lib.ptr(eng._col), eng.max_deg, _lib.ptr(lg), len(lg), U, width,
                                            _lib.ptr(d_seeds), _lib.ptr(d_sizes), args.n_add, args.alpha, *(_lib.ptr(x) for x in ints),
                                            *(_lib.ptr(x) for x in reals), _lib.current_stream()), "gss_diamond_grow")

    _, alone = all_of(call, args.reps)
    assert np.array_equal(ints[0].cpu().numpy(), res["node"])
    eng.close()
    out["gpu"] = {"diamond_grow_ms": [round(x, 3) for x in alone], "diamond_grow_ms_median": round(float(np.median(alone)), 3),
                  "engine_grow_ms": [round(x, 3) for x in whole], "engine_grow_ms_median": round(float(np.median(whole)), 3),
                  "note": "device events around the call; the entry point ends in its status read-back"}
    m_sets = sets if args.mirror_sets is None else sets[:args.mirror_sets]
    t0 = time.perf_counter()
    want = M.table(net.rowptr, net.col, m_sets, args.n_add, args.alpha)
    seconds = time.perf_counter() - t0
    live = want["node"] >= 0
    close = int((np.where(live, want["gap"], np.inf) <= 1e-9).sum())
    chain = want["terms"].sum(axis=1)
    rows = np.diff(net.rowptr)[np.where(live, want["node"], 0)] * live
    out["numpy_mirror"] = {"sets": len(m_sets), "seconds": round(seconds, 2), "seconds_per_set": round(seconds / len(m_sets), 3),
                           "note": "one host core, a host clock"}
    out["against_the_mirror"] = {"nodes_equal": bool(np.array_equal(res["node"][:len(m_sets)], want["node"])), "steps": int(live.sum()),
                                 "steps_with_a_runner_up_within_1e-9": close, "lt0_bits_equal": bool(np.array_equal(res["lt0"][:len(m_sets)], want["lt0"])),
                                 "S_bits_equal": bool(np.array_equal(res["S"][:len(m_sets)], want["S"]))}
    out["cost_model"] = {"scanned_words_per_step": net.n, "longest_tail_terms_summed_over_steps_max_unit": int(chain.max()),
                         "longest_tail_terms_summed_over_steps_mean_unit": round(float(chain.mean()), 1),
                         "longest_single_tail": int(want["terms"].max()), "winner_row_entries_max_unit": int(rows.sum(axis=1).max()),
                         "largest_kb": int(want["kb"].max())}
    if args.mirror_sets is None:
        out["speedup_engine_over_mirror"] = round(seconds * 1e3 / float(np.median(whole)), 1)
    out["device"] = torch.cuda.get_device_name(0)
    out["source_hashes"] = {k: v for k, v in _lib.source_hashes().items() if k in ("diamond.hip", "seed_units.h", "device_scope.h", "common.h", "*")}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
