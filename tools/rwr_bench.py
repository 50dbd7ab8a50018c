#!/usr/bin/env python3
"""The random walk with restart at the reference's size, from tests/golden/proximity_2016.npz: the 78 disease gene sets of the 2016
network (LCC 13,329 nodes), alone and with --n-random (1,000) degree-matched random sets each.  Writes one JSON file (default
profiles/rwr_bench.json) and prints it:
  * device-event milliseconds, the best and every one of --reps after one warm-up call, of gss_rwr_rank alone on the 78 sets (device
    tables in place) and of the whole RwrEngine.rank (uploads, the launch, the copies back);
  * the same for the null: the entry points alone (gss_rwr_rank with p_out and gss_rwr_null_stats, batch by batch on device tables in
    place, the two summed separately) and the whole RwrEngine.score_table (the random sets drawn, the batches, the copies back);
  * the seconds a scipy.sparse fp64 iteration of the same units takes on one host core (a host clock): the 78 sets, and the units of
    the first --host-sets sets of the null, scaled to all of them and said so;
  * whether the device's ranks, scores and iteration counts equal the mirror's (tests/rwr_mirror.py).
No pass / fail threshold: the times are recorded.  usage: rwr_bench.py [--reps R] [--n-random K] [--restart r] [--host-sets M] [--out FILE]"""
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
import rwr_mirror as M  # noqa: E402
from gcn_drug_repurposing_amd import _lib, proximity as P  # noqa: E402
from gcn_drug_repurposing_amd.rwr import SCRATCH_BYTES, RwrEngine  # noqa: E402


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


def report(times):
    return {"ms_best": round(min(times), 3), "ms": [round(x, 3) for x in times]}


def host_iteration(net, units, restart, tol, max_iter):
    """scipy.sparse, fp64, one core: p <- (1 - r) W p + r p0 on all units side by side until every one has err < tol -> (seconds, iterations)"""
    import scipy.sparse as sp
    deg = np.diff(net.rowptr).astype(np.float64)
    W = sp.csr_matrix((np.ones(len(net.col)), net.col, net.rowptr), shape=(net.n, net.n)) @ sp.diags(1.0 / deg)
    p0 = np.zeros((net.n, len(units)))
    for u, s in enumerate(units):
        if len(s):
            p0[s, u] = 1.0 / len(s)
    t0 = time.perf_counter()
    p, it = p0.copy(), 0
    while it < max_iter:
        it += 1
        new = (1.0 - restart) * (W @ p) + restart * p0
        err = np.abs(new - p).sum(axis=0).max()
        p = new
        if err < tol:
            break
    return time.perf_counter() - t0, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-add", type=int, default=200)
    ap.add_argument("--n-random", type=int, default=1000)
    ap.add_argument("--restart", type=float, default=0.75)
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=452456)
    ap.add_argument("--host-sets", type=int, default=2, help="sets whose null units the host iteration walks (scaled to all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rwr_bench.json"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    fx = PM.Fixture()
    net = fx.net
    sets = [net.node_set(s) for s in fx.diseases]
    eng = RwrEngine(net)
    n, U, width, R = net.n, len(sets), max(len(s) for s in sets), args.n_random + 1
    walk = dict(restart=args.restart, tol=args.tol, max_iter=args.max_iter)
    out = {"n": n, "nnz": len(net.col), "max_degree": eng.max_deg, "rows_longer_than_32": int((np.diff(net.rowptr) > M.LONG_ROW).sum()), "sets": U,
           "largest_set": width, "n_add": args.n_add, "n_random": args.n_random, "reps": args.reps, **walk}
    # ---- the 78 sets alone
    res, whole = all_of(lambda: eng.rank(sets, n_add=args.n_add, **walk), args.reps)
    d_nodes, d_sizes, _ = eng.pack(sets)
    node = torch.empty((U, args.n_add), dtype=torch.int32, device="cuda")
    score = torch.empty((U, args.n_add), dtype=torch.float64, device="cuda")
    iters = torch.empty(U, dtype=torch.int32, device="cuda")

    def rank_call(nodes, sizes, units, node, score, iters, p):
        _lib.check(eng.lib.gss_rwr_rank(n, _lib.ptr(eng._rowptr), _lib.ptr(eng._col), eng.max_deg, units, nodes.shape[-1], _lib.ptr(nodes),
                                        _lib.ptr(sizes), args.restart, args.tol, args.max_iter, args.n_add, _lib.ptr(node), _lib.ptr(score),
                                        _lib.ptr(iters), _lib.ptr(p), _lib.current_stream()), "gss_rwr_rank")

    _, alone = all_of(lambda: rank_call(d_nodes, d_sizes, U, node, score, iters, None), args.reps)
    assert np.array_equal(node.cpu().numpy(), res["node"])
    want = M.table(net.rowptr, net.col, sets, args.n_add, args.restart, args.tol, args.max_iter)
    out["sets_alone"] = {"gss_rwr_rank": report(alone), "engine_rank": report(whole),
                         "iterations": [int(res["iters"].min()), int(res["iters"].max())],
                         "equal_to_the_mirror": bool(np.array_equal(res["node"], want["node"]) and np.array_equal(res["iters"], want["iters"])
                                                     and np.array_equal(res["score"].view(np.int64), want["score"].view(np.int64))),
                         "note": "device events around the call; the entry point ends in its status read-back"}
    seconds, it = host_iteration(net, sets, **walk)
    out["sets_alone"]["scipy_one_core"] = {"seconds": round(seconds, 3), "iterations": it, "note": "a host clock; all units iterate until the last has err < tol"}
    # ---- with the null
    if args.n_random:
        genes = fx.diseases
        table, whole = all_of(lambda: eng.score_table(genes, 1, n_random=args.n_random, seed=args.seed, n_add=args.n_add, **walk), args.reps)
        t_nodes, t_sizes = eng.set_table(sets, 1, args.n_random, args.seed, P.degree_bins(net.degree, 100))
        t_nodes, t_sizes = t_nodes.contiguous(), t_sizes.contiguous()
        batch = max(1, SCRATCH_BYTES // (R * n * 8))
        p = torch.empty((batch, R, n), dtype=torch.float64, device="cuda")
        mean, sd, z = (torch.empty((batch, n), dtype=torch.float64, device="cuda") for _ in range(3))
        ge = torch.empty((batch, n), dtype=torch.int32, device="cuda")
        top = torch.empty((batch, args.n_add), dtype=torch.int32, device="cuda")
        its = torch.empty(batch * R, dtype=torch.int32, device="cuda")
        ms = t_nodes.shape[2]

        def null_calls():
            walk_ms = stats_ms = 0.0
            for s0 in range(0, U, batch):
                b = min(batch, U - s0)
                _, t = timed(lambda: rank_call(t_nodes[s0:s0 + b].reshape(b * R, ms), t_sizes[s0:s0 + b].reshape(b * R), b * R, None, None, its, p))
                walk_ms += t
                _, t = timed(lambda: _lib.check(eng.lib.gss_rwr_null_stats(n, b, R, _lib.ptr(p), ms, _lib.ptr(t_nodes[s0:]), _lib.ptr(t_sizes[s0:]),
                                                                           args.n_add, 0, _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(z), _lib.ptr(ge),
                                                                           _lib.ptr(top), _lib.current_stream()), "gss_rwr_null_stats"))
                stats_ms += t
            return walk_ms, stats_ms

        null_calls()
        pairs = [null_calls() for _ in range(args.reps)]
        out["with_null"] = {"units": U * R, "sets_per_batch": batch, "batches": -(-U // batch), "vector_bytes_per_set": R * n * 8,
                            "gss_rwr_rank_all_batches": report([a for a, _ in pairs]), "gss_rwr_null_stats_all_batches": report([b for _, b in pairs]),
                            "engine_score_table": report(whole),
                            "note": "the entry points: device events around each call, summed over the batches; the engine call also draws the random sets"}
        m = min(args.host_sets, U)
        t_host = t_nodes[:m].cpu().numpy()
        z_host = t_sizes[:m].cpu().numpy()
        units = [t_host[s, k, :z_host[s, k]] for s in range(m) for k in range(R)]
        seconds, it = host_iteration(net, units, **walk)
        out["with_null"]["scipy_one_core"] = {"sets_walked": m, "units_walked": len(units), "seconds": round(seconds, 2), "iterations": it,
                                              "seconds_scaled_to_all_units": round(seconds * U / m, 1),
                                              "note": "a host clock; measured on the first sets' units and scaled by the number of sets, not measured whole"}
    eng.close()
    out["device"] = torch.cuda.get_device_name(0)
    out["source_hashes"] = {k: v for k, v in _lib.source_hashes().items() if k in ("rwr.hip", "rank_keys.h", "seed_units.h", "device_scope.h", "common.h", "*")}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
