#!/usr/bin/env python3
"""Shortest-path counts, best paths and the between pass (csrc/trace.hip) on the 29,960-node whole-graph stand-in, by device events
(2 warm-ups, median of --reps): one pass toward 64 targets (NodeCovid + 63 indications) as distances alone, then counts, then counts +
best path, with the time per level launch; the mediators of those 64 targets over all 1,661 drugs (26 passes of sources) end to end
and by stage; the interpret.py stages' wall time on the small fixture; and networkx's full enumeration (nx.all_shortest_paths) on a
sample of (drug, target) pairs of the stand-in, with the extrapolation to every pair marked as one.
Writes profiles/trace_bench.json.   python tools/trace_bench.py [--reps 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, reps):
    """device-event milliseconds of fn(), after 2 warm-ups -> list"""
    import torch
    out = []
    for r in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if r >= 2:
            out.append(e0.elapsed_time(e1))
    return out


def stats(times, **more):
    return dict(ms_median=float(np.median(times)), ms_min=float(np.min(times)), reps=len(times), **more)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nx-sample", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_bench.json"))
    a = ap.parse_args()
    import torch
    from paths_bench import standin
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd.trace import MAX_TARGETS, PathTracer
    hashes = _lib.source_hashes()
    out = {"graph": "synth.standin_tables(seed=1) through MsiGraph", "source_hash": {k: hashes[k] for k in ("paths.hip", "trace.hip")}}
    with tempfile.TemporaryDirectory() as tmp:
        g = standin(tmp)
    adj, names, types = g.to_csr()
    n = adj.shape[0]
    out["nodes"], out["entries"] = int(n), int(adj.nnz)
    idx = {x: i for i, x in enumerate(names)}
    inds = [idx[x] for x in g.indications_in_graph if x != "NodeCovid"]
    targets = np.asarray([idx["NodeCovid"]] + inds[:63], np.int32)
    drugs = np.asarray([idx[x] for x in g.drugs_in_graph], np.int32)
    lib = _lib.load()
    tr = PathTracer(adj)
    pt = tr._pass("toward", True)
    ps = tr._pass("from", False)
    w = np.random.RandomState(7).randn(len(targets), n)
    pt.w[:len(targets)].copy_(torch.from_numpy(w))
    st = _lib.current_stream
    lv = C.c_int32(0)
    q = len(targets)

    def run_dist(p=pt, nodes=targets):
        _lib.check(lib.gss_paths_run(p.h, len(nodes), nodes.ctypes.data, _lib.ptr(p.dist), _lib.ptr(p.next), C.byref(lv), st()))

    def run_count(weighted, p=pt, nodes=targets):
        _lib.check(lib.gss_paths_count(p.h, len(nodes), nodes.ctypes.data, _lib.ptr(p.dist), lv.value, _lib.ptr(p.w if weighted else None),
                                       _lib.ptr(p.sigma), _lib.ptr(p.best if weighted else None), _lib.ptr(p.best_next if weighted else None), st()))

    run_dist()
    levels = int(lv.value)
    t_dist = timed(run_dist, a.reps)
    t_count = timed(lambda: run_count(False), a.reps)
    t_best = timed(lambda: run_count(True), a.reps)
    out["toward_64_targets"] = {
        "levels": levels,
        "distances": stats(t_dist, level_launches=levels + 1, ms_per_level_launch=float(np.median(t_dist)) / (levels + 1)),
        "counts": stats(t_count, level_launches=levels, other_launches=2, ms_per_launch=float(np.median(t_count)) / (levels + 2)),
        "counts_and_best_path": stats(t_best, level_launches=levels, other_launches=2, ms_per_launch=float(np.median(t_best)) / (levels + 2)),
        "sigma_max": float(pt.sigma[:q].max().item()),
    }
    print("toward", out["toward_64_targets"])
    # one pass of 64 sources against the 64 targets, by stage
    dev = torch.device("cuda")
    d_len = torch.empty((64, 64), dtype=torch.int32, device=dev)
    d_paths = torch.empty((64, 64), dtype=torch.float64, device=dev)
    d_nodes = torch.empty((64, 64), dtype=torch.int32, device=dev)
    d_M = torch.zeros((q, n), dtype=torch.float64, device=dev)
    d_C = torch.zeros((q, n), dtype=torch.int32, device=dev)
    src = np.ascontiguousarray(drugs[:64])
    run_dist(ps, src)
    run_count(False, ps, src)
    run_dist()
    run_count(True)

    def run_between(med):
        _lib.check(lib.gss_paths_between(n, len(src), src.ctypes.data, _lib.ptr(ps.dist), _lib.ptr(ps.sigma), q, targets.ctypes.data, _lib.ptr(pt.dist),
                                         _lib.ptr(pt.sigma), _lib.ptr(d_len), _lib.ptr(d_paths), _lib.ptr(d_nodes), _lib.ptr(d_M if med else None),
                                         _lib.ptr(d_C if med else None), st()))

    t_pairs = timed(lambda: run_between(False), a.reps)
    t_both = timed(lambda: run_between(True), a.reps)
    out["between_64x64"] = {"pair_table": stats(t_pairs), "pair_table_and_mediators": stats(t_both),
                            "pair_node_tests": int(64 * 64 * n)}
    print("between", out["between_64x64"])
    # the mediators of the 64 targets over every drug, end to end (host wall clock around the whole call, the read-backs included)
    walls = []
    for r in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = tr.between(drugs, targets, pairs=None, weights=w, mediators=True)
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    out["mediators_64_targets_all_drugs"] = {
        "drugs": int(len(drugs)), "source_passes": -(-len(drugs) // MAX_TARGETS), "wall_s_runs": walls, "wall_s_best": min(walls),
        "pairs": int(res.length.size), "pairs_unreachable": int((res.length < 0).sum()), "paths_max": float(res.n_paths.max()),
        "paths_median": float(np.median(res.n_paths)), "nodes_on_paths_max": int(res.n_nodes.max()), "mediator_nodes": int((res.mediators[1] > 0).sum())}
    print("mediators", out["mediators_64_targets_all_drugs"])
    tr.close()
    # the CLI on the small fixture, by stage (wall time, one run after a warm-up run)
    import predict_fixture as F
    from gcn_drug_repurposing_amd import interpret, predict
    for r in range(2):
        with tempfile.TemporaryDirectory() as tmp:
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                s = predict.Settings(predict.load_config(F.stage(tmp, "gcn")))
                tm = {}
                t0 = time.perf_counter()
                interpret.run(s, nodes="nodes.tsv", edges="edges.tsv", mediators="mediators.tsv", timings=tm)
                tm["total_s"] = time.perf_counter() - t0
            finally:
                os.chdir(cwd)
    out["cli_fixture_gcn_all_tables_s"] = tm
    print("cli", tm)
    try:
        import networkx as nx
    except ImportError:
        out["networkx"] = "not importable here: no speedup quoted"
    else:
        G = nx.DiGraph()
        G.add_nodes_from(range(n))
        rows = np.repeat(np.arange(n), np.diff(adj.indptr))
        G.add_edges_from(zip(rows.tolist(), adj.indices.tolist()))
        rng = np.random.RandomState(0)
        sample = [(int(drugs[rng.randint(len(drugs))]), int(targets[rng.randint(q)])) for _ in range(a.nx_sample)]
        t0 = time.perf_counter()
        total = 0
        for s_, t_ in sample:
            try:
                total += sum(1 for _ in nx.all_shortest_paths(G, s_, t_))
            except nx.NetworkXNoPath:
                pass
        per = (time.perf_counter() - t0) / len(sample)
        out["networkx"] = {"all_shortest_paths_ms_per_pair_sample_mean": per * 1e3, "sample": len(sample), "paths_enumerated": total,
                           f"extrapolated_{len(drugs)}x{q}_pairs_s": per * len(drugs) * q,
                           "note": "extrapolated from the sample, not timed in full; enumeration only, without the per-node shares"}
        print("networkx", out["networkx"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
