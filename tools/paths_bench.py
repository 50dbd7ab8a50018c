#!/usr/bin/env python3
"""Shortest-path trees (csrc/paths.hip) on the 29,960-node whole-graph stand-in: device-event time per pass for 1 target (NodeCovid)
and for 64 targets (NodeCovid + 63 indications), the levels each took and the mean time per level; the predict_drug.py stages' wall
time on the small fixture; and networkx's one-search-per-row cost on the stand-in, timed on a sample of the proteins when networkx imports
(no speedup is quoted otherwise).  Writes profiles/paths_bench.json.   python tools/paths_bench.py [--reps 20]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def standin(tmp):
    from gcn_drug_repurposing_amd import synth
    from gcn_drug_repurposing_amd.msi import MsiGraph
    files = {}
    for name, rows in synth.standin_tables(seed=1).items():
        files[name] = os.path.join(tmp, name + ".tsv")
        with open(files[name], "w") as f:
            f.write("node_1\tnode_2\n")
            f.writelines(f"{a}\t{b}\n" for a, b in rows)
    return MsiGraph().load(files)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nx-sample", type=int, default=300)
    a = ap.parse_args()
    import torch
    from gcn_drug_repurposing_amd import _lib
    from gcn_drug_repurposing_amd.paths import ShortestPathTrees
    out = {"graph": "synth.standin_tables(seed=1) through MsiGraph", "source_hash": _lib.source_hashes()["paths.hip"]}
    with tempfile.TemporaryDirectory() as tmp:
        g = standin(tmp)
    adj, names, types = g.to_csr()
    out["nodes"], out["entries"] = int(adj.shape[0]), int(adj.nnz)
    idx = {n: i for i, n in enumerate(names)}
    inds = [idx[n] for n in g.indications_in_graph if n != "NodeCovid"]
    trees = ShortestPathTrees(adj)
    import ctypes as C
    lib = _lib.load()
    for label, targets in (("1_target", [idx["NodeCovid"]]), ("64_targets", [idx["NodeCovid"]] + inds[:63])):
        t = np.asarray(targets, np.int32)
        dist = torch.empty((len(t), adj.shape[0]), dtype=torch.uint8, device="cuda")
        nxt = torch.empty((len(t), adj.shape[0]), dtype=torch.int32, device="cuda")
        lv = C.c_int32(0)
        times = []
        for r in range(a.reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.gss_paths_run(trees._h, len(t), t.ctypes.data, _lib.ptr(dist), _lib.ptr(nxt), C.byref(lv), _lib.current_stream()))
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                times.append(e0.elapsed_time(e1))
        ms = float(np.median(times))
        launches = lv.value + 1        # the last level finds nothing and ends the search
        out[label] = {"pass_ms_median": ms, "pass_ms_min": float(np.min(times)), "levels": int(lv.value), "level_launches": launches,
                      "ms_per_level_launch_mean": ms / launches, "reps": a.reps}
        print(label, out[label])
    # the CLI on the small fixture, by stage (wall time, one run after a warm-up run)
    import predict_fixture as F
    from gcn_drug_repurposing_amd import predict
    for r in range(2):
        with tempfile.TemporaryDirectory() as tmp:
            cwd = os.getcwd()
            os.chdir(tmp)
            try:
                s = predict.Settings(predict.load_config(F.stage(tmp, "gcn")))
                tm = {}
                t0 = time.perf_counter()
                predict.run(s, "proteins.tsv", timings=tm)
                tm["total_s"] = time.perf_counter() - t0
            finally:
                os.chdir(cwd)
    out["cli_fixture_gcn_with_protein_table_s"] = tm
    print("cli", tm)
    try:
        import networkx as nx
    except ImportError:
        out["networkx"] = "not importable here: no speedup quoted"
    else:
        G = nx.DiGraph()
        G.add_nodes_from(names)
        G.add_edges_from((u, v) for u, s_ in g.adj.items() for v in s_)
        prots = [n for n, t_ in zip(names, types) if t_ == "protein"]
        rng = np.random.RandomState(0)
        sample = [prots[i] for i in rng.choice(len(prots), min(a.nx_sample, len(prots)), replace=False)]
        t0 = time.perf_counter()
        for v in sample:
            try:
                nx.shortest_path(G, source=v, target="NodeCovid")
            except nx.NetworkXNoPath:
                pass
        per = (time.perf_counter() - t0) / len(sample)
        out["networkx"] = {"per_search_ms_sample_mean": per * 1e3, "sample": len(sample),
                           "extrapolated_17444_searches_s": per * 17444, "note": "extrapolated from the sample, not timed in full"}
        print("networkx", out["networkx"])
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "paths_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
