#!/usr/bin/env python3
"""gss_rank_metrics_rows beside gss_auc_rows on evaluate_bench.py's shape: the 29,960-node whole-graph stand-in's 840 indications +
NodeCovid x 1,661 drugs with the reference's 5,926 labels, scores = inner products of seeded Gaussian embeddings (d 128), ks = (10, 50).
Each entry point by device events around the call (it includes the status read-back), median of 4 x --reps calls after two warm-ups, as
profiles/evaluate_bench.json was made; and evaluate.device_metrics' upload / kernel split by the host clock, median of --reps.
Writes profiles/rank_metrics_bench.json.   python tools/rank_metrics_bench.py [--reps 5]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KS = (10, 50)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from gcn_drug_repurposing_amd import _lib, evaluate, synth
    from gcn_drug_repurposing_amd.msi import COMPONENTS, MsiGraph
    hashes = _lib.source_hashes()
    out = {"graph": "synth.standin_tables(seed=1) + synth.standin_drug_indications()", "scores": "seeded N(0,1) d=128 inner products",
           "ks": list(KS), "source_hash": {k: hashes[k] for k in ("rank_metrics.hip", "auc.hip", "rank_keys.h")}, "reps": a.reps}
    with tempfile.TemporaryDirectory() as tmp:
        for name, rows in synth.standin_tables(seed=1).items():
            with open(os.path.join(tmp, name + ".tsv"), "w") as f:
                f.write("node_1\tnode_2\n")
                f.writelines(f"{x}\t{y}\n" for x, y in rows)
        g = MsiGraph().load({name: os.path.join(tmp, name + ".tsv") for name, _, _ in COMPONENTS})
    names = g.names
    x = np.round(np.random.RandomState(4).randn(len(names), 128), 6)
    idx = {n: i for i, n in enumerate(names)}
    drugs = [n for n in names if g.type[n] == "drug"]
    inds = [n for n in names if g.type[n] == "indication"]
    scores = np.ascontiguousarray(x[[idx[i] for i in inds]] @ x[[idx[d] for d in drugs]].T)
    ptr, col, _, _ = evaluate.label_rows(inds, drugs, synth.standin_drug_indications())
    R, C = scores.shape
    out["rows"], out["cols"], out["positives"] = R, C, int(len(col))
    lib = _lib.load()
    d_s = torch.from_numpy(scores).cuda()
    d_p, d_c = torch.from_numpy(ptr).cuda(), torch.from_numpy(col).cuda()
    auc = torch.empty(R, dtype=torch.float64, device="cuda")
    auc2 = torch.empty(R, dtype=torch.float64, device="cuda")
    avp = torch.empty(R, dtype=torch.float64, device="cuda")
    hits = torch.empty(R, len(KS), dtype=torch.float64, device="cuda")
    n_p = torch.empty(R, dtype=torch.int32, device="cuda")
    n_n = torch.empty(R, dtype=torch.int32, device="cuda")
    ws_bytes = lib.gss_rank_metrics_workspace_bytes(R, C)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device="cuda")
    ks = np.asarray(KS, np.int32)
    out["workspace_bytes"] = int(ws_bytes)

    def call_auc():
        _lib.check(lib.gss_auc_rows(R, C, _lib.ptr(d_s), C, _lib.ptr(d_p), _lib.ptr(d_c), _lib.ptr(auc), _lib.ptr(n_p), _lib.ptr(n_n),
                                    _lib.current_stream()))

    def call_metrics():
        _lib.check(lib.gss_rank_metrics_rows(R, C, _lib.ptr(d_s), C, _lib.ptr(d_p), _lib.ptr(d_c), len(KS), ks.ctypes.data, _lib.ptr(auc2),
                                             _lib.ptr(avp), _lib.ptr(hits), _lib.ptr(n_p), _lib.ptr(n_n), _lib.ptr(ws), ws_bytes,
                                             _lib.current_stream()))

    for key, call in (("auc_rows_ms_device_events_median", call_auc), ("rank_metrics_rows_ms_device_events_median", call_metrics)):
        ev = []
        for r in range(a.reps * 4 + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ev.append(e0.elapsed_time(e1))
        out[key] = float(np.median(ev))
    out["auc_bits_equal"] = bool(np.array_equal(auc.cpu().numpy().view(np.uint64), auc2.cpu().numpy().view(np.uint64)))
    split = []
    for r in range(a.reps + 1):
        t = {}
        res = evaluate.device_metrics(scores, ptr, col, KS, timings=t)
        if r:
            split.append(t)
    out["device_metrics_s_median"] = {k: float(np.median([t[k] for t in split])) for k in ("upload_s", "kernel_s")}
    kept = (res[3] > 0) & (res[4] > 0)
    out["indications_evaluated"] = int(kept.sum())
    out["lines"] = [evaluate.format_line(res[0][kept]), evaluate.format_metric_line("ap", res[1][kept])] + [
        evaluate.format_metric_line(f"recall@{k}", res[2][kept, j] / res[3][kept]) for j, k in enumerate(KS)]
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "rank_metrics_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
