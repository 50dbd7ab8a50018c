#!/usr/bin/env python3
"""node2vec input embeddings at the MSI size (the real-layer stand-in, 29,960 nodes) and the reference settings (predict_drug.py:40-46:
64 walks of 16 nodes per node, p = q = 0.25, dim 128, window 10; gensim's negative 5, sample 1e-3, 5 epochs).  Prints one JSON line:
setup, walk and SGNS seconds, skip-gram pairs per second, and the byte model of DESIGN.md section 9.1 (12 rows of d fp32 per pair:
the context row read and written, five negative rows read and written) with the fraction of the L2 / Infinity-Cache band it reaches.
The pair count is the expectation over the reduced windows with every token kept (downsampling drops a few tokens of the hubs).
gensim is not measured (it is not part of this project's dependencies); no speedup is quoted.
usage: node2vec_bench.py [--reps R] [--concurrency C]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gcn_drug_repurposing_amd import _lib, node2vec as N  # noqa: E402
from gcn_drug_repurposing_amd.synth import whole_graph_standin  # noqa: E402


def expected_pairs(lengths, window):
    """sum over sentences of the expected number of (center, context) pairs: reduced window b uniform in [0, window)"""
    hist = np.bincount(lengths)
    total = 0.0
    for k, cnt in enumerate(hist):
        if cnt == 0:
            continue
        per = 0.0
        for b in range(window):
            r = window - b
            per += sum(min(k, i + r + 1) - max(0, i - r) - 1 for i in range(k))
        total += cnt * per / window
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--concurrency", type=int, default=None)
    ap.add_argument("--epochs", type=int, default=5)
    args = ap.parse_args()
    lib = _lib.load()
    adj, _, names = whole_graph_standin()
    n, L, R, d, window = adj.shape[0], 16, 64, 128, 10
    rows = []
    for rep in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = N.prepare_csr(adj)
        starts = N.start_nodes(n, R, rep)
        t1 = time.perf_counter()
        w, ln = N.random_walks(a, R, L, 0.25, 0.25, seed=rep)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        syn0, _ = N.train_sgns(w, ln, n, d, window, args.epochs, seed=rep, concurrency=args.concurrency)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        rows.append((t1 - t0, t2 - t1, t3 - t2))
        del starts
    lengths = ln.cpu().numpy()
    pairs = expected_pairs(lengths, window) * args.epochs
    med = np.median(np.asarray(rows), axis=0)
    bytes_model = pairs * 12 * d * 4
    out = {
        "workload": "node2vec_msi_standin", "nodes": n, "edges": int(adj.nnz), "walks": int(n * R), "walk_length": L,
        "tokens_per_epoch": int(lengths.sum()), "epochs": args.epochs, "dim": d, "window": window, "negative": 5,
        "concurrency": args.concurrency or lib.gss_sgns_default_concurrency(), "reps": args.reps,
        "setup_s": round(float(med[0]), 4), "walk_s": round(float(med[1]), 4), "sgns_s": round(float(med[2]), 4),
        "walk_s_all": [round(r[1], 4) for r in rows], "sgns_s_all": [round(r[2], 4) for r in rows],
        "pairs_expected": int(pairs), "pairs_per_s": round(pairs / float(med[2]), 1),
        "bytes_model": int(bytes_model), "achieved_TBps": round(bytes_model / float(med[2]) / 1e12, 3),
        "fraction_of_8TBps": round(bytes_model / float(med[2]) / 8e12, 4), "fraction_of_17TBps": round(bytes_model / float(med[2]) / 17e12, 4),
        "finite": bool(torch.isfinite(syn0).all().item()),
        "gensim": "not measured (not installed); no speedup quoted",
        "sgns_hip": _lib.load().gss_source_hash(b"sgns.hip").decode(), "walk_hip": _lib.load().gss_source_hash(b"walk.hip").decode(),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
