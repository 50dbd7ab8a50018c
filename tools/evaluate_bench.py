#!/usr/bin/env python3
"""evaluate_auc.py's stages on the 29,960-node whole-graph stand-in (840 indications + NodeCovid x 1,661 drugs, the reference's 5,926
labels), node2vec method with seeded Gaussian embeddings (d 128): graph (load + eval edgelist), scores (embedding file + 841 fp64
matvecs + labels), upload and kernel (device_aucs: host clock around synchronised work; the kernel figure includes the entry point's
status read-back), total; the kernel alone by device events; and consumer.indication_aucs (host numpy) on the same embeddings.
Median of --reps runs after a warm-up.  Writes profiles/evaluate_bench.json.   python tools/evaluate_bench.py [--reps 5]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    from gcn_drug_repurposing_amd import _lib, consumer, evaluate, synth
    out = {"graph": "synth.standin_tables(seed=1) + synth.standin_drug_indications()", "method": "node2vec, seeded N(0,1) d=128",
           "source_hash": {k: _lib.source_hashes()[k] for k in ("auc.hip", "rank_keys.h")}, "reps": a.reps}
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "data")
        os.makedirs(d)
        for name, rows in synth.standin_tables(seed=1).items():
            with open(os.path.join(d, name + ".tsv"), "w") as f:
                f.write("node_1\tnode_2\n")
                f.writelines(f"{x}\t{y}\n" for x, y in rows)
        pos = synth.standin_drug_indications()
        labels = os.path.join(d, "drug_indication_df.tsv")
        with open(labels, "w") as f:
            f.write("drug\tdrug_name\tindication\tindication_name\n")
            f.writelines(f"{dr}\tx\t{i}\ty\n" for i, ds in pos.items() for dr in sorted(ds))
        from gcn_drug_repurposing_amd.msi import MsiGraph
        g = MsiGraph().load({n: os.path.join(d, n + ".tsv") for n in ("drug_to_protein", "indication_to_protein", "protein_to_protein",
                                                                      "protein_to_functional_pathway",
                                                                      "functional_pathway_to_functional_pathway")})
        names = g.names
        x = np.round(np.random.RandomState(4).randn(len(names), 128), 6)
        with open(os.path.join(tmp, "n2v_num_64_len_16.embs.txt"), "w") as f:
            f.write(f"{len(names)} 128\n")
            f.writelines(n + " " + " ".join(repr(float(v)) for v in row) + "\n" for n, row in zip(names, x))
        cfg = {"method": "node2vec", "eval": {"graph": os.path.join(tmp, "eval.edgelist")},
               "networks": {"protein_to_protein": os.path.join(d, "protein_to_protein.tsv"), "drug_to_indication": labels},
               "node2vec": {"eval_emb_file_prefix": os.path.join(tmp, "n2v"), "walk_length": 16, "number_walk": 64}}
        s = evaluate.Settings(cfg)
        stages = []
        res = None
        for r in range(a.reps + 1):
            if os.path.exists(cfg["eval"]["graph"]):
                os.remove(cfg["eval"]["graph"])
            t, dev = {}, {}
            res = evaluate.run(s, timings=t, auc_source=lambda sc, p, c: evaluate.device_aucs(sc, p, c, timings=dev))
            t.update(dev)
            if r:
                stages.append(t)
        out["stages_s_median"] = {k: float(np.median([t[k] for t in stages])) for k in ("graph_s", "scores_s", "upload_s", "kernel_s",
                                                                                         "auc_s", "total_s")}
        out["indications_evaluated"], out["drugs"] = len(res.kept), int(res.n_pos[0] + res.n_neg[0])
        out["line"] = res.line
        # the kernel alone, device events, on the same score matrix
        _, drugs, scores = evaluate.score_rows(s, g, 0)
        ptr, col, _, _ = evaluate.label_rows(res.indications, drugs, consumer.read_drug_indication_tsv(labels))
        lib = _lib.load()
        d_s = torch.from_numpy(scores).cuda()
        d_p, d_c = torch.from_numpy(ptr).cuda(), torch.from_numpy(col).cuda()
        R, C = scores.shape
        auc = torch.empty(R, dtype=torch.float64, device="cuda")
        n_p = torch.empty(R, dtype=torch.int32, device="cuda")
        n_n = torch.empty(R, dtype=torch.int32, device="cuda")
        ev = []
        for r in range(a.reps * 4 + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _lib.check(lib.gss_auc_rows(R, C, _lib.ptr(d_s), C, _lib.ptr(d_p), _lib.ptr(d_c), _lib.ptr(auc), _lib.ptr(n_p), _lib.ptr(n_n),
                                        _lib.current_stream()))
            e1.record()
            torch.cuda.synchronize()
            if r >= 2:
                ev.append(e0.elapsed_time(e1))
        out["entry_point_ms_device_events_median"] = float(np.median(ev))
        out["upload_bytes"] = int(scores.nbytes + ptr.nbytes + col.nbytes)
        # consumer.indication_aucs (host numpy, a Python loop per indication) on the same embeddings
        inds = [n for n in names if g.type[n] == "indication"]
        host = []
        for r in range(2):
            t0 = time.perf_counter()
            want, used = consumer.indication_aucs(x, names, drugs, inds, consumer.read_drug_indication_tsv(labels))
            host.append(time.perf_counter() - t0)
        out["consumer_indication_aucs_s"] = float(min(host))
        out["consumer_note"] = "normalises the rows (the GCN form); same skipped set: " + str(used == [res.indications[k] for k in res.kept])
    print(json.dumps(out, indent=1))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "evaluate_bench.json"), "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
