#!/usr/bin/env python3
"""Golden fixture for interpret.py: the four tables it writes for the top drugs of the predict_msi_small fixture (make_predict_fixture.py)
under node2vec, gcn and diffusion, from networkx's full ENUMERATION of the shortest paths (nx.all_shortest_paths) on the graph the
reference's own MSI class builds from the fixture tables -- not from the code under test.  Counts are lengths of lists of paths, shares
are one division of two such integers, the best path is the enumerated path with the largest weight sum taken from the target outward.
The generator asserts that every best path it records beats the second best by a relative margin of 1e-3, so the files depend neither
on an index order nor on the last bits of a device-computed diffusion profile.
Run in the build container only, after make_predict_fixture.py:  python tests/golden/make_trace_fixture.py"""
import csv
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_predict_fixture as P  # noqa: E402

SRC = P.OUT
OUT = os.path.join(HERE, "trace_msi_small")
QUERY = "NodeCovid"
MARGIN = 1e-3
TRACE_HEADER = ["query", "drug name", "proximity", "path length", "shortest paths", "nodes on them", "best path", "best path score"]
NODES_HEADER = ["query", "drug", "node", "name", "type", "hops from drug", "hops to query", "paths through", "share", "proximity"]
EDGES_HEADER = ["query", "drug", "from", "to", "share"]
MEDIATORS_HEADER = ["query", "node", "name", "type", "drugs", "share sum"]


def shown(m, node):
    v = m.node2name[node]
    return node if v is np.nan else v


def cell(v):
    return "NA" if v is None else repr(float(v)) if isinstance(v, (float, np.floating)) else v


def write(path, header, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", lineterminator="\n")
        w.writerow(header)
        for r in rows:
            w.writerow([cell(v) for v in r])


def outward_sum(weight, path):
    """the weights of a path's interior nodes and its source, summed from the target outward -> (interior sum, whole sum)"""
    total = 0.0
    inner = None
    for k in range(len(path) - 2, -1, -1):
        if k == 0:
            inner = total
        total = weight[path[k]] + total
    return inner, total


def tables(m, weight, ranked, prox, index):
    import networkx as nx
    trace, nodes, edges = [], [], []
    med_sum, med_cnt = {}, {}
    for drug, px in zip(ranked, prox):
        label = shown(m, drug)
        try:
            paths = [list(p) for p in nx.all_shortest_paths(m.graph, drug, QUERY)]
        except nx.NetworkXNoPath:
            trace.append([QUERY, label, float(px)] + [None] * 5)
            continue
        total = len(paths)
        length = len(paths[0]) - 1
        on = sorted({v for p in paths for v in p}, key=lambda v: index[v])
        scored = sorted(((outward_sum(weight, p), p) for p in paths), key=lambda t: -t[0][1])
        (inner, whole), best = scored[0]
        if total > 1:
            second = scored[1][0][1]
            assert whole - second > MARGIN * max(abs(whole), abs(second)), (drug, whole, second)
        trace.append([QUERY, label, float(px), length, total, len(on) - 2, ", ".join(shown(m, v) for v in best), inner if length > 1 else None])
        through = {v: sum(1 for p in paths if v in p) for v in on}
        hops = {v: paths[[v in p for p in paths].index(True)].index(v) for v in on}
        for v in sorted(on, key=lambda v: (hops[v], index[v])):
            name = m.node2name[v]
            nodes.append([QUERY, label, v, None if name is np.nan else name, m.graph.nodes[v]["type"], hops[v], length - hops[v], through[v],
                          through[v] / total, float(weight[v])])
            if v not in (drug, QUERY):
                med_sum[v] = med_sum.get(v, 0.0) + through[v] / total
                med_cnt[v] = med_cnt.get(v, 0) + 1
        count = {}
        for p in paths:
            for e in zip(p, p[1:]):
                count[e] = count.get(e, 0) + 1
        for (a, b) in sorted(count, key=lambda e: (index[e[0]], index[e[1]])):
            edges.append([QUERY, label, a, b, count[(a, b)] / total])
    med = []
    for v in sorted(med_sum, key=lambda v: (-med_sum[v], index[v])):
        name = m.node2name[v]
        med.append([QUERY, v, None if name is np.nan else name, m.graph.nodes[v]["type"], med_cnt[v], med_sum[v]])
    return trace, nodes, edges, med


def main():
    from sklearn.preprocessing import normalize
    os.makedirs(OUT, exist_ok=True)
    pd_, ref_msi, _ = P.stub_modules()
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            for case, gcn, pathway in (("node2vec", False, False), ("gcn", True, True), ("diffusion", None, False)):
                m = P.ref_msi_graph(ref_msi, pathway)
                index = {v: i for i, v in enumerate(m.graph.nodes)}
                if gcn is None:
                    res = np.load(os.path.join(SRC, "diffusion_NodeCovid.npy"))
                    nodelist = json.load(open(os.path.join(SRC, "diffusion_nodelist.json")))
                    weight = {v: float(res[i]) for i, v in enumerate(nodelist)}
                    drugs = [v for v in nodelist if m.graph.nodes[v]["type"] == "drug"]
                    prox = np.asarray([weight[d] for d in drugs])
                    rid = np.argsort(np.array(prox))[::-1]
                    ranked, prox = [drugs[i] for i in rid], prox[rid]
                else:
                    shutil.copy(os.path.join(SRC, "n2v.embs.txt"), os.path.join(tmp, "n2v_num_64_len_16.embs.txt"))
                    cfg = {"node2vec": {"emb_file_prefix": os.path.join(tmp, "n2v"), "walk_length": 16, "number_walk": 64},
                           "gcn": {"emb_file": os.path.join(SRC, "gcn.embs.txt")}}
                    _, ranked, prox = pd_.graph_embedding(cfg, m, gcn=gcn)
                    vecs = np.loadtxt(os.path.join(SRC, "n2v.embs.txt"), skiprows=1, dtype=object)
                    file_nodes = list(vecs[:, 0])
                    embs = normalize(np.loadtxt(os.path.join(SRC, "gcn.embs.txt")), axis=1) if gcn else vecs[:, 1:].astype(float)
                    w = np.matmul(embs, np.array(embs[file_nodes.index(QUERY)]))
                    weight = {v: float(w[i]) for i, v in enumerate(file_nodes)}
                trace, nodes, edges, med = tables(m, weight, ranked[:P.TOPK], prox[:P.TOPK], index)
                write(os.path.join(OUT, f"expected_{case}_trace.tsv"), TRACE_HEADER, trace)
                write(os.path.join(OUT, f"expected_{case}_nodes.tsv"), NODES_HEADER, nodes)
                write(os.path.join(OUT, f"expected_{case}_edges.tsv"), EDGES_HEADER, edges)
                write(os.path.join(OUT, f"expected_{case}_mediators.tsv"), MEDIATORS_HEADER, med)
                print(case, f"{len(trace)} drugs, {len(nodes)} nodes, {len(edges)} edges, {len(med)} mediators")
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    main()
