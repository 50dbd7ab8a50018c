"""interpret.py: trace the ranked drug candidates back to the query.  The reference's interpret.py is a note of intent ("given a node
(drug/disease, etc.), tracing the connections in the networks based on exact connections or computed proximities"); this is the
command.  It reads predict_drug.py's config, builds the same graph and ranks the drugs with the same functions (predict.py), then per
(drug, query) pair reports every shortest path at once instead of one of them: how many there are, which nodes and edges lie on them
and what share of the paths passes through each, the one path that the model's own proximities favour, and over all selected drugs the
mediators of the query.  Counts, best paths and the between pass run on the GPU (trace.py / csrc/trace.hip); no CPU fallback.

The weight of node v for query t is the model's proximity of v to t: x[v] . x[t] in fp64 for node2vec / gcn (rows normalised for gcn,
as predict.embedding_scores does), the query's diffusion profile at v for diffusion -- also when the config's diffusion.compare ranks the
drugs by a distance between profiles, which changes which drugs are traced and their proximity column, nothing else.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from . import predict
from .paths import PathsError
from .predict import PredictError, display, write_tsv

TRACE_HEADER = ["query", "drug name", "proximity", "path length", "shortest paths", "nodes on them", "best path", "best path score"]
NODES_HEADER = ["query", "drug", "node", "name", "type", "hops from drug", "hops to query", "paths through", "share", "proximity"]
EDGES_HEADER = ["query", "drug", "from", "to", "share"]
MEDIATORS_HEADER = ["query", "node", "name", "type", "drugs", "share sum"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: trace drug candidates to the query node (interpret.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as predict_drug.py reads it")
    p.add_argument("--query", action="append", default=None, help="node to trace to (repeatable; default NodeCovid)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--top", default=None, type=int, help="trace the first K drugs of the ranking (default: the config's topk)")
    g.add_argument("--drug", action="append", default=None, help="trace this drug (node id, repeatable), in the ranking's order")
    g.add_argument("--all-drugs", action="store_true", help="trace every drug of the ranking")
    p.add_argument("--out", default="trace.tsv", type=str, help="one row per (query, drug) (default: trace.tsv)")
    p.add_argument("--nodes", default=None, type=str, help="also write the nodes on the shortest paths of every pair")
    p.add_argument("--edges", default=None, type=str, help="also write the edges on the shortest paths of every pair")
    p.add_argument("--mediators", default=None, type=str, help="also write the mediators of every query over the traced drugs")
    p.add_argument("--seed", default=0, type=int, help="seed of the node2vec walks / skip-gram when the embedding file is generated")
    return p.parse_args(argv)


def device_tracer(adj):
    from .trace import PathTracer
    return PathTracer(adj)


def select(drugs, top, chosen, every, g):
    """positions in the ranking of the drugs to trace"""
    if every:
        return list(range(len(drugs)))
    if chosen:
        if len(set(chosen)) != len(chosen):
            raise PredictError(f"--drug: repeated drug in {chosen}")
        for d in chosen:
            if d not in g.adj:
                raise PredictError(f"--drug {d!r} is not a node of the graph")
            if d not in drugs:
                raise PredictError(f"--drug {d!r} is not a drug of the ranking")
        want = set(chosen)
        return [k for k, d in enumerate(drugs) if d in want]
    if top < 1:
        raise PredictError(f"--top {top} must be at least 1")
    return list(range(min(top, len(drugs))))


def embedding_weights(names, x, graph_names, query):
    """x[v] . x[t] for every graph node v, in graph order"""
    idx = {n: i for i, n in enumerate(names)}
    if query not in idx:
        raise PredictError(f"--query {query!r} has no row in the embedding file")
    missing = [n for n in graph_names if n not in idx]
    if missing:
        raise PredictError(f"graph node {missing[0]!r} has no row in the embedding file")
    w = np.matmul(x, np.array(x[idx[query]]))
    return w[[idx[n] for n in graph_names]]


def profile_weights(nodelist, profiles, graph_names, query):
    pos = {n: i for i, n in enumerate(nodelist)}
    missing = [n for n in graph_names if n not in pos]
    if missing:
        raise PredictError(f"graph node {missing[0]!r} has no entry in the diffusion profiles' node order")
    res = np.asarray(profiles[query], np.float64)
    return res[[pos[n] for n in graph_names]]


def node_name(g, node):
    return g.node2name.get(node)


def run(s, top=None, drugs=None, all_drugs=False, out="trace.tsv", nodes=None, edges=None, mediators=None, seed=0, tracer=device_tracer,
        timings=None):
    """the command on Settings s -> {table name: path written}.  tracer(adj) -> an object with trace.PathTracer's interface"""
    import time

    from .trace import edges_between
    if drugs and top is not None:
        raise PredictError("--top and --drug exclude each other")
    t = {} if timings is None else timings
    t0 = time.perf_counter()
    g = predict.build_graph(s)
    predict.check_queries(s, g)
    for d in drugs or []:
        if d not in g.adj:
            raise PredictError(f"--drug {d!r} is not a node of the graph")
    adj, names, types = g.to_csr()
    idx = {n: i for i, n in enumerate(names)}
    t1 = time.perf_counter()
    t["graph_s"] = t1 - t0
    if s.method == "diffusion":
        nodelist, profiles = predict.diffusion_profiles(s, g)
        ranked = predict.rank_profiles(s, nodelist, profiles, g)   # diffusion.compare changes the ranking only: the node weights
        weights = {q: profile_weights(nodelist, profiles, names, q) for q in s.queries}
    else:
        emb_names, x = predict.embedding_scores(s, g, seed)
        ranked = {q: predict.rank_embeddings(emb_names, x, g, q) for q in s.queries}
        weights = {q: embedding_weights(emb_names, x, names, q) for q in s.queries}
    for q, w in weights.items():
        bad = np.nonzero(~np.isfinite(w))[0]
        if len(bad):
            raise PredictError(f"the proximity of node {names[bad[0]]!r} to {q!r} is not finite")
    t2 = time.perf_counter()
    t["rank_s"] = t2 - t1
    chosen = {q: select(ranked[q][0], s.topk if top is None else top, drugs, all_drugs, g) for q in s.queries}
    tr = tracer(adj)      # every refusal of the arguments comes before anything touches the GPU
    rows_trace, rows_nodes, rows_edges, rows_med = [], [], [], []
    t["trace_s"] = 0.0
    for query in s.queries:
        ranked_drugs, prox = ranked[query]
        picked = chosen[query]
        sources = [idx[ranked_drugs[k]] for k in picked]
        w = weights[query]
        ta = time.perf_counter()
        want_tables = nodes is not None or edges is not None
        res = tr.between(sources, [idx[query]], pairs="all" if want_tables else None, weights=w[None, :], mediators=mediators is not None)
        t["trace_s"] += time.perf_counter() - ta
        tw = res.toward
        for i, k in enumerate(picked):
            drug = ranked_drugs[k]
            label = display(g, drug)
            if res.length[i, 0] < 0:
                rows_trace.append([query, label, float(prox[k]), None, None, None, None, None])
                continue
            path = tr.best_path(0, sources[i])
            score = float(tw.best[0, path[1]]) if len(path) > 2 else None
            rows_trace.append([query, label, float(prox[k]), int(res.length[i, 0]), int(res.n_paths[i, 0]), max(int(res.n_nodes[i, 0]) - 2, 0),
                               ", ".join(display(g, names[v]) for v in path), score])
            if not want_tables:
                continue
            tab = res.tables[(i, 0)]
            if nodes is not None:
                for j in np.lexsort((tab.node, tab.hops_from)):
                    v = int(tab.node[j])
                    rows_nodes.append([query, label, names[v], node_name(g, names[v]), types[v], int(tab.hops_from[j]), int(tab.hops_to[j]),
                                       int(tab.through[j]), float(tab.share[j]), float(w[v])])
            if edges is not None:
                eu, ev, es = edges_between(tr.rowptr, tr.col, tab, res.n_paths[i, 0], tw.sigma[0])
                for a, b, sh in zip(eu, ev, es):
                    rows_edges.append([query, label, names[a], names[b], float(sh)])
        if mediators is not None:
            M, C = res.mediators
            hit = np.nonzero(C[0] > 0)[0]
            for v in hit[np.lexsort((hit, -M[0, hit]))]:
                rows_med.append([query, names[v], node_name(g, names[v]), types[v], int(C[0, v]), float(M[0, v])])
    tr.close()
    t3 = time.perf_counter()
    written = {}
    for key, path, header, rows in (("trace", out, TRACE_HEADER, rows_trace), ("nodes", nodes, NODES_HEADER, rows_nodes),
                                    ("edges", edges, EDGES_HEADER, rows_edges), ("mediators", mediators, MEDIATORS_HEADER, rows_med)):
        if path is not None:
            write_tsv(path, header, rows)
            written[key] = path
    t["tables_s"] = time.perf_counter() - t3
    return written


def main(argv=None):
    args = parse_args(argv)
    try:
        s = predict.Settings(predict.load_config(args.config), args.query)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"interpret: {e}", file=sys.stderr)
        sys.exit(2)
    try:
        written = run(s, args.top, args.drug, args.all_drugs, args.out, args.nodes, args.edges, args.mediators, args.seed)
    except (PredictError, PathsError) as e:
        print(f"interpret: {e}", file=sys.stderr)
        sys.exit(2)
    for k, p in written.items():
        print(f"{k}: {p}")
