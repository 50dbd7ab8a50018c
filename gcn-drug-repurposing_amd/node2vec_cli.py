"""The OpenNE command line for node2vec (multiscale/openne/__main__.py:22-120, the flags predict_drug.py's pipeline uses)."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="node2vec input embeddings (biased walks + skip-gram) on the GPU")
    p.add_argument('--input', required=True, help='Input graph file')
    p.add_argument('--output', required=True, help='Output representation file')
    p.add_argument('--graph-format', default='edgelist', help='Input graph format (edgelist only)')
    p.add_argument('--weighted', action='store_true', help='Treat graph as weighted')
    p.add_argument('--directed', action='store_true', help='Treat graph as directed')
    p.add_argument('--number-walks', default=10, type=int, help='Number of random walks to start at each node')
    p.add_argument('--walk-length', default=80, type=int, help='Length of the random walk started at each node')
    p.add_argument('--representation-size', default=128, type=int, help='Number of latent dimensions to learn for each node')
    p.add_argument('--window-size', default=10, type=int, help='Window size of skipgram model')
    p.add_argument('--p', default=1.0, type=float)
    p.add_argument('--q', default=1.0, type=float)
    p.add_argument('--workers', default=8, type=int, help='Accepted for compatibility and ignored (the GPU runs the walks)')
    p.add_argument('--method', default='node2vec', help='The learning method (node2vec only)')
    p.add_argument('--epochs', default=5, type=int, help='Skip-gram epochs (gensim iter)')
    p.add_argument('--seed', default=0, type=int, help='Seed of the counter-based generator (walks, start order, skip-gram)')
    p.add_argument('--concurrency', default=None, type=int, help='Skip-gram center positions in flight (default: fill the GPU)')
    args = p.parse_args(argv)
    if args.method != 'node2vec':
        p.error(f"--method {args.method}: only node2vec is implemented (not deepWalk / line / gcn / grarep / tadw / lle / ...)")
    if args.graph_format != 'edgelist':
        p.error(f"--graph-format {args.graph_format}: only edgelist is implemented")
    return args


def read_graph(path, weighted, directed):
    """OpenNE Graph.read_edgelist: a networkx DiGraph, nodes in order of first appearance (src, then dst), weight 1.0 unless
    --weighted; undirected input adds both directions; a repeated edge keeps the weight of its last line -> (CSR, names)"""
    import scipy.sparse as sp

    from .embio import read_edgelist
    src, dst, w, names = read_edgelist(path)
    if path.endswith(".sif") or path.endswith(".sif.lcc"):   # read_edgelist emits both directions of a .sif line already
        directed = True
    if not weighted:
        w = np.ones_like(w)
    if not directed:
        src, dst, w = np.stack([src, dst], 1).reshape(-1), np.stack([dst, src], 1).reshape(-1), np.repeat(w, 2)
    n = len(names)
    key = src * n + dst
    _, last = np.unique(key[::-1], return_index=True)
    keep = len(key) - 1 - last
    adj = sp.csr_matrix((w[keep], (src[keep], dst[keep])), shape=(n, n))
    adj.sort_indices()
    return adj, names


def main(argv=None):
    args = parse_args(argv)
    from .node2vec import Node2vec, check_walk_args
    check_walk_args(args.p, args.q, args.walk_length, args.number_walks)
    t0 = time.time()
    adj, names = read_graph(args.input, args.weighted, args.directed)
    print(f"Reading... {len(names)} nodes, {adj.nnz} directed edges")
    model = Node2vec((adj, names), path_length=args.walk_length, num_paths=args.number_walks, dim=args.representation_size,
                     p=args.p, q=args.q, window=args.window_size, epochs=args.epochs, seed=args.seed, concurrency=args.concurrency)
    print(f"walks {model.timings['walks_s']:.3f} s, skip-gram {model.timings['sgns_s']:.3f} s")
    print("Saving embeddings...")
    model.save_embeddings(args.output)
    print(f"time used: {time.time() - t0:.3f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
