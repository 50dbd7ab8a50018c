"""The command line of the Steiner trees: connect every disease's genes, every drug's targets or every line of a seeds file by an
approximate Steiner tree on the GPU, name the connector nodes, and compare their number and the tree's length with degree-matched random
sets (the lower tail: fewer and shorter than random is the signal)."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._sets_cli import add_null_arguments, add_set_source, check_null_arguments, read_sets, write_null
from .proximity import ProximityError
from .proximity_cli import _fmt
from .set_modules import STAT_FIELDS

HEADER = ["set", "a", "b", "kind"]
NODES_HEADER = ["set", "gene", "role", "parent", "degree"]
SUMMARY_HEADER = (["set", "n", "trees", "steiner", "length", "edges", "longest.bridge", "listed"]
                  + [f"steiner.{f}" for f in STAT_FIELDS] + [f"length.{f}" for f in STAT_FIELDS] + ["short"])


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="steiner.py", description="approximate Steiner trees: the smallest subnetwork that connects a gene set, on the GPU")
    p.add_argument("--network", required=True, help="gene network .sif (gene rel gene), read as undirected; its LCC is used")
    add_set_source(p, seeds=True, null=True)
    p.add_argument("--max-add", default=4096, type=int, help="Steiner nodes listed per set at the most (the counts are exact beyond it)")
    add_null_arguments(p, or_zero=True)
    p.add_argument("--out", default="edges.tsv", help="the trees' edges, one row per set and edge: kind path (a Steiner node and its parent) or bridge")
    p.add_argument("--nodes", default=None, help="also write the trees' nodes: role seed or steiner, a Steiner node's parent, the degree in the tree")
    p.add_argument("--summary", default=None, help="also write one row per set: trees, Steiner nodes, length, the null")
    p.add_argument("--genes", default=None, help="also write every tree's nodes, seeds and Steiner nodes, as a gene table in the layout of "
                   "disease_genes.tsv: what disease_modules.py and proximity.py --diseases read")
    p.add_argument("--null", default=None, help="also write the integer nulls, int32 [n_sets][2][n_random] (Steiner nodes, length), as .npy")
    args = p.parse_args(argv)
    if args.max_add < 1:
        p.error(f"--max-add {args.max_add} must be >= 1")
    check_null_arguments(p, args, or_zero=True)
    if args.null and args.n_random == 0:
        p.error("--null needs --n-random >= 2")
    return args


def write_edges(path, names, genes, trees):
    """edges.tsv: one row per set and tree edge, in the order of `names` (trees: SteinerEngine.trees' return; genes: the network's names
    by node index): the parent edges of the listed Steiner nodes, then the bridges"""
    with open(path, "w") as f:
        f.write("\t".join(HEADER) + "\n")
        for name, edges in zip(names, trees["edges"]):
            for a, b, kind in edges:
                f.write(f"{name}\t{genes[a]}\t{genes[b]}\t{kind}\n")


def write_nodes(path, names, genes, trees):
    """nodes.tsv: one row per set and tree node, the seeds in their order and then the listed Steiner nodes; parent is NA for a seed,
    degree the node's edges in the listed tree"""
    with open(path, "w") as f:
        f.write("\t".join(NODES_HEADER) + "\n")
        for i, name in enumerate(names):
            degree = {}
            for a, b, _ in trees["edges"][i]:
                degree[a] = degree.get(a, 0) + 1
                degree[b] = degree.get(b, 0) + 1
            for v in trees["terminals"][i]:
                f.write(f"{name}\t{genes[int(v)]}\tseed\tNA\t{degree.get(int(v), 0)}\n")
            for v, p in zip(trees["steiner"][i], trees["parent"][i]):
                f.write(f"{name}\t{genes[int(v)]}\tsteiner\t{genes[int(p)]}\t{degree.get(int(v), 0)}\n")


def write_summary(path, names, res):
    """summary.tsv: one row per set (res: SteinerEngine.tree_table's return); without a null its columns are NA"""
    trees = res["trees"]
    nan = np.full(len(names), np.nan)
    blank = {f: nan for f in STAT_FIELDS}
    with open(path, "w") as f:
        f.write("\t".join(SUMMARY_HEADER) + "\n")
        for i, name in enumerate(names):
            cells = [name] + [str(int(x[i])) for x in (res["n"], trees["n_comp"], trees["n_steiner"], trees["length"], trees["n_edges"], trees["max_w"])]
            cells.append(str(len(trees["steiner"][i])))
            for stats in ("steiner_stats", "length_stats"):
                cells += [_fmt(res.get(stats, blank)[k][i]) for k in STAT_FIELDS]
            f.write("\t".join(cells + [str(int(res["short"][i])) if "short" in res else "NA"]) + "\n")


def write_genes(path, names, genes, trees):
    """the trees' nodes as a gene table: `<empty>\\t<name>\\t<gene>...`, seeds first, then the listed Steiner nodes in node order"""
    with open(path, "w") as f:
        for name, seeds, steiner in zip(names, trees["terminals"], trees["steiner"]):
            f.write("\t".join(["", name] + [genes[int(v)] for v in seeds] + [genes[int(v)] for v in steiner]) + "\n")


def main(argv=None):
    from . import proximity as P
    from .steiner import SteinerEngine
    args = parse_args(argv)
    t0 = time.time()
    try:
        sets, names, _ = read_sets(args)
        net = P.read_network(args.network)
    except (OSError, ValueError) as e:
        sys.exit(f"steiner: {e}")
    eng = SteinerEngine(net)
    try:
        res = eng.tree_table([sets[n] for n in names], 0 if args.drugs else 1, n_random=args.n_random, seed=args.seed,
                             min_bin_size=args.min_bin_size, max_add=args.max_add)
    except ProximityError as e:
        sys.exit(f"steiner: {e}")
    finally:
        eng.close()
    trees = res["trees"]
    write_edges(args.out, names, net.names, trees)
    print(f"wrote {args.out}")
    for where, writer in ((args.nodes, write_nodes), (args.genes, write_genes)):
        if where:
            writer(where, names, net.names, trees)
            print(f"wrote {where}")
    if args.summary:
        write_summary(args.summary, names, res)
        print(f"wrote {args.summary}")
    if args.null:
        write_null(args.null, [res[k][:, 1:] for k in ("n_steiner", "length")])
        print(f"wrote {args.null}")
    print(f"steiner: {len(names)} sets, max_add={args.max_add}, n_random={args.n_random}, LCC {net.n} nodes, "
          f"{int(trees['n_steiner'].sum())} Steiner nodes, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
