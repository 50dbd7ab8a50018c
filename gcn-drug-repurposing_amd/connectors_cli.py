"""The command line of the seed connector algorithm (Wang and Loscalzo 2018): join the fragments of every disease's genes, every drug's
targets or every line of a seeds file on the GPU, name the connectors, and compare the seeds joined with degree-matched random sets."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._sets_cli import add_null_arguments, add_set_source, check_null_arguments, read_sets, write_null
from .proximity import ProximityError
from .proximity_cli import _fmt
from .set_modules import STAT_FIELDS, largest_component

HEADER = ["set", "rank", "gene", "lcc", "merged", "degree"]
CONNECTORS_HEADER = ["set", "step", "gene", "degree", "lcc.before", "lcc.after", "gain", "merged", "in.final.lcc"]
SUMMARY_HEADER = (["set", "n", "lcc.before", "lcc.after", "seeds.joined", "connectors", "connectors.null.mean", "connectors.null.sd"]
                  + [f"joined.{f}" for f in STAT_FIELDS] + [f"fraction.{f}" for f in STAT_FIELDS] + [f"lcc.{f}" for f in STAT_FIELDS] + ["short"])


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="seed_connectors.py", description="seed connector algorithm: join a gene set's fragments on the GPU")
    p.add_argument("--network", required=True, help="gene network .sif (gene rel gene), read as undirected; its LCC is used")
    add_set_source(p, seeds=True, null=True)
    p.add_argument("--max-add", default=500, type=int, help="connectors to add to a set at the most")
    add_null_arguments(p, or_zero=True)
    p.add_argument("--out", default="modules.tsv", help="the connectors, one row per set and rank (the layout of diamond.py --out)")
    p.add_argument("--connectors", default=None, help="also write every step: the LCC before and after, the components joined")
    p.add_argument("--summary", default=None, help="also write one row per set: the LCC before and after, seeds joined, connectors, the null")
    p.add_argument("--genes", default=None, help="also write every grown module, seeds and connectors, as a gene table in the layout of "
                   "disease_genes.tsv: what disease_modules.py and proximity.py --diseases read")
    p.add_argument("--null", default=None, help="also write the integer nulls, int32 [n_sets][3][n_random] (steps, final lcc, seeds joined), as .npy")
    args = p.parse_args(argv)
    if args.max_add < 1:
        p.error(f"--max-add {args.max_add} must be >= 1")
    check_null_arguments(p, args, or_zero=True)
    if args.null and args.n_random == 0:
        p.error("--null needs --n-random >= 2")
    return args


def write_modules(path, names, genes, grown):
    """modules.tsv: one row per set and connector, in the order of `names` (grown: ConnectorEngine.grow's return; genes: the network's
    names by node index); a set that stopped has fewer rows than --max-add"""
    with open(path, "w") as f:
        f.write("\t".join(HEADER) + "\n")
        for i, name in enumerate(names):
            for r in range(int(grown["steps"][i])):
                f.write(f"{name}\t{r + 1}\t{genes[int(grown['node'][i, r])]}\t{int(grown['lcc'][i, r])}\t{int(grown['merged'][i, r])}\t"
                        f"{int(grown['deg'][i, r])}\n")


def write_connectors(path, names, genes, grown):
    """connectors.tsv: one row per (set, step); in.final.lcc = 1 when the connector is in the final largest component"""
    with open(path, "w") as f:
        f.write("\t".join(CONNECTORS_HEADER) + "\n")
        for i, name in enumerate(names):
            steps = int(grown["steps"][i])
            label = grown["label"][i]
            top, before = largest_component(label), int(grown["first_lcc"][i])
            for r in range(steps):
                after = int(grown["lcc"][i, r])
                inside = int(int(label[len(label) - steps + r]) == top)
                f.write(f"{name}\t{r + 1}\t{genes[int(grown['node'][i, r])]}\t{int(grown['deg'][i, r])}\t{before}\t{after}\t{after - before}\t"
                        f"{int(grown['merged'][i, r])}\t{inside}\n")
                before = after


def write_summary(path, names, res):
    """summary.tsv: one row per set (res: ConnectorEngine.connector_table's return); without a null its columns are NA"""
    grown = res["grow"]
    nan = np.full(len(names), np.nan)
    blank = {f: nan for f in STAT_FIELDS}
    with open(path, "w") as f:
        f.write("\t".join(SUMMARY_HEADER) + "\n")
        for i, name in enumerate(names):
            cells = [name] + [str(int(x[i])) for x in (res["n"], grown["first_lcc"], grown["final_lcc"], grown["seeds_in"], grown["steps"])]
            cells += [_fmt(res.get(k, nan)[i]) for k in ("connectors_null_mean", "connectors_null_sd")]
            for stats in ("joined_stats", "fraction_stats", "lcc_stats"):
                cells += [_fmt(res.get(stats, blank)[k][i]) for k in STAT_FIELDS]
            f.write("\t".join(cells + [str(int(res["short"][i])) if "short" in res else "NA"]) + "\n")


def write_genes(path, names, genes, grown):
    """the grown modules as a gene table: `<empty>\\t<name>\\t<gene>...`, seeds first, then the connectors in the order added"""
    with open(path, "w") as f:
        for name, members in zip(names, grown["members"]):
            f.write("\t".join(["", name] + [genes[int(v)] for v in members]) + "\n")


def main(argv=None):
    from . import proximity as P
    from .connectors import ConnectorEngine
    args = parse_args(argv)
    t0 = time.time()
    try:
        sets, names, _ = read_sets(args)
        net = P.read_network(args.network)
    except (OSError, ValueError) as e:
        sys.exit(f"seed_connectors: {e}")
    eng = ConnectorEngine(net)
    try:
        res = eng.connector_table([sets[n] for n in names], 0 if args.drugs else 1, n_add=args.max_add, n_random=args.n_random, seed=args.seed,
                                  min_bin_size=args.min_bin_size)
    except ProximityError as e:
        sys.exit(f"seed_connectors: {e}")
    finally:
        eng.close()
    grown = res["grow"]
    write_modules(args.out, names, net.names, grown)
    print(f"wrote {args.out}")
    for where, writer in ((args.connectors, write_connectors), (args.genes, write_genes)):
        if where:
            writer(where, names, net.names, grown)
            print(f"wrote {where}")
    if args.summary:
        write_summary(args.summary, names, res)
        print(f"wrote {args.summary}")
    if args.null:
        write_null(args.null, [res[k][:, 1:] for k in ("steps", "final_lcc", "seeds_in")])
        print(f"wrote {args.null}")
    print(f"seed_connectors: {len(names)} sets, max_add={args.max_add}, n_random={args.n_random}, LCC {net.n} nodes, "
          f"{int(grown['steps'].sum())} connectors, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
