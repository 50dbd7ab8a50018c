"""The command line of the module check (Menche et al. 2015): for every disease's gene set, or every drug's target set, the largest
connected component it induces on the interactome against degree-matched random sets -- the sets proximity.py scores against."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._sets_cli import add_null_arguments, add_set_source, check_null_arguments, read_sets, write_null
from .proximity import ProximityError
from .proximity_cli import _fmt
from .set_modules import STAT_FIELDS, largest_component

HEADER = (["set", "n", "n.lcc", "n.components", "n.edges"] + [f"lcc.{f}" for f in STAT_FIELDS] + [f"edges.{f}" for f in STAT_FIELDS]
          + ["short"])
MEMBERS_HEADER = ["set", "gene", "component", "in_lcc"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="disease_modules.py",
                                description="module significance of gene sets: largest connected component vs degree-matched random sets, on the GPU")
    p.add_argument("--network", required=True, help="gene network .sif (gene rel gene), read as undirected; its LCC is used")
    add_set_source(p, seeds=False, null=True)
    add_null_arguments(p, or_zero=False)
    p.add_argument("--out", default="modules.tsv", help="the table, one row per set")
    p.add_argument("--members", default=None, help="also write every set's genes with their component")
    p.add_argument("--null", default=None, help="also write the integer nulls, int32 [n_sets][2][n_random] (lcc, edges), as .npy")
    args = p.parse_args(argv)
    check_null_arguments(p, args, or_zero=False)
    return args


def write_table(path, names, res):
    """modules.tsv: one row per set, in the order of `names` (res: ModuleEngine.module_table's return for those sets)"""
    with open(path, "w") as f:
        f.write("\t".join(HEADER) + "\n")
        for i, name in enumerate(names):
            cells = [name] + [str(int(res[k][i])) for k in ("n", "lcc", "n_comp", "n_edges")]
            for stats in (res["lcc_stats"], res["edges_stats"]):
                cells += [_fmt(stats[k][i]) for k in STAT_FIELDS]
            f.write("\t".join(cells + [str(int(res["short"][i]))]) + "\n")


def write_members(path, names, genes, res):
    """members.tsv: one row per gene of every set (genes: the network's names by node index); component = the label, in_lcc = 1 for the
    largest component (of two as large, the one with the smaller label)"""
    with open(path, "w") as f:
        f.write("\t".join(MEMBERS_HEADER) + "\n")
        for name, members, label in zip(names, res["members"], res["label"]):
            top = largest_component(label)
            for v, c in zip(members, label):
                f.write(f"{name}\t{genes[int(v)]}\t{int(c)}\t{int(int(c) == top)}\n")


def main(argv=None):
    from . import proximity as P
    from .set_modules import ModuleEngine
    args = parse_args(argv)
    t0 = time.time()
    try:
        sets, names, _ = read_sets(args)
        net = P.read_network(args.network)
    except (OSError, ValueError) as e:
        sys.exit(f"disease_modules: {e}")
    eng = ModuleEngine(net)
    try:
        res = eng.module_table([sets[n] for n in names], 1 if args.diseases else 0, n_random=args.n_random, seed=args.seed,
                               min_bin_size=args.min_bin_size)
    except ProximityError as e:
        sys.exit(f"disease_modules: {e}")
    finally:
        eng.close()
    write_table(args.out, names, res)
    print(f"wrote {args.out}")
    if args.members:
        write_members(args.members, names, net.names, res)
        print(f"wrote {args.members}")
    if args.null:
        write_null(args.null, [res["null_lcc"], res["null_edges"]])
        print(f"wrote {args.null}")
    q = res["lcc_stats"]["q"]
    print(f"disease_modules: {len(names)} sets, n_random={args.n_random}, LCC {net.n} nodes, {int(np.sum(q <= 0.05))} with lcc.q <= 0.05, "
          f"{time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
