"""The command line of the random walk with restart: rank the network's genes from every disease's genes, every drug's targets or every
line of a seeds file, on the GPU; on request against degree-matched random sets, and with the leave-out validation of diamond.py."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._sets_cli import add_null_arguments, add_set_source, check_null_arguments, read_sets
from .diamond_cli import write_recovery
from .proximity import ProximityError
from .proximity_cli import _fmt

HEADER = ["set", "rank", "gene", "score"]
NULL_HEADER = HEADER + ["null.mean", "null.sd", "z", "ge", "p"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="rwr.py", description="random walk with restart: rank genes from seed sets on the GPU")
    p.add_argument("--network", required=True, help="gene network .sif (gene rel gene), read as undirected; its LCC is used")
    add_set_source(p, seeds=True, null=True)
    p.add_argument("--n-add", default=200, type=int, help="genes to rank per set (at most 1024)")
    p.add_argument("--restart", default=0.75, type=float, help="the probability of a restart on the set, in (0, 1)")
    p.add_argument("--tol", default=1e-6, type=float, help="stop when the L1 change of an iteration is below this")
    p.add_argument("--max-iter", default=1000, type=int, help="iterations at the most")
    add_null_arguments(p, or_zero=True)
    p.set_defaults(n_random=0)
    p.add_argument("--rank-by", default="p", choices=("p", "z"), help="rank by the visit probability or by its z against the random sets")
    p.add_argument("--out", default="ranking.tsv", help="the ranked genes, one row per set and rank")
    p.add_argument("--genes", default=None, help="also write every set with its ranked genes as a gene table in the layout of "
                   "disease_genes.tsv: what disease_modules.py and proximity.py --diseases read")
    p.add_argument("--holdout", default=None, type=float, help="leave-out validation: the fraction of every set to hold out")
    p.add_argument("--repeats", default=100, type=int, help="hold-outs per set")
    p.add_argument("--holdout-seed", default=0, type=int, help="seed of the hold-out draws (diamond.py's --seed)")
    p.add_argument("--recovery", default="recovery.tsv", help="the validation's table, one row per set and rank (the layout of diamond.py's)")
    args = p.parse_args(argv)
    if not 1 <= args.n_add <= 1024:
        p.error(f"--n-add {args.n_add} must be in [1, 1024]")
    if not 0.0 < args.restart < 1.0:
        p.error(f"--restart {args.restart} must be in (0, 1)")
    if not args.tol >= 0.0:
        p.error(f"--tol {args.tol} must be >= 0")
    if args.max_iter < 1:
        p.error(f"--max-iter {args.max_iter} must be >= 1")
    check_null_arguments(p, args, or_zero=True)
    if args.rank_by == "z" and args.n_random == 0:
        p.error("--rank-by z needs --n-random >= 2")
    if args.holdout is not None and not 0.0 < args.holdout < 1.0:
        p.error(f"--holdout {args.holdout} must be in (0, 1)")
    if args.repeats < 1:
        p.error(f"--repeats {args.repeats} must be >= 1")
    return args


def write_ranking(path, names, genes, res):
    """ranking.tsv: one row per set and ranked gene, in the order of `names` (res: RwrEngine.rank's or score_table's return; genes: the
    network's names by node index); a set with fewer candidates has fewer rows, an empty set none"""
    null = "mean" in res
    with open(path, "w") as f:
        f.write("\t".join(NULL_HEADER if null else HEADER) + "\n")
        for i, name in enumerate(names):
            for r, v in enumerate(res["node"][i]):
                if v < 0:
                    break
                cells = [name, str(r + 1), genes[int(v)], _fmt(res["p" if null else "score"][i, r])]
                if null:
                    cells += [_fmt(res["mean"][i, r]), _fmt(res["sd"][i, r]), _fmt(res["z"][i, r]), str(int(res["ge"][i, r])), _fmt(res["emp_p"][i, r])]
                f.write("\t".join(cells) + "\n")


def write_genes(path, names, genes, members, node):
    """every set with its ranked genes as a gene table: `<empty>\\t<name>\\t<gene>...`, seeds first, then the genes in rank order"""
    with open(path, "w") as f:
        for name, seeds, row in zip(names, members, node):
            f.write("\t".join(["", name] + [genes[int(v)] for v in seeds] + [genes[int(v)] for v in row if v >= 0]) + "\n")


def main(argv=None):
    from . import proximity as P
    from .rwr import RwrEngine
    args = parse_args(argv)
    t0 = time.time()
    try:
        sets, names, _ = read_sets(args)
        net = P.read_network(args.network)
    except (OSError, ValueError) as e:
        sys.exit(f"rwr: {e}")
    members = [net.node_set(sets[n]) for n in names]
    walk = dict(n_add=args.n_add, restart=args.restart, tol=args.tol, max_iter=args.max_iter)
    eng = None
    try:
        eng = RwrEngine(net)
        if args.n_random:
            res = eng.score_table([sets[n] for n in names], 0 if args.drugs else 1, n_random=args.n_random, seed=args.seed,
                                  min_bin_size=args.min_bin_size, rank_by=args.rank_by, **walk)
        else:
            res = eng.rank(members, **walk)
        rec = None
        if args.holdout is not None:
            rec = eng.recovery(members, holdout=args.holdout, repeats=args.repeats, seed=args.holdout_seed, **walk)
    except ProximityError as e:
        sys.exit(f"rwr: {e}")
    finally:
        if eng is not None:
            eng.close()
    write_ranking(args.out, names, net.names, res)
    print(f"wrote {args.out}")
    if args.genes:
        write_genes(args.genes, names, net.names, members, res["node"])
        print(f"wrote {args.genes}")
    if rec is not None:
        write_recovery(args.recovery, names, rec)
        print(f"wrote {args.recovery}")
    print(f"rwr: {len(names)} sets, n_add={args.n_add}, restart={args.restart}, n_random={args.n_random}, LCC {net.n} nodes, "
          f"{int(np.max(res['iters'], initial=0))} iterations at the most, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
