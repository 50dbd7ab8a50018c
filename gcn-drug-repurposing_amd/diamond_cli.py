"""The command line of DIAMOnD (Ghiassian, Menche and Barabasi 2015): grow a module from every disease's genes, every drug's targets or
every line of a seeds file, on the GPU, and, on request, validate the growth by leaving seeds out and counting how many come back."""
from __future__ import annotations

import argparse
import sys
import time

import numpy as np

from ._sets_cli import add_set_source, load_seed_sets, read_sets  # noqa: F401  (load_seed_sets: this module's callers import it here)
from .proximity import ProximityError
from .proximity_cli import _fmt

HEADER = ["set", "rank", "gene", "k", "kb", "logp", "p"]
SUMMARY_HEADER = ["set", "n.seeds", "n.added", "lcc.seeds", "lcc.module"]
RECOVERY_HEADER = ["set", "rank", "recovered", "held"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="diamond.py", description="DIAMOnD: grow disease modules from seed genes on the GPU")
    p.add_argument("--network", required=True, help="gene network .sif (gene rel gene), read as undirected; its LCC is used")
    add_set_source(p, seeds=True, null=False)
    p.add_argument("--n-add", default=200, type=int, help="nodes to add to every set")
    p.add_argument("--alpha", default=1, type=int, help="the seeds' weight, an integer >= 1")
    p.add_argument("--out", default="modules.tsv", help="the added nodes, one row per set and rank")
    p.add_argument("--summary", default=None, help="also write per set the largest connected component of the seeds and of the module")
    p.add_argument("--holdout", default=None, type=float, help="leave-out validation: the fraction of every set to hold out")
    p.add_argument("--repeats", default=100, type=int, help="hold-outs per set")
    p.add_argument("--seed", default=0, type=int, help="seed of the hold-out draws")
    p.add_argument("--recovery", default="recovery.tsv", help="the validation's table, one row per set and rank")
    args = p.parse_args(argv)
    if args.n_add < 1:
        p.error(f"--n-add {args.n_add} must be >= 1")
    if args.alpha < 1:
        p.error(f"--alpha {args.alpha} must be >= 1")
    if args.holdout is not None and not 0.0 < args.holdout < 1.0:
        p.error(f"--holdout {args.holdout} must be in (0, 1)")
    if args.repeats < 1:
        p.error(f"--repeats {args.repeats} must be >= 1")
    return args


def write_modules(path, names, genes, res):
    """modules.tsv: one row per set and added node, in the order of `names` (res: DiamondEngine.grow's return; genes: the network's
    names by node index); a set whose surroundings were used up has fewer rows"""
    with open(path, "w") as f:
        f.write("\t".join(HEADER) + "\n")
        for i, name in enumerate(names):
            for r, v in enumerate(res["node"][i]):
                if v < 0:
                    break
                f.write(f"{name}\t{r + 1}\t{genes[int(v)]}\t{int(res['k'][i, r])}\t{int(res['kb'][i, r])}\t{_fmt(res['logp'][i, r])}\t"
                        f"{_fmt(res['p'][i, r])}\n")


def write_summary(path, names, n_seeds, n_added, lcc_seeds, lcc_module):
    with open(path, "w") as f:
        f.write("\t".join(SUMMARY_HEADER) + "\n")
        for row in zip(names, n_seeds, n_added, lcc_seeds, lcc_module):
            f.write("\t".join([row[0]] + [str(int(x)) for x in row[1:]]) + "\n")


def write_recovery(path, names, rec):
    with open(path, "w") as f:
        f.write("\t".join(RECOVERY_HEADER) + "\n")
        for i, name in enumerate(names):
            for r, x in enumerate(rec["recovered"][i]):
                f.write(f"{name}\t{r + 1}\t{int(x)}\t{int(rec['held'][i])}\n")


def module_lcc(eng, sets, node):
    """largest connected component of every seed set and of seeds + added nodes, by the engine's components -> two int64 [n_sets]"""
    from ._network_engine import MAX_SET
    both = [u for s, row in zip(sets, node) for u in (s, np.unique(np.concatenate([s, row[row >= 0]])))]
    width = max(1, max(len(u) for u in both))
    if width > MAX_SET:
        raise ProximityError(f"a module of {width} nodes; the component search takes at most {MAX_SET}")
    nodes, sizes, _ = eng.pack(both)
    lcc = eng.components(nodes.reshape(len(sets), 2, -1), sizes.reshape(len(sets), 2))[0].cpu().numpy().astype(np.int64)
    return lcc[:, 0], lcc[:, 1]


def main(argv=None):
    from . import proximity as P
    from .diamond import DiamondEngine
    args = parse_args(argv)
    t0 = time.time()
    try:
        sets, names, _ = read_sets(args)
        net = P.read_network(args.network)
    except (OSError, ValueError) as e:
        sys.exit(f"diamond: {e}")
    members = [net.node_set(sets[n]) for n in names]
    eng = DiamondEngine(net)
    try:
        res = eng.grow(members, n_add=args.n_add, alpha=args.alpha)
        rec = None
        if args.holdout is not None:
            rec = eng.recovery(members, holdout=args.holdout, repeats=args.repeats, seed=args.seed, n_add=args.n_add, alpha=args.alpha)
        lcc = module_lcc(eng, members, res["node"]) if args.summary else None
    except ProximityError as e:
        sys.exit(f"diamond: {e}")
    finally:
        eng.close()
    write_modules(args.out, names, net.names, res)
    print(f"wrote {args.out}")
    if lcc is not None:
        write_summary(args.summary, names, [len(m) for m in members], (res["node"] >= 0).sum(axis=1), *lcc)
        print(f"wrote {args.summary}")
    if rec is not None:
        write_recovery(args.recovery, names, rec)
        print(f"wrote {args.recovery}")
    print(f"diamond: {len(names)} sets, n_add={args.n_add}, alpha={args.alpha}, LCC {net.n} nodes, {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
