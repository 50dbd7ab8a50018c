"""The command line of the network proximity scorer: what method/test_proximity.py runs (toolbox wrappers.calculate_proximity over
the rows of a proximity table), for every pair of the table at once on the GPU."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

from .proximity import MEASURES, ProximityError


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="drug-disease network proximity (Guney et al. 2016) z-scores on the GPU")
    p.add_argument("--network", required=True, help="gene network .sif (gene rel gene), read as undirected; its LCC is used")
    p.add_argument("--drugs", required=True, help="drug target pickle {drug id: set(gene id)} (drug_to_geneids.pcl.all)")
    p.add_argument("--diseases", required=True, help="disease gene table (disease_genes.tsv)")
    p.add_argument("--pairs", default=None, help="a proximity .dat table whose group / disease columns list the pairs "
                                                 "(default: every drug against every disease)")
    p.add_argument("--measure", default="closest", help=f"{' | '.join(MEASURES)} | all")
    p.add_argument("--n-random", default=1000, type=int, help="degree-matched random samples per set")
    p.add_argument("--seed", default=452456, type=int, help="seed of the counter-based generator of the random sets")
    p.add_argument("--min-bin-size", default=100, type=int, help="smallest degree bin")
    p.add_argument("--out", default=".", help="output directory: one <measure>.dat per measure")
    args = p.parse_args(argv)
    if args.measure != "all" and args.measure not in MEASURES:
        p.error(f"--measure {args.measure}: choose from {', '.join(MEASURES)} or all")
    if args.n_random < 2:
        p.error(f"--n-random {args.n_random}: need at least 2 random samples for a standard deviation")
    if args.min_bin_size < 1:
        p.error(f"--min-bin-size {args.min_bin_size} must be >= 1")
    return args


def _fmt(x):
    return "NA" if not np.isfinite(x) else repr(float(x))


def main(argv=None):
    from . import proximity as P
    args = parse_args(argv)
    t0 = time.time()
    drugs = P.load_drug_targets(args.drugs)
    diseases = P.load_disease_genes(args.diseases)
    if args.pairs:
        pairs = P.read_table_pairs(args.pairs)
    else:
        pairs = [(a, b) for a in sorted(drugs) for b in sorted(diseases)]
    unknown_d = sorted({a for a, _ in pairs if a not in drugs})
    unknown_s = sorted({b for _, b in pairs if b not in diseases})
    if unknown_d or unknown_s:
        sys.exit(f"proximity: unknown drug(s) {unknown_d[:5]} / disease(s) {unknown_s[:5]} (not in --drugs / --diseases)")
    fn = sorted({a for a, _ in pairs})
    tn = sorted({b for _, b in pairs})
    fi, ti = {n: i for i, n in enumerate(fn)}, {n: i for i, n in enumerate(tn)}
    measures = MEASURES if args.measure == "all" else (args.measure,)
    net = P.read_network(args.network)
    eng = P.ProximityEngine(net)
    try:
        res = eng.score([drugs[n] for n in fn], [diseases[n] for n in tn],
                        pairs=None if not args.pairs else [(fi[a], ti[b]) for a, b in pairs], measures=measures,
                        n_random=args.n_random, seed=args.seed, min_bin_size=args.min_bin_size)
    except ProximityError as e:
        sys.exit(f"proximity: {e}")
    if not args.pairs:
        pairs = [(a, b) for a in fn for b in tn]
    os.makedirs(args.out, exist_ok=True)
    for m in measures:
        r = res[m]
        path = os.path.join(args.out, f"{m}.dat")
        with open(path, "w") as f:
            f.write("group disease n.target n.disease d z pval\n")
            for q, (a, b) in enumerate(pairs):
                na = r["n_from"][q] == 0 or r["n_to"][q] == 0
                f.write(f"{a} {b} {r['n_from'][q]} {r['n_to'][q]} "
                        f"{'NA' if na else _fmt(r['d'][q])} {'NA' if na else _fmt(r['z'][q])} {'NA' if na else _fmt(r['pval'][q])}\n")
        print(f"wrote {path}")
    print(f"proximity: {len(pairs)} pairs x {len(measures)} measure(s), n_random={args.n_random}, LCC {net.n} nodes "
          f"(diameter {eng.diameter}), {time.time() - t0:.1f} s")
    eng.close()


if __name__ == "__main__":
    main()
