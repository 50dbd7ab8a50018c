"""What the command lines over gene sets share (modules_cli, diamond_cli, connectors_cli): where the sets come from -- --diseases,
--drugs or --seeds, narrowed by --set -- and the arguments and the file of a null of degree-matched random sets."""
from __future__ import annotations

import numpy as np

from .proximity import ProximityError, disease_key


def add_set_source(p, seeds, null):
    """the mutually exclusive --diseases / --drugs and, with `seeds`, --seeds and the --set filter; with `null` the help says which
    random sets of proximity.py a source draws"""
    which = p.add_mutually_exclusive_group(required=True)
    which.add_argument("--diseases", default=None,
                       help="disease gene table (disease_genes.tsv)" + (": the to-side random sets of proximity.py" if null else ""))
    which.add_argument("--drugs", default=None,
                       help="drug target pickle (drug_to_geneids.pcl.all)" + (": the from-side random sets of proximity.py" if null else ""))
    if seeds:
        which.add_argument("--seeds", default=None, help="a seeds file: one set per line, `name<TAB>gene<TAB>gene...`"
                           + (" (random sets as for diseases)" if null else ""))
        p.add_argument("--set", action="append", default=None, metavar="NAME", help="grow only this set (may be repeated)")


def load_seed_sets(path):
    """{set name: set of gene ids (str)} from a seeds file (`name\\tgene\\tgene...`; empty lines and lines starting with # are skipped;
    a name on several lines collects them all).  The name is kept as written"""
    out = {}
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if not p[0] or p[0].startswith("#"):
                continue
            out.setdefault(p[0], set()).update(g for g in p[1:] if g)
    return out


def read_sets(args):
    """parsed arguments -> ({name: gene ids}, the names to work on, sorted, the file's path).  A --set names a disease as proximity's
    tables do (disease_key), any other set as written.  An empty file and an unknown name are ProximityErrors"""
    from . import proximity as P
    seeds, wanted = getattr(args, "seeds", None), getattr(args, "set", None)
    path = args.diseases or args.drugs or seeds
    sets = P.load_disease_genes(path) if args.diseases else P.load_drug_targets(path) if args.drugs else load_seed_sets(path)
    if not sets:
        raise ProximityError(f"{path}: no gene set")
    if not wanted:
        return sets, sorted(sets), path
    wanted = [disease_key(s) if args.diseases else s for s in wanted]
    unknown = [s for s in wanted if s not in sets]
    if unknown:
        raise ProximityError(f"{path}: no set named {unknown[0]!r}")
    return sets, sorted(set(wanted)), path


def add_null_arguments(p, or_zero):
    p.add_argument("--n-random", default=1000, type=int, help="degree-matched random samples per set" + ("; 0 skips the null" if or_zero else ""))
    p.add_argument("--seed", default=452456, type=int, help="seed of the counter-based generator of the random sets")
    p.add_argument("--min-bin-size", default=100, type=int, help="smallest degree bin")


def check_null_arguments(p, args, or_zero):
    if args.n_random < 2 and not (or_zero and args.n_random == 0):
        p.error(f"--n-random {args.n_random}: need at least 2 random samples for a standard deviation" + (", or 0 for no null" if or_zero else ""))
    if args.min_bin_size < 1:
        p.error(f"--min-bin-size {args.min_bin_size} must be >= 1")


def write_null(path, nulls):
    """the integer nulls, each [n_sets, n_random], as one int32 [n_sets][len(nulls)][n_random] .npy"""
    with open(path, "wb") as f:                  # np.save on a name would append .npy
        np.save(f, np.stack(nulls, axis=1).astype(np.int32))
