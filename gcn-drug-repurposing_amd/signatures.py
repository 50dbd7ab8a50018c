"""drug_signatures.py: do drugs with similar diffusion profiles perturb gene expression similarly?  The multiscale interactome's validation
against the Broad Connectivity Map: the reference ships the table (data/bcm_df.tsv, multiscale/README.md dataset 8: one row per drug with
its DrugBank id, name, signature id, cell line, dose and time, then one column per landmark gene, headed by its Entrez id) and no code that
reads it.  Two drug x drug matrices over the table's drugs -- the distance between diffusion profiles and the distance between expression
signatures -- are correlated over their n (n - 1) / 2 pairs, and the correlation is tested by Mantel's permutation test (mantel.py).

Both matrices are diffusion.compare_profiles' (the signatures are a host [drugs][genes] array to it, compared by the kernels and the
metrics of the profiles) and stay on the device; the null is a HIP kernel (csrc/matrix_mantel.hip; no CPU fallback)."""
from __future__ import annotations

import argparse
import csv
import json
import sys

import numpy as np

from . import mantel as M
from . import predict
from .diffusion import ALL_METRICS as METRICS
from .predict import PredictError, write_tsv

MAX_POOL = M.MAX_N
REPLICATES = ("refuse", "mean")
HEADER = ["drug_a", "drug_b", "name_a", "name_b", "profile_distance", "signature_distance"]
RANK_HEADER = ["profile_rank", "signature_rank"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: diffusion profiles against gene-expression signatures, Mantel's test "
                                            "(drug_signatures.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as predict_drug.py reads it")
    p.add_argument("--signatures", required=True, type=str, help="the signature table (data/bcm_df.tsv): drug, drug_name, one column per Entrez id")
    p.add_argument("--metric", default="correlation", type=str, help="distance between two profiles: " + ", ".join(METRICS) + " (default: correlation)")
    p.add_argument("--signature-metric", default="correlation", type=str,
                   help="distance between two signatures: " + ", ".join(METRICS) + " (default: correlation)")
    p.add_argument("--method", default="spearman", type=str, help="correlation of the pair values: " + ", ".join(M.METHODS) + " (default: spearman)")
    p.add_argument("--permutations", default=10000, type=int, help="relabellings of the drugs in the null (default: 10000)")
    p.add_argument("--seed", default=0, type=int, help="seed of the relabellings (default: 0)")
    p.add_argument("--replicates", default="refuse", type=str, help="a drug with several rows: refuse, or mean = average them (default: refuse)")
    p.add_argument("--out", default="signature_pairs.tsv", type=str, help=", ".join(HEADER) + " (default: signature_pairs.tsv)")
    p.add_argument("--matrix", default=None, type=str, help="also save the pool x pool profile distance matrix as .npy (pool in node order)")
    p.add_argument("--signature-matrix", default=None, type=str, help="also save the pool x pool signature distance matrix as .npy")
    p.add_argument("--null", default=None, type=str, help="also save the null correlations [permutations] as .npy")
    return p.parse_args(argv)


def check_args(metric, signature_metric, method, permutations, replicates):
    """every refusal that needs neither the table, the graph nor the GPU"""
    for flag, m in (("--metric", metric), ("--signature-metric", signature_metric)):
        if m not in METRICS:
            raise PredictError(f"{flag} {m!r} is unknown; choose one of {', '.join(METRICS)}")
    if method not in M.METHODS:
        raise PredictError(f"--method {method!r} is unknown; choose one of {', '.join(M.METHODS)}")
    if permutations < 1:
        raise PredictError(f"--permutations {permutations} must be at least 1")
    if replicates not in REPLICATES:
        raise PredictError(f"--replicates {replicates!r} is unknown; choose one of {', '.join(REPLICATES)}")


def read_signatures(path, replicates="refuse"):
    """the table -> (the drug ids in order of first appearance, {drug id: name} ("" without a drug_name column), the gene ids = the headers
    made of digits only, in file order, fp64 [drugs][genes]).  A drug with several rows is refused under "refuse" and averaged column by
    column under "mean"; a cell that is no number is refused with its drug and gene"""
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    if not rows:
        raise PredictError(f"--signatures {path}: the table is empty")
    head = rows[0]
    if "drug" not in head:
        raise PredictError(f"--signatures {path}: column 'drug' is missing")
    at, at_name = head.index("drug"), head.index("drug_name") if "drug_name" in head else None
    gene_cols = [i for i, h in enumerate(head) if h.isascii() and h.isdigit()]
    if not gene_cols:
        raise PredictError(f"--signatures {path}: no gene column (a header made of digits, an Entrez id)")
    genes = [head[i] for i in gene_cols]
    values, names = {}, {}
    for r in rows[1:]:
        if not any(r):
            continue
        r = r + [""] * (len(head) - len(r))
        drug = r[at]
        vec = np.empty(len(genes))
        for k, i in enumerate(gene_cols):
            try:
                vec[k] = float(r[i])
            except ValueError:
                raise PredictError(f"--signatures {path}: drug {drug!r}, gene {genes[k]}: {r[i]!r} is not a number") from None
        values.setdefault(drug, []).append(vec)
        names.setdefault(drug, r[at_name] if at_name is not None else "")
    drugs = list(values)
    if replicates == "refuse":
        for d in drugs:
            if len(values[d]) > 1:
                raise PredictError(f"--signatures {path}: drug {d!r} has {len(values[d])} rows; --replicates mean averages them")
    table = np.stack([np.mean(values[d], axis=0) if len(values[d]) > 1 else values[d][0] for d in drugs]) if drugs else np.zeros((0, len(genes)))
    return drugs, names, genes, table


def pool_of(drugs, nodelist, profiles, g):
    """-> (the pool: the table's drugs that are nodes with a diffusion profile, in node order; the table's drugs that are no nodes; those
    without a profile)"""
    no_node = [n for n in drugs if n not in g.adj]
    no_profile = [n for n in drugs if n in g.adj and n not in profiles]
    pos = {n: i for i, n in enumerate(nodelist)}
    pool = sorted((n for n in drugs if n in g.adj and n in profiles), key=pos.__getitem__)
    return pool, no_node, no_profile


def summary_line(rec, genes, method, permutations, seed, out):
    return (f"signatures: {rec['n']} drugs, {rec['n_pairs']} pairs, {genes} genes: {method} r = {rec['r']!r}, z = {rec['z']!r}, "
            f"p = {rec['p_greater']!r} (two-sided {rec['p_two_sided']!r}; {permutations} permutations, seed {seed}): {out}")


def run(s, signatures_path, metric="correlation", signature_metric="correlation", method="spearman", permutations=10000, seed=0,
        replicates="refuse", out="signature_pairs.tsv", matrix=None, signature_matrix=None, null=None):
    """the command on predict.Settings s -> (the pool, the gene ids, mantel's record)"""
    from .diffusion import compare_profiles
    check_args(metric, signature_metric, method, permutations, replicates)
    drugs, names, genes, table = read_signatures(signatures_path, replicates)
    if not s.diffusion_dir:
        raise PredictError("config: diffusion.diffusion_embs_dir is missing")
    g = predict.build_graph(s)
    nodelist, profiles = predict.diffusion_profiles(s, g)
    pool, no_node, no_profile = pool_of(drugs, nodelist, profiles, g)
    for skipped, why in ((no_node, "not in the graph"), (no_profile, "no diffusion profile")):
        if skipped:
            print(f"drug_signatures: skipped {len(skipped)} drugs of the table: {why}", file=sys.stderr)
    if len(pool) > MAX_POOL:
        raise PredictError(f"the pool of {len(pool)} drugs is above {MAX_POOL}, the most a permutation is drawn over")
    if len(pool) < 3:
        raise PredictError(f"the pool of {len(pool)} drugs with a signature and a diffusion profile is below 3: a correlation over pairs needs 3")
    row = {n: i for i, n in enumerate(drugs)}
    dist = predict.profile_distances(profiles, pool, pool, metric)
    try:
        sig = compare_profiles(table[[row[n] for n in pool]], None, None, signature_metric)
        rec, null_host = M.mantel(dist, sig, method, permutations, seed, labels=pool, return_null=True)
        iu, dv = M.pair_values(dist)
        _, ev = M.pair_values(sig)
        cols = [dv, ev] + ([M.pair_ranks(dv), M.pair_ranks(ev)] if method == "spearman" else [])
    except ValueError as e:
        raise PredictError(str(e)) from None
    header = HEADER + (RANK_HEADER if method == "spearman" else [])
    iu = iu.cpu().numpy()
    cols = [c.cpu().numpy() for c in cols]
    write_tsv(out, header, [[pool[i], pool[j], names[pool[i]], names[pool[j]]] + [float(c[k]) for c in cols]
                            for k, (i, j) in enumerate(zip(iu[0], iu[1]))])
    for path, what in ((matrix, dist), (signature_matrix, sig)):
        if path:
            np.save(path, what.cpu().numpy())
    if null:
        np.save(null, null_host)
    return pool, genes, rec


def main(argv=None):
    args = parse_args(argv)
    try:
        check_args(args.metric, args.signature_metric, args.method, args.permutations, args.replicates)
        s = predict.Settings(predict.load_config(args.config))
        pool, genes, rec = run(s, args.signatures, args.metric, args.signature_metric, args.method, args.permutations, args.seed, args.replicates,
                               args.out, args.matrix, args.signature_matrix, args.null)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"drug_signatures: {e}", file=sys.stderr)
        sys.exit(2)
    print(summary_line(rec, len(genes), args.method, args.permutations, args.seed, args.out))
