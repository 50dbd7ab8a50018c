"""drug_classes.py: do the drugs of one ATC class have more similar diffusion profiles than random drugs do?  The multiscale interactome's
third validation beside the treatment AUC (evaluate.py) and the gene knock-outs (knockout.py): the reference ships the table
(data/drug_classification_df.tsv, multiscale/README.md dataset 7: DrugBank id, ATC code, the four ATC levels with their names) and no code
that reads it.  Per class: the mean distance over its drug pairs, against the same mean over random drug sets of the class's size.

The distance matrix is diffusion.compare_profiles' and stays on the device; the sums over it are HIP kernels (csrc/class_cohesion.hip; no
CPU fallback): gss_pair_sums_lists for the classes, gss_pair_sums_random for the null -- one seeded permutation of the pool per sample, whose
first m places are the random set of size m, so one launch serves every class size of every level.  What comes back is [samples][sizes]
sums; mean, standard deviation, z, the empirical p and the Benjamini-Hochberg q over them are host numpy."""
from __future__ import annotations

import argparse
import csv
import json
import sys

import numpy as np

from . import _lib, predict
from ._nulls import NULL_CHUNK_BYTES, benjamini_hochberg, chunked_null, device_lists, int32_array, square_matrix  # noqa: F401
from .diffusion import ALL_METRICS as METRICS
from .predict import PredictError, write_tsv

MAX_POOL = 4096               # gss_pair_sums_random sorts a sample's permutation in LDS
LEVELS = (1, 2, 3, 4)
HEADER = ["level", "class", "class_name", "n_drugs", "n_pairs", "mean_distance", "null_mean", "null_std", "z", "p", "q"]


# ---- the kernels ---------------------------------------------------------------------------------------------------------------------

def pair_sums(dist, lists, labels=None):
    """the sum of dist over the pairs of each list -> device tensor fp64 [len(lists)]: for the ordered list a, T = r_1 + ... + r_{m-1} with
    r_j = the sum of dist[a[j]][a[i]] over i < j (gss_pair_sums_lists; the order of the additions depends on the list alone, so a list has
    the same bits alone and among others).  dist: the square device fp64 tensor compare_profiles returned, used in place, or a host array,
    uploaded; assumed symmetric.  lists: sequences of row numbers in [0, n), any order and length; one shorter than 2 gives 0.0.  A NaN in
    dist is refused with the row's label (labels[i], else its number).  No CPU fallback."""
    import torch
    d = square_matrix(dist, "pair_sums", labels)
    hl = [int32_array(f"list {c}", l, "pair_sums") for c, l in enumerate(lists)]
    out = torch.empty(len(hl), dtype=torch.float64, device=d.device)
    if not hl:
        return out
    with torch.cuda.device(d.device):
        d_ptr, d_idx = device_lists(hl, "pair_sums", "lists", d.device)
        _lib.check(_lib.load().gss_pair_sums_lists(d.shape[0], d.data_ptr(), _lib.row_stride(d), len(hl), d_ptr.data_ptr(), d_idx.data_ptr(),
                                                   out.data_ptr(), _lib.current_stream()), "gss_pair_sums_lists")
    return out


def random_pair_sums(dist, sizes, samples, seed=0, first=0, perms=False, labels=None):
    """the same sums over random sets -> device tensor fp64 [samples][len(sizes)]: row s - first holds T(m) for every m in sizes of the
    first m places of permutation number s of the n rows, s = first .. first + samples - 1 (gss_pair_sums_random: rows sorted by the
    counter-based key of (seed, s, row), a pure function of its arguments -- a call equals the same samples in any split through `first`,
    and a size has the same bits alone and among others).  sizes: strictly ascending in [2, n]; n <= 4096.  perms=True also returns the
    permutations' prefixes, device int32 [samples][sizes[-1]].  dist and labels as in pair_sums.  No CPU fallback."""
    import torch
    d = square_matrix(dist, "random_pair_sums", labels)
    hs = int32_array("sizes", sizes, "random_pair_sums")
    P, ns = int(samples), len(hs)
    with torch.cuda.device(d.device):
        sums = torch.empty(max(P, 0), ns, dtype=torch.float64, device=d.device)
        d_sizes = torch.from_numpy(hs if ns else np.zeros(1, dtype=np.int32)).to(d.device)
        perm = torch.empty(max(P, 0), int(hs[-1]) if ns and hs[-1] > 0 else 0, dtype=torch.int32, device=d.device) if perms else None
        _lib.check(_lib.load().gss_pair_sums_random(d.shape[0], d.data_ptr(), _lib.row_stride(d), _lib.seed64(seed), int(first), P, ns, d_sizes.data_ptr(),
                                                    sums.data_ptr(), _lib.ptr(perm), _lib.current_stream()), "gss_pair_sums_random")
    return (sums, perm) if perms else sums


def null_sums(d, sizes, samples, seed=0):
    """random_pair_sums brought to the host -> fp64 [samples][len(sizes)], in calls of at most NULL_CHUNK_BYTES of sums each"""
    return chunked_null(lambda count, first: random_pair_sums(d, sizes, count, seed, first), samples, 8 * len(sizes))


# ---- the statistics (host) -----------------------------------------------------------------------------------------------------------

def cohesion_stats(observed, n_drugs, sizes, null):
    """per class c of n_drugs[c] = m drugs with the pair sum observed[c] = T_c, against column sizes.index(m) of the null sums [P][sizes]:
    K = m (m - 1) / 2 pairs, mean_distance = T_c / K, null_mean and null_std = np.mean and np.std (ddof 0) of T_s / K over the samples,
    z = (mean_distance - null_mean) / null_std (nan when the std is 0) and p = (1 + #{s: T_s <= T_c}) / (P + 1), counted on the sums -> a
    list of dicts"""
    col = {int(m): k for k, m in enumerate(sizes)}
    null = np.asarray(null, dtype=np.float64)
    out = []
    for T, m in zip(observed, n_drugs):
        T, m = float(T), int(m)
        K = m * (m - 1) // 2
        t = null[:, col[m]]
        quot = t / K
        mean, nm, ns = T / K, float(np.mean(quot)), float(np.std(quot))
        out.append({"n_drugs": m, "n_pairs": K, "mean_distance": mean, "null_mean": nm, "null_std": ns,
                    "z": (mean - nm) / ns if ns > 0 else float("nan"), "p": (1 + int(np.count_nonzero(t <= T))) / (len(t) + 1)})
    return out


def class_cohesion(dist, classes, samples, seed=0, labels=None, return_null=False):
    """classes: {name: rows} or a sequence of row lists (rows of dist, each drug once, at least 2) -> one dict per class, in order: "class"
    (the name or the position), n_drugs, n_pairs, mean_distance, null_mean, null_std, z, p (cohesion_stats) from pair_sums of the classes
    and `samples` random sets per distinct class size (random_pair_sums with `seed`).  return_null=True: -> (records, sizes, null sums
    [samples][sizes] on the host)."""
    names = list(classes.keys()) if isinstance(classes, dict) else list(range(len(classes)))
    lists = [list(classes[k]) for k in names]
    for k, l in zip(names, lists):
        if len(l) < 2 or len(set(l)) != len(l):
            raise ValueError(f"class_cohesion: class {k!r} must list at least 2 drugs, each once")
    if not lists:
        raise ValueError("class_cohesion: no class")
    if int(samples) < 1:
        raise ValueError(f"class_cohesion: samples={samples} must be at least 1")
    d = square_matrix(dist, "class_cohesion", labels)
    sizes = sorted({len(l) for l in lists})
    observed = pair_sums(d, lists).cpu().numpy()
    null = null_sums(d, sizes, int(samples), seed)
    rec = [{"class": k, **r} for k, r in zip(names, cohesion_stats(observed, [len(l) for l in lists], sizes, null))]
    return (rec, sizes, null) if return_null else rec


# ---- the program ---------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: ATC drug-class coherence of the diffusion profiles (drug_classes.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as predict_drug.py reads it")
    p.add_argument("--classes", required=True, type=str, help="the drug-class table (data/drug_classification_df.tsv): db_id, level_k, level_k_name")
    p.add_argument("--levels", default="1,2,3,4", type=str, help="ATC levels to score, comma-separated (default: 1,2,3,4)")
    p.add_argument("--metric", default="correlation", type=str, help="distance between two profiles: " + ", ".join(METRICS) + " (default: correlation)")
    p.add_argument("--min-size", default=2, type=int, help="drop classes with fewer drugs in the pool (default: 2)")
    p.add_argument("--samples", default=10000, type=int, help="random drug sets per class size (default: 10000)")
    p.add_argument("--seed", default=0, type=int, help="seed of the random sets (default: 0)")
    p.add_argument("--out", default="classes.tsv", type=str, help=", ".join(HEADER) + " (default: classes.tsv)")
    p.add_argument("--matrix", default=None, type=str, help="also save the pool x pool distance matrix as .npy (pool in node order)")
    p.add_argument("--null", default=None, type=str, help="also save the null sums [samples][sizes] as .npy (sizes = the distinct class sizes, ascending)")
    return p.parse_args(argv)


def parse_levels(text, flag="--levels"):
    """flag: the option the refusals name (evaluate_auc.py calls it --class-levels)"""
    try:
        levels = [int(t) for t in str(text).split(",")]
    except ValueError:
        raise PredictError(f"{flag} {text!r} must be comma-separated integers out of 1,2,3,4") from None
    for k in levels:
        if k not in LEVELS:
            raise PredictError(f"{flag}: level {k} is unknown; the ATC levels are 1, 2, 3 and 4")
    if len(set(levels)) != len(levels):
        raise PredictError(f"{flag} {text!r} repeats a level")
    return sorted(levels)


def check_args(levels, metric, min_size, samples):
    """every refusal that needs neither the table, the graph nor the GPU -> the levels"""
    levels = parse_levels(levels)
    if metric not in METRICS:
        raise PredictError(f"--metric {metric!r} is unknown; choose one of {', '.join(METRICS)}")
    if samples < 1:
        raise PredictError(f"--samples {samples} must be at least 1")
    if min_size < 2:
        raise PredictError(f"--min-size {min_size} must be at least 2 (a class of one drug has no pair)")
    return levels


def read_classes(path, levels, flag="--classes"):
    """the table -> (the drug ids in order of first appearance, {level: {class code: [name, [drug ids, each once, in file order]]}}).  A drug
    carries one row per ATC code, so it can be in several classes of a level; an empty or NA code names no class.  flag: the option the
    refusals name (evaluate_auc.py calls it --by-class)"""
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    if not rows:
        raise PredictError(f"{flag} {path}: the table is empty")
    head = {h: i for i, h in enumerate(rows[0])}
    for col in ["db_id"] + [c for k in levels for c in (f"level_{k}", f"level_{k}_name")]:
        if col not in head:
            raise PredictError(f"{flag} {path}: column {col!r} is missing")
    drugs, table = {}, {k: {} for k in levels}
    for r in rows[1:]:
        if not any(r):
            continue
        r = r + [""] * (len(rows[0]) - len(r))
        drug = r[head["db_id"]]
        drugs.setdefault(drug, None)
        for k in levels:
            code = r[head[f"level_{k}"]]
            if code in ("", "NA"):
                continue
            entry = table[k].setdefault(code, [r[head[f"level_{k}_name"]], []])
            if drug not in entry[1]:
                entry[1].append(drug)
    return list(drugs), table


def pool_and_classes(drugs, table, nodelist, profiles, g, min_size):
    """-> (the pool: the table's drugs that are nodes with a diffusion profile and carry a code of a requested level, in node order;
    [(level, code, name, [pool rows])] of the classes with at least min_size drugs in the pool; the table's drugs that are no nodes; those
    without a profile)"""
    no_node = [n for n in drugs if n not in g.adj]
    no_profile = [n for n in drugs if n in g.adj and n not in profiles]
    coded = {n for by_code in table.values() for _, members in by_code.values() for n in members}
    pos = {n: i for i, n in enumerate(nodelist)}
    pool = sorted((n for n in drugs if n in g.adj and n in profiles and n in coded), key=pos.__getitem__)
    row = {n: i for i, n in enumerate(pool)}
    classes = []
    for k in sorted(table):
        for code in sorted(table[k]):
            name, members = table[k][code]
            rows = sorted(row[n] for n in members if n in row)
            if len(rows) >= min_size:
                classes.append((k, code, name, rows))
    return pool, classes, no_node, no_profile


def run(s, classes_path, levels="1,2,3,4", metric="correlation", min_size=2, samples=10000, seed=0, out="classes.tsv", matrix=None, null=None):
    """the command on predict.Settings s -> (the pool, the table's rows as dicts)"""
    levels = check_args(levels, metric, min_size, samples)
    drugs, table = read_classes(classes_path, levels)
    if not s.diffusion_dir:
        raise PredictError("config: diffusion.diffusion_embs_dir is missing")
    g = predict.build_graph(s)
    nodelist, profiles = predict.diffusion_profiles(s, g)
    pool, classes, no_node, no_profile = pool_and_classes(drugs, table, nodelist, profiles, g, min_size)
    for skipped, why in ((no_node, "not in the graph"), (no_profile, "no diffusion profile")):
        if skipped:
            print(f"drug_classes: skipped {len(skipped)} drugs of the table: {why}", file=sys.stderr)
    if len(pool) > MAX_POOL:
        raise PredictError(f"the pool of {len(pool)} drugs is above {MAX_POOL}, the most a random set is drawn from")
    if not classes:
        raise PredictError(f"no class has {min_size} drugs with a diffusion profile ({len(pool)} drugs in the pool)")
    dist = predict.profile_distances(profiles, pool, pool, metric)
    try:
        rec, _, null_host = class_cohesion(dist, [c[3] for c in classes], samples, seed, labels=pool, return_null=True)
    except ValueError as e:
        raise PredictError(str(e)) from None
    for r, (k, code, name, _) in zip(rec, classes):
        r.update({"level": k, "class": code, "class_name": name})
    for k in levels:
        of_level = [r for r in rec if r["level"] == k]
        for r, q in zip(of_level, benjamini_hochberg([r["p"] for r in of_level])):
            r["q"] = float(q)
    rec.sort(key=lambda r: (r["level"], r["p"], r["class"]))
    write_tsv(out, HEADER, [[r[h] for h in HEADER] for r in rec])
    if matrix:
        np.save(matrix, dist.cpu().numpy())
    if null:
        np.save(null, null_host)
    return pool, rec


def main(argv=None):
    args = parse_args(argv)
    try:
        check_args(args.levels, args.metric, args.min_size, args.samples)
        s = predict.Settings(predict.load_config(args.config))
        pool, rec = run(s, args.classes, args.levels, args.metric, args.min_size, args.samples, args.seed, args.out, args.matrix, args.null)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"drug_classes: {e}", file=sys.stderr)
        sys.exit(2)
    print(f"classes: {len(rec)} classes of {len(pool)} drugs, {args.samples} random sets per size: {args.out}")
