"""compare_profiles.py: the nearest diffusion profiles of every chosen node.  The multiscale interactome "predicts whether the drug treats
the disease by comparing the diffusion profiles of a drug and a disease" (multiscale/README.md, overview (c)); the reference ships the
profiles and the drug-class table and never compares two of them.  This reads predict_drug.py's config, builds (or reuses) its profile
directory with the same functions (predict.py), computes the distance of every (row, column) pair on the GPU (diffusion.compare_profiles /
csrc/profile_dist.hip; no CPU fallback) and lists the K nearest columns of every row.  `--rows drugs --cols drugs` is the drug-drug
similarity the MSI data's drug-class table exists for.  The selection of K out of a few thousand columns is host numpy.
"""
from __future__ import annotations

import argparse
import json
import sys

import numpy as np

from . import predict
from .diffusion import ALL_METRICS as METRICS
from .msi import DRUG, INDICATION
from .predict import PredictError, write_tsv

SETS = ("drugs", "indications", "all")
HEADER = ["row", "row name", "rank", "column", "column name", "distance"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: nearest diffusion profiles of drugs / indications (compare_profiles.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as predict_drug.py reads it")
    p.add_argument("--metric", required=True, type=str, help="distance between two profiles: " + ", ".join(METRICS))
    p.add_argument("--rows", default="indications", type=str, help="the nodes to list neighbours for: " + ", ".join(SETS) + " (default: indications)")
    p.add_argument("--cols", default="drugs", type=str, help="the nodes to choose the neighbours from: " + ", ".join(SETS) + " (default: drugs)")
    p.add_argument("--row-id", action="append", default=None, help="list neighbours for this node id instead of the --rows set (repeatable)")
    p.add_argument("--col-id", action="append", default=None, help="choose neighbours from these node ids instead of the --cols set (repeatable)")
    p.add_argument("--top", default=10, type=int, help="neighbours per row (default: 10)")
    p.add_argument("--out", default="neighbours.tsv", type=str, help="row id, row name, rank, column id, column name, distance (default: neighbours.tsv)")
    p.add_argument("--matrix", default=None, type=str, help="also save the whole distance matrix [rows][columns] as .npy (columns in node order)")
    return p.parse_args(argv)


def check_args(metric, rows, cols, row_ids, col_ids, top):
    """every refusal that needs neither the graph nor the GPU"""
    if metric not in METRICS:
        raise PredictError(f"--metric {metric!r} is unknown; choose one of {', '.join(METRICS)}")
    for flag, value in (("--rows", rows), ("--cols", cols)):
        if value not in SETS:
            raise PredictError(f"{flag} {value!r} is unknown; choose one of {', '.join(SETS)}")
    for flag, ids in (("--row-id", row_ids), ("--col-id", col_ids)):
        if ids and len(set(ids)) != len(ids):
            raise PredictError(f"{flag}: repeated id in {ids}")
    if top < 1:
        raise PredictError(f"--top {top} must be at least 1")


def node_set(which, ids, flag, nodelist, profiles, g):
    """the chosen nodes: explicit ids as given, or the named set in node order; every one needs a profile"""
    if ids:
        for n in ids:
            if n not in g.adj:
                raise PredictError(f"{flag} {n!r} is not a node of the graph")
            if n not in profiles:
                raise PredictError(f"{flag} {n!r} has no diffusion profile (only drugs and indications with proteins have one)")
        return list(ids)
    want = {"drugs": (DRUG,), "indications": (INDICATION,), "all": (DRUG, INDICATION)}[which]
    return [n for n in nodelist if g.type.get(n) in want and n in profiles]


def select(dist, row_nodes, col_nodes, top):
    """per row the `top` nearest columns: ascending distance, ties by the column's position, the row's own id never listed
    -> [(row position, rank from 1, column position)]"""
    out = []
    for i, r in enumerate(row_nodes):
        order = [j for j in np.argsort(dist[i], kind="stable") if col_nodes[j] != r][:top]
        out += [(i, k + 1, int(j)) for k, j in enumerate(order)]
    return out


def run(s, metric, rows="indications", cols="drugs", row_ids=None, col_ids=None, top=10, out="neighbours.tsv", matrix=None):
    """the command on predict.Settings s -> (rows, columns, host distance matrix [rows][columns])"""
    check_args(metric, rows, cols, row_ids, col_ids, top)
    if not s.diffusion_dir:
        raise PredictError("config: diffusion.diffusion_embs_dir is missing")
    g = predict.build_graph(s)
    nodelist, profiles = predict.diffusion_profiles(s, g)
    pos = {n: i for i, n in enumerate(nodelist)}
    row_nodes = node_set(rows, row_ids, "--row-id", nodelist, profiles, g)
    col_nodes = sorted(node_set(cols, col_ids, "--col-id", nodelist, profiles, g), key=pos.__getitem__)   # ties go by the node order
    if not row_nodes or not col_nodes:
        raise PredictError(f"nothing to compare: {len(row_nodes)} rows, {len(col_nodes)} columns have a diffusion profile")
    dist = predict.profile_distances(profiles, row_nodes, col_nodes, metric).cpu().numpy()
    table = [[row_nodes[i], g.node2name.get(row_nodes[i]), rank, col_nodes[j], g.node2name.get(col_nodes[j]), float(dist[i, j])]
             for i, rank, j in select(dist, row_nodes, col_nodes, top)]
    write_tsv(out, HEADER, table)
    if matrix:
        np.save(matrix, dist)
    return row_nodes, col_nodes, dist


def main(argv=None):
    args = parse_args(argv)
    try:
        check_args(args.metric, args.rows, args.cols, args.row_id, args.col_id, args.top)
        s = predict.Settings(predict.load_config(args.config))
        rows, cols, _ = run(s, args.metric, args.rows, args.cols, args.row_id, args.col_id, args.top, args.out, args.matrix)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"compare_profiles: {e}", file=sys.stderr)
        sys.exit(2)
    print(f"{args.metric}: {len(rows)} rows x {len(cols)} columns: {args.out}" + (f", {args.matrix}" if args.matrix else ""))
