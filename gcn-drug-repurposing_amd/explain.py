"""explain.py: which proteins and biological functions does a treatment run through?  A diffusion profile "identifies the proteins and
biological functions" a drug or a disease acts on (multiscale/README.md, overview), and a treatment is explained by what the drug's and the
disease's profiles rank highest in common; the reference's interpret.py asks for "tracing the connections ... based on exact connections or
computed proximities" (:7-8) and ships no code.  interpret.py here answers the exact connections with shortest paths; this answers the
computed proximities.  It reads predict_drug.py's config, builds (or reuses) its profile directory with the same functions (predict.py),
selects the K highest nodes of every referenced profile per node type on the GPU (diffusion.top_nodes / csrc/profile_topk.hip, one call; no
CPU fallback) and counts what two selections share (diffusion.top_overlap, one call).

  --drug D --indication I        one row per node in the top K of either profile, per type, with its rank and value in both (and, with
                                 --edges, the weighted graph's edges among those nodes, the drug and the indication)
  --pairs pairs.tsv | --treatments   one row per drug-indication pair: per type the number of shared nodes, the Jaccard index and the nodes
"""
from __future__ import annotations

import argparse
import csv
import json
import sys

import numpy as np

from . import predict
from .diffusion import MAX_TOP
from .msi import DRUG, FUNCTIONAL_PATHWAY, INDICATION, PROTEIN
from .predict import PredictError, write_tsv

TYPES = (DRUG, INDICATION, PROTEIN, FUNCTIONAL_PATHWAY)
DEFAULT_TYPES = f"{PROTEIN},{FUNCTIONAL_PATHWAY}"
NODE_HEADER = ["node", "name", "type", "drug_rank", "drug_value", "indication_rank", "indication_value", "shared"]
EDGE_HEADER = ["source", "target", "weight"]
PAIR_HEADER = ["drug", "drug_name", "indication", "indication_name"]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: the proteins and biological functions a drug's and an indication's diffusion "
                                            "profiles rank highest, and what they share (explain.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as predict_drug.py reads it")
    p.add_argument("--drug", default=None, type=str, help="single pair: the drug id")
    p.add_argument("--indication", default=None, type=str, help="single pair: the indication id")
    p.add_argument("--pairs", default=None, type=str, help="table: a TSV with the columns drug and indication, one row out per pair")
    p.add_argument("--treatments", action="store_true", help="table: the pairs of the config's networks.drug_to_indication table that both have a profile")
    p.add_argument("--top", default=20, type=int, help=f"nodes per profile and type, 1 .. {MAX_TOP} (default: 20)")
    p.add_argument("--types", default=DEFAULT_TYPES, type=str, help="comma list of node types, one group each: " + ", ".join(TYPES) + f" (default: {DEFAULT_TYPES})")
    p.add_argument("--out", default=None, type=str, help="the table (default: explain_nodes.tsv for a single pair, overlaps.tsv for a table)")
    p.add_argument("--edges", default=None, type=str, help="single pair: also write the weighted edges among the listed nodes, the drug and the indication")
    return p.parse_args(argv)


def check_args(types, top, drug=None, indication=None, pairs=None, treatments=False, edges=None):
    """every refusal that needs neither the graph nor the GPU -> the listed types"""
    listed = [t.strip() for t in types.split(",")] if isinstance(types, str) else list(types)
    if not listed or listed == [""]:
        raise PredictError("--types lists no type; choose from " + ", ".join(TYPES))
    for t in listed:
        if t not in TYPES:
            raise PredictError(f"--types: {t!r} is unknown; choose from {', '.join(TYPES)}")
    if len(set(listed)) != len(listed):
        raise PredictError(f"--types: repeated type in {listed}")
    if not 1 <= top <= MAX_TOP:
        raise PredictError(f"--top {top} is outside 1 .. {MAX_TOP}")
    single = drug is not None or indication is not None
    table = pairs is not None or bool(treatments)
    if single == table:
        raise PredictError("give either --drug and --indication, or one of --pairs / --treatments")
    if single and (drug is None or indication is None):
        raise PredictError("a single pair needs both --drug and --indication")
    if table and pairs is not None and treatments:
        raise PredictError("give one of --pairs / --treatments, not both")
    if table and edges is not None:
        raise PredictError("--edges needs a single pair (--drug and --indication)")
    return listed


def read_pairs(path, flag="--pairs"):
    """a tab-separated table with the columns drug and indication -> [(drug, indication)] in row order"""
    with open(path, newline="") as f:
        rows = csv.reader(f, delimiter="\t")
        header = next(rows, None)
        if header is None or "drug" not in header or "indication" not in header:
            raise PredictError(f"{flag} {path!r}: the table needs the columns drug and indication")
        di, ii = header.index("drug"), header.index("indication")
        return [(r[di], r[ii]) for r in rows if len(r) > max(di, ii)]


def node_groups(nodelist, g, types):
    """-> int32 [N]: the position of a node's type in `types`, -1 for every other node"""
    at = {t: i for i, t in enumerate(types)}
    return np.asarray([at.get(g.type.get(n), -1) for n in nodelist], dtype=np.int32)


def check_profile(what, node, nodelist, profiles, g):
    if node not in g.adj:
        raise PredictError(f"{what} {node!r} is not a node of the graph")
    if node not in profiles:
        raise PredictError(f"{what} {node!r} has no diffusion profile (only drugs and indications with proteins have one)")
    if len(profiles[node]) != len(nodelist):
        raise PredictError(f"the profile of {node!r} has {len(profiles[node])} entries, node2idx.pkl {len(nodelist)}")


def refuse_nan(selected, cnt, profiles, groups, types, nodelist):
    """a selection flagged by the kernel (cnt = -1): the profile holds a NaN within a requested type -- refused by the node it sits at"""
    for s, node in enumerate(selected):
        for t, name in enumerate(types):
            if cnt[s][t] < 0:
                at = np.flatnonzero((groups == t) & np.isnan(np.asarray(profiles[node], dtype=np.float64)))
                where = nodelist[int(at[0])] if len(at) else "?"
                raise PredictError(f"the profile of {node!r} is NaN at node {where!r} (type {name}); its top nodes cannot be selected")


def node_rows(types, idx, cnt, drug_profile, indication_profile, nodelist, g):
    """single pair: idx [2][G][k], cnt [2][G] (selection 0 = the drug's, 1 = the indication's, host arrays) -> NODE_HEADER rows: per type
    as listed, the shared nodes first, then by drug rank, then by indication rank; a rank that is missing sorts last and prints empty"""
    rows = []
    for t, name in enumerate(types):
        rank = [{int(n): r + 1 for r, n in enumerate(idx[s][t][:max(int(cnt[s][t]), 0)])} for s in (0, 1)]
        nodes = sorted(set(rank[0]) | set(rank[1]),
                       key=lambda n: (not (n in rank[0] and n in rank[1]), rank[0].get(n, MAX_TOP + 1), rank[1].get(n, MAX_TOP + 1)))
        for n in nodes:
            node = nodelist[n]
            rows.append([node, g.node2name.get(node), name, rank[0].get(n, ""), float(drug_profile[n]), rank[1].get(n, ""),
                         float(indication_profile[n]), int(n in rank[0] and n in rank[1])])
    return rows


def edge_rows(g, nodes):
    """the weighted graph's edges among `nodes`, from the host CSR, in its order -> EDGE_HEADER rows"""
    adj, names, _ = g.to_csr()
    keep = np.asarray([n in nodes for n in names], dtype=bool)
    rows = []
    for u in np.flatnonzero(keep):
        lo, hi = adj.indptr[u], adj.indptr[u + 1]
        for v, w in zip(adj.indices[lo:hi], adj.data[lo:hi]):
            if keep[v]:
                rows.append([names[u], names[v], float(w)])
    return rows


def pair_header(types):
    return PAIR_HEADER + [f"{col}_{t}" for t in types for col in ("shared", "jaccard", "nodes")]


def jaccard(shared, cnt_a, cnt_b):
    union = cnt_a + cnt_b - shared
    return float("nan") if union == 0 else shared / union


def pair_rows(types, pairs, where, idx, cnt, shared, nodelist, g):
    """table: pairs [(drug, indication)], where {node: its selection}, idx [S][G][k], cnt [S][G], shared [T][G] (host arrays) -> rows of
    pair_header(types); the shared nodes of a type are listed in the order of the drug's ranks"""
    rows = []
    for p, (d, i) in enumerate(pairs):
        row = [d, g.node2name.get(d), i, g.node2name.get(i)]
        a, b = where[d], where[i]
        for t in range(len(types)):
            ca, cb, sh = int(cnt[a][t]), int(cnt[b][t]), int(shared[p][t])
            other = set(int(n) for n in idx[b][t][:cb])
            both = [nodelist[int(n)] for n in idx[a][t][:ca] if int(n) in other]
            if len(both) != sh:
                raise PredictError(f"pair {d!r}, {i!r}, type {types[t]}: the device counted {sh} shared nodes, the lists hold {len(both)}")
            row += [sh, jaccard(sh, ca, cb), ",".join(both)]
        rows.append(row)
    return rows


def treatment_pairs(cfg_path):
    cfg = predict.load_config(cfg_path)
    table = predict._get(cfg, "networks", "drug_to_indication", default=None)
    if not table:
        raise PredictError("config: missing key networks.drug_to_indication (--treatments reads the drug-indication table from it)")
    return read_pairs(table, "networks.drug_to_indication")


def run(cfg_path, drug=None, indication=None, pairs=None, treatments=False, top=20, types=DEFAULT_TYPES, out=None, edges=None, device="cuda",
        err=None):
    """the command -> (rows written, the table's path)"""
    from .diffusion import top_nodes, top_overlap
    err = sys.stderr if err is None else err
    types = check_args(types, top, drug, indication, pairs, treatments, edges)
    s = predict.Settings(predict.load_config(cfg_path))
    if not s.diffusion_dir:
        raise PredictError("config: diffusion.diffusion_embs_dir is missing")
    single = drug is not None
    if single:
        listed = [(drug, indication)]
    else:
        listed = read_pairs(pairs) if pairs is not None else treatment_pairs(cfg_path)
    g = predict.build_graph(s)
    nodelist, profiles = predict.diffusion_profiles(s, g)
    if treatments:
        every = len(listed)
        listed = [(d, i) for d, i in dict.fromkeys(listed) if d in profiles and i in profiles and g.type.get(d) == DRUG and g.type.get(i) == INDICATION]
        if every != len(listed):
            print(f"explain: skipped {every - len(listed)} pairs of the table: repeated, or without a profile on either side", file=err)
    for d, i in listed:
        check_profile("--drug" if single else "drug", d, nodelist, profiles, g)
        check_profile("--indication" if single else "indication", i, nodelist, profiles, g)
    if not listed:
        raise PredictError("nothing to explain: no pair is listed")
    groups = node_groups(nodelist, g, types)
    selected = list(dict.fromkeys(n for pair in listed for n in pair))
    where = {n: k for k, n in enumerate(selected)}
    try:
        idx, _, cnt = top_nodes(profiles, selected, top, groups, len(types), device)          # every referenced profile: one call
        a, b = [where[d] for d, _ in listed], [where[i] for _, i in listed]
        shared = top_overlap(idx, cnt, a, b).cpu().numpy()                                    # every pair: one call
    except ValueError as e:
        raise PredictError(str(e)) from None
    idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
    refuse_nan(selected, cnt, profiles, groups, types, nodelist)
    if single:
        out = out or "explain_nodes.tsv"
        sel = np.stack([idx[where[drug]], idx[where[indication]]]), np.stack([cnt[where[drug]], cnt[where[indication]]])
        rows = node_rows(types, sel[0], sel[1], profiles[drug], profiles[indication], nodelist, g)
        for t in range(len(types)):
            if sum(r[7] for r in rows if r[2] == types[t]) != int(shared[0][t]):
                raise PredictError(f"type {types[t]}: the device counted {int(shared[0][t])} shared nodes, the table holds another number")
        write_tsv(out, NODE_HEADER, rows)
        if edges:
            write_tsv(edges, EDGE_HEADER, edge_rows(g, {r[0] for r in rows} | {drug, indication}))
    else:
        out = out or "overlaps.tsv"
        rows = pair_rows(types, listed, where, idx, cnt, shared, nodelist, g)
        write_tsv(out, pair_header(types), rows)
    return rows, out


def main(argv=None):
    a = parse_args(argv)
    try:
        check_args(a.types, a.top, a.drug, a.indication, a.pairs, a.treatments, a.edges)
        rows, out = run(a.config, a.drug, a.indication, a.pairs, a.treatments, a.top, a.types, a.out, a.edges)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"explain: {e}", file=sys.stderr)
        sys.exit(2)
    what = f"{a.drug} x {a.indication}: {len(rows)} nodes" if a.drug is not None else f"{len(rows)} pairs"
    print(f"top {a.top}: {what}: {out}" + (f", {a.edges}" if a.edges else ""))
