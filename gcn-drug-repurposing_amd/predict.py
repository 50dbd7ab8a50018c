"""The ranked drug-candidate table of predict_drug.py (predict_drug.main + output_drugs), and run_covid.py:294-328's protein table.

predict_drug.py ties the pieces together: the weighted MSI (msi.py), a ranking of the drugs by node2vec, GCN or diffusion scores, and
per table row the query's protein neighbours the drug touches and a shortest path drug -> query.  The reference's script does not run
(a missing package, numpy 2's removed np.float, a crash on the diffusion branch's return); this is what it evidently does.

Scores and their order stay host numpy (fp64 np.matmul, np.argsort(...)[::-1]): at 1,661 drugs x 128 a device port would gain nothing
and would have to reproduce numpy's tie order.  The paths come from one device pass of shortest-path trees toward every query
(paths.py / csrc/paths.hip) instead of one networkx search per row.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import pickle
import sys
import warnings

import numpy as np

from .msi import COMPONENTS, COVID_WEIGHTS, DRUG, FUNCTIONAL_PATHWAY, PROTEIN, MsiGraph

METHODS = ("node2vec", "gcn", "diffusion")
DRUG_HEADER = ["drug name", "proximity", "conected gordon proteins", "shortest path to Covid", "path length"]   # the typo is the reference's
PROTEIN_HEADER = ["protein name", "proximity to Covid-19", "shortest path to Covid-19", "path length"]
DIFFUSION = dict(alpha=0.8595436247434408, max_iter=1000, tol=1e-06, weights=COVID_WEIGHTS)   # predict_drug.py:80-96
NODE2VEC = dict(dim=128, p=0.25, q=0.25, window=10)                                          # predict_drug.py:37-41


class PredictError(ValueError):
    pass


# ---- configuration -------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: rank drug candidates for a disease node (predict_drug.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json)")
    p.add_argument("-s", "--save-dir", default=None, type=str, help="accepted and ignored")
    p.add_argument("-r", "--resume", default=None, type=str, help="accepted and ignored")
    p.add_argument("-d", "--device", default=None, type=str, help="accepted and ignored")
    p.add_argument("--query", action="append", default=None,
                   help="node to rank for (repeatable; default NodeCovid); with several, outputs are named <stem>.<query>.tsv")
    p.add_argument("--protein-table", default=None, type=str,
                   help="also write run_covid.py's table: every named protein, its proximity to the query, its path and its length "
                        "(unaffected by the config's diffusion.compare: proteins have no profile of their own, so their proximity stays the "
                        "query's visit probability)")
    p.add_argument("--seed", default=0, type=int, help="seed of the node2vec walks / skip-gram when the embedding file is generated")
    return p.parse_args(argv)


def _get(cfg, *keys, default=KeyError):
    d = cfg
    for k in keys:
        if not isinstance(d, dict) or k not in d:
            if default is KeyError:
                raise PredictError(f"config: missing key {'.'.join(keys)}")
            return default
        d = d[k]
    return d


def compare_setting(cfg, method):
    """diffusion.compare: 'visit' (the default: the query's visit probability at the drug's node, the reference's score) or one of
    diffusion.ALL_METRICS (the score is minus that distance between the query's profile and the drug's own)"""
    from .diffusion import ALL_METRICS as METRICS
    compare = _get(cfg, "diffusion", "compare", default="visit")
    if compare == "visit":
        return compare
    if compare not in METRICS:
        raise PredictError(f"config: diffusion.compare = {compare!r} is unknown; choose 'visit' or one of {', '.join(METRICS)}")
    if method != "diffusion":
        raise PredictError(f"config: diffusion.compare = {compare!r} compares diffusion profiles and needs method = 'diffusion', "
                           f"not {method!r}")
    return compare


class Settings:
    """the config keys predict_drug.main reads, resolved and checked before anything touches the GPU"""

    def __init__(self, cfg, queries=None):
        self.method = _get(cfg, "method")
        if self.method not in METHODS:
            raise PredictError(f"config: method {self.method!r} is unknown; choose one of {', '.join(METHODS)}")
        self.compare = compare_setting(cfg, self.method)
        if self.method == "gcn" and _get(cfg, "gcn", "embs") != "node2vec":
            raise PredictError(f"config: gcn.embs = {_get(cfg, 'gcn', 'embs')!r} is not supported; only 'node2vec' (the reference's one branch)")
        self.topk = int(_get(cfg, "topk"))
        self.drug_out = _get(cfg, "output", "drug_candidates")
        self.graph_out = _get(cfg, "output", "graph")
        self.covid_table = _get(cfg, "covid", "save_dir")
        if _get(cfg, "covid", "add_permutation", default=False):
            raise PredictError("config: covid.add_permutation = true needs the UniProt web service (utils.py:10-33), which this tool "
                               "never calls; set it to false")
        if not os.path.exists(self.covid_table):
            raise PredictError(f"config: covid.save_dir {self.covid_table!r} does not exist; building it needs the UniProt web service "
                               "(utils.py:10-33), which this tool never calls")
        self.add_pathway = bool(_get(cfg, "covid", "add_pathway", default=False))
        self.pathway_file = _get(cfg, "covid", "pertub_pathway_file") if self.add_pathway else None
        self.ppi = _get(cfg, "networks", "protein_to_protein")
        self.data_dir = os.path.dirname(self.ppi)
        self.diffusion_dir = _get(cfg, "diffusion", "diffusion_embs_dir", default=None)
        prefix = _get(cfg, "node2vec", "emb_file_prefix")
        self.walk_length = int(_get(cfg, "node2vec", "walk_length"))
        self.number_walk = int(_get(cfg, "node2vec", "number_walk"))
        self.n2v_file = f"{prefix}_num_{self.number_walk}_len_{self.walk_length}.embs.txt"   # predict_drug.py:28-31
        self.gcn_file = _get(cfg, "gcn", "emb_file", default=None)
        if self.method == "gcn" and not os.path.exists(self.gcn_file):
            raise PredictError(f"gcn.emb_file {self.gcn_file!r} does not exist; make it with `python train.py --emb-file {self.n2v_file} "
                               f"--adj-file {self.graph_out}` (it writes graph_embs.txt) and move that file to {self.gcn_file!r}")
        if self.method == "diffusion" and not self.diffusion_dir:
            raise PredictError("config: diffusion.diffusion_embs_dir is missing")
        self.queries = list(queries) if queries else ["NodeCovid"]
        if len(set(self.queries)) != len(self.queries):
            raise PredictError(f"--query: repeated query in {self.queries}")
        files = self.tables()
        for name, path in files.items():
            if not os.path.exists(path):
                raise PredictError(f"MSI table {name}: {path!r} does not exist")

    def tables(self):
        """MSI(indication2protein_file_path=covid.save_dir) with the other tables in the directory of networks.protein_to_protein
        (predict_drug.py:168-170: the reference's defaults are data/<table>.tsv)"""
        files = {name: os.path.join(self.data_dir, name + ".tsv") for name, _, _ in COMPONENTS}
        files["indication_to_protein"] = self.covid_table
        return files


def load_config(path):
    with open(path) as f:
        return json.load(f)


def output_name(path, query, many):
    if not many:
        return path
    stem, ext = os.path.splitext(path)
    return f"{stem}.{query}{ext or '.tsv'}"


# ---- the graph -----------------------------------------------------------------------------------------------------------------------

def read_pathway_ids(path):
    """the Pathway_ID column of covid.pertub_pathway_file"""
    with open(path, newline="") as f:
        rows = csv.reader(f, delimiter="\t")
        header = next(rows)
        i = header.index("Pathway_ID")
        return [r[i] for r in rows if len(r) > i]


def build_graph(s):
    """predict_drug.py:168-196: the MSI with the covid table as its indication table, weighted, plus the pathway edges"""
    g = MsiGraph().load(s.tables())
    g.weight_graph(COVID_WEIGHTS)
    if s.add_pathway:
        g.add_covid_pathway_edges(read_pathway_ids(s.pathway_file))
    return g


def check_queries(s, g):
    for q in s.queries:
        if q not in g.adj:
            raise PredictError(f"--query {q!r} is not a node of the graph")
        if s.method == "diffusion" and q not in g.drugs_in_graph + g.indications_in_graph:
            raise PredictError(f"--query {q!r} has no diffusion profile (only drugs and indications with proteins have one)")


def display(g, node):
    """node2name, or the node id where the name is missing (predict_drug.py:70-71)"""
    name = g.node2name.get(node)
    return node if name is None else name


# ---- rankings ------------------------------------------------------------------------------------------------------------------------

def node2vec_file(s, g, seed):
    """the node2vec embedding file of the config, generated with the reference's arguments when absent (predict_drug.py:31-45)"""
    if not os.path.exists(s.n2v_file):
        from .node2vec import Node2vec
        model = Node2vec(g, path_length=s.walk_length, num_paths=s.number_walk, seed=seed, **NODE2VEC)
        print("Saving embeddings...")
        model.save_embeddings(s.n2v_file)
    return s.n2v_file


def embedding_scores(s, g, seed):
    """-> (node names in embedding-file order, embeddings [N, d]): raw node2vec (predict_drug.py:55) or row-normalised GCN (:52-53)"""
    from .embio import read_embs
    names, x = read_embs(node2vec_file(s, g, seed))
    if s.method == "gcn":
        x = normalize_like_sklearn(np.loadtxt(s.gcn_file, ndmin=2))
        if x.shape[0] != len(names):
            raise PredictError(f"{s.gcn_file}: {x.shape[0]} rows, but the node2vec file has {len(names)} nodes")
    unknown = [n for n in names if n not in g.adj]
    if unknown:
        raise PredictError(f"{s.n2v_file}: node {unknown[0]!r} is not in the graph")
    return names, x


def normalize_like_sklearn(e):
    """consumer.normalize_rows' row L2 normalisation with sklearn.preprocessing.normalize's arithmetic (einsum norms), so the scores
    equal the reference's to the last bit"""
    e = np.asarray(e, dtype=np.float64)
    n = np.sqrt(np.einsum("ij,ij->i", e, e))
    n[n == 0] = 1.0
    return e / n[:, None]


def rank_embeddings(names, x, g, query):
    """predict_drug.py:57-71: drugs in file order, fp64 matmul with the query's row, argsort descending"""
    drugs = [n for n in names if g.type[n] == DRUG]
    idx = {n: i for i, n in enumerate(names)}
    if query not in idx:
        raise PredictError(f"--query {query!r} has no row in the embedding file")
    prox = np.matmul(x[[idx[d] for d in drugs]], np.array(x[idx[query]]))
    order = np.argsort(np.array(prox))[::-1]
    return [drugs[i] for i in order], prox[order]


class _NoGlobals(pickle.Unpickler):
    def find_class(self, module, name):
        raise pickle.UnpicklingError(f"node2idx.pkl names {module}.{name}; only a dict of node -> index is expected")


def diffusion_profiles(s, g):
    """profiles of every drug and indication into diffusion_embs_dir (reused when the directory exists) -> (node order, {node: profile})"""
    from .diffusion import DiffusionProfiles
    if not os.path.exists(s.diffusion_dir):
        print("Calculate diffusion profiles")
        DiffusionProfiles(num_cores=None, save_load_file_path=s.diffusion_dir, **DIFFUSION).calculate_diffusion_profiles(g)
    with open(os.path.join(s.diffusion_dir, "node2idx.pkl"), "rb") as f:
        node2idx = _NoGlobals(f).load()
    nodelist = [None] * len(node2idx)
    for node, i in node2idx.items():
        nodelist[i] = node
    dp = DiffusionProfiles(alpha=None, max_iter=None, tol=None, weights=None, num_cores=None, save_load_file_path=s.diffusion_dir)
    dp.load_diffusion_profiles(g.drugs_in_graph + g.indications_in_graph)
    return nodelist, dp.drug_or_indication2diffusion_profile


def rank_diffusion(nodelist, profiles, g, query):
    """predict_drug.py:99-125 with the evident intent of its return line: the probabilities as an array"""
    if query not in profiles:
        raise PredictError(f"--query {query!r} has no diffusion profile in the profile directory")
    res = profiles[query]
    if len(res) != len(nodelist):
        raise PredictError(f"the profile of {query!r} has {len(res)} entries, node2idx.pkl {len(nodelist)}")
    drugs = [n for n in nodelist if g.type.get(n) == DRUG]
    pos = {n: i for i, n in enumerate(nodelist)}
    prox = np.asarray([res[pos[d]] for d in drugs])
    order = np.argsort(np.array(prox))[::-1]
    return [drugs[i] for i in order], prox[order]


def profile_distances(profiles, rows, cols, metric):
    """the distance of every (row node, column node) pair of diffusion profiles, on the device (diffusion.compare_profiles) -> device
    tensor fp64 [len(rows)][len(cols)].  A node whose distances are NaN (a zero profile, or a constant one under 'correlation') is refused
    by its id: it cannot be ranked"""
    import torch

    from .diffusion import compare_profiles
    for what, nodes in (("query", rows), ("drug", cols)):
        for n in nodes:
            if n not in profiles:
                raise PredictError(f"{what} {n!r} has no diffusion profile in the profile directory; diffusion.compare needs one")
    try:
        d = compare_profiles(profiles, rows, cols, metric)
    except ValueError as e:
        raise PredictError(str(e)) from None
    bad = torch.isnan(d)
    if bool(bad.any()):
        bad = bad.cpu().numpy()
        whole = np.flatnonzero(bad.all(axis=1))
        node = rows[whole[0]] if len(whole) else cols[np.flatnonzero(bad.any(axis=0))[0]]
        raise PredictError(f"the {metric} distance of node {node!r} is NaN (its diffusion profile is zero or constant); it cannot be ranked")
    return d


def rank_compare(nodelist, profiles, g, queries, metric):
    """diffusion.compare = a metric: the score of drug d for query q is -dist(profile_q, profile_d); drugs in nodelist order, nearest first,
    ties by that order -> {query: (drugs ranked, scores ranked)}"""
    drugs = [n for n in nodelist if g.type.get(n) == DRUG]
    dist = profile_distances(profiles, list(queries), drugs, metric).cpu().numpy()
    out = {}
    for q, row in zip(queries, dist):
        order = np.argsort(row, kind="stable")
        out[q] = ([drugs[i] for i in order], -row[order])
    return out


def rank_profiles(s, nodelist, profiles, g):
    """-> {query: (drugs ranked, scores ranked)} by the config's diffusion.compare"""
    if s.compare == "visit":
        return {q: rank_diffusion(nodelist, profiles, g, q) for q in s.queries}
    return rank_compare(nodelist, profiles, g, s.queries, s.compare)


# ---- the tables ----------------------------------------------------------------------------------------------------------------------

def fmt_float(v):
    """an fp64 as pandas' to_csv writes it (repr)"""
    return repr(float(v))


def write_tsv(path, header, rows):
    """DataFrame.to_csv(path, sep='\\t', na_rep='NA', index=False) for columns of str / int / float values (None -> NA)"""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", lineterminator="\n")
        w.writerow(header)
        for r in rows:
            w.writerow(["NA" if v is None else fmt_float(v) if isinstance(v, (float, np.floating)) else v for v in r])


class PathSource:
    """shortest paths toward the queries: node index lists from (dist, next) of one device pass (or any source of the same arrays)"""

    def __init__(self, names, dist, nxt, targets):
        self.names, self.dist, self.next, self.targets = names, dist, nxt, targets
        self.index = {n: i for i, n in enumerate(names)}

    def path(self, q, node):
        from .paths import follow
        p = follow(self.dist, self.next, self.targets, q, self.index[node])
        return None if p is None else [self.names[i] for i in p]


def path_columns(g, paths, q, node):
    p = paths.path(q, node)
    if p is None:
        return None, None      # the reference's networkx call raises NetworkXNoPath here
    return ", ".join(display(g, x) for x in p), len(p) - 1


def drug_rows(g, query, drugs_ranked, prox_ranked, topk, paths, q):
    """predict_drug.output_drugs (:251-283)"""
    gordon = [n for n in g.adj[query] if g.type[n] == PROTEIN]
    rows = []
    for drug, prox in zip(drugs_ranked[:topk], prox_ranked[:topk]):
        conn = [display(g, p) for p in gordon if p in g.adj[drug]]
        text, length = path_columns(g, paths, q, drug)
        rows.append([display(g, drug), float(prox), ", ".join(conn) if conn else "NA", text, length])
    return rows


def named_proteins(g, names):
    """run_covid.py:300-302: the mask of the proteins that have a name, in `names` order"""
    return np.array([g.type.get(n) == PROTEIN and g.node2name.get(n) is not None for n in names], bool)


def protein_rows(g, names, scores, paths, q):
    """run_covid.py:294-328: every protein with a name, in `names` order, its score (scores[i] for the i-th such protein), path and
    length"""
    rows = []
    for node, s in zip(np.asarray(names, dtype=object)[named_proteins(g, names)], scores):
        text, length = path_columns(g, paths, q, node)
        rows.append([g.node2name[node], float(s), text, length])
    return rows


def device_paths(g, queries):
    """one batched device pass of shortest-path trees toward every query"""
    from .paths import ShortestPathTrees
    adj, names, _ = g.to_csr()
    idx = {n: i for i, n in enumerate(names)}
    targets = [idx[q] for q in queries]
    trees = ShortestPathTrees(adj)
    dist, nxt = trees.to(targets)
    trees.close()
    return PathSource(names, dist, nxt, np.asarray(targets))


def run(s, protein_table=None, seed=0, path_source=device_paths, timings=None):
    """predict_drug.main on Settings s -> {query: (drug table path, protein table path or None)}"""
    import time
    t = {} if timings is None else timings
    t0 = time.perf_counter()
    g = build_graph(s)
    check_queries(s, g)
    if not os.path.exists(s.graph_out):
        g.write_weighted_edgelist(s.graph_out)
    else:
        warnings.warn(f"graph struc file {s.graph_out} already exists. change this line if want to overwrite.")
    t1 = time.perf_counter()
    t["graph_s"] = t1 - t0
    if s.method == "diffusion":
        nodelist, profiles = diffusion_profiles(s, g)
        ranked = rank_profiles(s, nodelist, profiles, g)
        prot_names = nodelist
        prot_scores = {q: np.asarray(profiles[q])[named_proteins(g, nodelist)] for q in s.queries} if protein_table else None
    else:
        names, x = embedding_scores(s, g, seed)
        ranked = {q: rank_embeddings(names, x, g, q) for q in s.queries}
        prot_names = names
        if protein_table:   # run_covid.py:303-305: the named proteins' rows times the query's
            mask = named_proteins(g, names)
            prot_scores = {q: np.matmul(x[mask], np.array(x[names.index(q)])) for q in s.queries}
    t2 = time.perf_counter()
    t["rank_s"] = t2 - t1
    paths = path_source(g, s.queries)
    t3 = time.perf_counter()
    t["paths_s"] = t3 - t2
    many = len(s.queries) > 1
    out = {}
    for q_i, query in enumerate(s.queries):
        drugs, prox = ranked[query]
        dpath = output_name(s.drug_out, query, many)
        write_tsv(dpath, DRUG_HEADER, drug_rows(g, query, drugs, prox, s.topk, paths, q_i))
        ppath = None
        if protein_table:
            ppath = output_name(protein_table, query, many)
            write_tsv(ppath, PROTEIN_HEADER, protein_rows(g, prot_names, prot_scores[query], paths, q_i))
        out[query] = (dpath, ppath)
    t["tables_s"] = time.perf_counter() - t3
    return out


def main(argv=None):
    args = parse_args(argv)
    try:
        s = Settings(load_config(args.config), args.query)
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"predict_drug: {e}", file=sys.stderr)
        sys.exit(2)
    try:
        out = run(s, args.protein_table, args.seed)
    except PredictError as e:
        print(f"predict_drug: {e}", file=sys.stderr)
        sys.exit(2)
    for q, (d, p) in out.items():
        print(f"{q}: {d}" + (f", {p}" if p else ""))
