"""evaluate_auc.py (evaluate_auc.py:114-171): the median and mean ROC-AUC, over every indication, of ranking all drugs for it by a method's
scores -- diffusion profiles, raw node2vec inner products or row-normalised GCN inner products -- against the drugs listed for it in
networks.drug_to_indication.

The reference's embedding branches end in a NameError (dp_saved is only set for diffusion); the evident intent, embedding inner products
as scores (consumer.py), is what this does.  It crashes on an indication without a row in the label table, on a listed drug that is not in
the graph and on a single-class label vector; here such indications are skipped and counted on stderr, listed drugs that are not drug
nodes are left out (consumer.indication_aucs' rules).  Scores of the CLI stay host fp64 (np.matmul per indication, predict.py's arithmetic; a
gather from the profiles for diffusion); the ranking statistic of every indication runs in one device launch (csrc/auc.hip).  DESIGN.md
section 9.4 has the contract decisions and the measurements.

--metrics adds average precision and recall@K beside the AUC (csrc/rank_metrics.hip: all three in one launch in place of auc.hip's;
DESIGN.md section 9.8).  Without it nothing here launches or prints anything it did not before.

--bootstrap B adds, behind those lines, one line per reported metric with the percentile intervals of its median and mean over B bootstrap
resamples of the indications (csrc/resample.hip through resample.bootstrap_summary).  The same holds without it.

--by-class TABLE adds the AUC and the --metrics per ATC drug class: one stratum per (indication, class) pair with a listed drug in common,
the class's listed drugs ranked against all the indication's unlisted drugs, every stratum in one launch (csrc/rank_strata.hip through
device_metrics_strata), a table per class, optionally one per pair, and one more line.  The same holds without it.
"""
from __future__ import annotations

import argparse
import contextlib
import csv
import json
import os
import re
import sys
import time
import types
import warnings

import numpy as np

from .consumer import read_drug_indication_tsv
from .msi import COMPONENTS, DRUG, INDICATION, MsiGraph
from .predict import PredictError, _get, compare_setting, diffusion_profiles, display, embedding_scores, load_config, profile_distances

METHODS = ("diffusion", "node2vec", "gcn")
PER_INDICATION_HEADER = ["indication", "name", "positives", "negatives", "auc"]
MAX_COLS = 16384          # drugs per row: csrc/auc.hip sorts a row's keys in one workgroup's LDS
MAX_CUTS = 8              # distinct K of recall@K in one launch (csrc/rank_metrics.hip)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: median / mean ROC-AUC over indications (evaluate_auc.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json)")
    p.add_argument("-s", "--save-dir", default=None, type=str, help="accepted and ignored")
    p.add_argument("-r", "--resume", default=None, type=str, help="accepted and ignored")
    p.add_argument("-d", "--device", default=None, type=str, help="accepted and ignored")
    p.add_argument("--seed", default=0, type=int, help="seed of the node2vec walks / skip-gram when the eval embedding file is generated")
    p.add_argument("--per-indication", default=None, type=str,
                   help="also write a TSV with one row per evaluated indication: id, name, positives, negatives, AUC")
    p.add_argument("--metrics", default=None, type=str,
                   help="comma-separated ranking statistics to report after the AUC line, one line each: ap (average precision), "
                        f"recall@K (K >= 1, at most {MAX_CUTS} distinct K), auc; --per-indication gains one column per metric")
    p.add_argument("--bootstrap", default=None, type=int,
                   help="also print, per reported metric, the percentile intervals of the median and the mean over this many bootstrap "
                        "resamples of the indications (seeded by --seed)")
    p.add_argument("--level", default=0.95, type=float, help="coverage of the --bootstrap intervals (default: 0.95)")
    p.add_argument("--by-class", default=None, type=str,
                   help="the drug-class table (data/drug_classification_df.tsv): also report the AUC and the --metrics per ATC class, over "
                        "the (indication, class) pairs with a listed drug in common, each ranked against all the indication's unlisted drugs")
    p.add_argument("--class-levels", default=None, type=str, help="ATC levels of --by-class, comma-separated (default: 1,2,3,4)")
    p.add_argument("--min-indications", default=1, type=int, help="drop classes with fewer (indication, class) pairs from --per-class (default: 1)")
    p.add_argument("--per-class", default=None, type=str, help="the table of --by-class, one row per class (default: class_metrics.tsv)")
    p.add_argument("--per-stratum", default=None, type=str, help="with --by-class, also write one row per (indication, class) pair")
    return p.parse_args(argv)


class Settings:
    """the config keys evaluate_auc.main reads, resolved and checked before anything touches the GPU.  The attribute names are those
    predict.node2vec_file / embedding_scores / diffusion_profiles read."""

    def __init__(self, cfg):
        self.method = _get(cfg, "method")
        if self.method not in METHODS:
            raise PredictError(f"config: method {self.method!r} is unknown; choose one of {', '.join(METHODS)}")
        self.compare = compare_setting(cfg, self.method)
        if self.method == "gcn" and _get(cfg, "gcn", "embs") != "node2vec":
            raise PredictError(f"config: gcn.embs = {_get(cfg, 'gcn', 'embs')!r} is not supported; only 'node2vec' (the reference's one branch)")
        self.graph_out = _get(cfg, "eval", "graph")
        self.ppi = _get(cfg, "networks", "protein_to_protein")
        self.data_dir = os.path.dirname(self.ppi)
        self.labels = _get(cfg, "networks", "drug_to_indication")
        if not os.path.exists(self.labels):
            raise PredictError(f"networks.drug_to_indication {self.labels!r} does not exist")
        self.diffusion_dir = _get(cfg, "diffusion", "eval_diffusion_embs_dir") if self.method == "diffusion" else None
        self.n2v_file = self.walk_length = self.number_walk = self.gcn_file = None
        if self.method != "diffusion":
            prefix = _get(cfg, "node2vec", "eval_emb_file_prefix")
            self.walk_length = int(_get(cfg, "node2vec", "walk_length"))
            self.number_walk = int(_get(cfg, "node2vec", "number_walk"))
            self.n2v_file = f"{prefix}_num_{self.number_walk}_len_{self.walk_length}.embs.txt"   # evaluate_auc.py:29-32
        if self.method == "gcn":
            self.gcn_file = _get(cfg, "gcn", "emb_file")
            if not os.path.exists(self.gcn_file):
                raise PredictError(f"gcn.emb_file {self.gcn_file!r} does not exist; make it with `python train.py --emb-file {self.n2v_file} "
                                   f"--adj-file {self.graph_out}` (it writes graph_embs.txt) and move that file to {self.gcn_file!r}")
        for name, path in self.tables().items():
            if not os.path.exists(path):
                raise PredictError(f"MSI table {name}: {path!r} does not exist")

    def tables(self):
        """MSI() with its default tables, data/<table>.tsv, the directory taken from networks.protein_to_protein (the plain
        indication_to_protein.tsv, not the covid table)"""
        return {name: os.path.join(self.data_dir, name + ".tsv") for name, _, _ in COMPONENTS}


def format_line(aucs):
    """evaluate_auc.py:170's f-string on fp64 values"""
    a = np.asarray(aucs, dtype=np.float64)
    return f"median auc: {np.median(a)}, mean auc: {a.mean()}"


# ---- metric names ------------------------------------------------------------------------------------------------------------------------

_RECALL = re.compile(r"^recall@([0-9]+)$")


def parse_metric(name):
    """'auc' | 'ap' | 'recall@K' (K >= 1) -> (kind, K or None); anything else is refused by name"""
    name = str(name)
    if name in ("auc", "ap"):
        return name, None
    m = _RECALL.match(name)
    if m and int(m.group(1)) >= 1:
        return "recall", int(m.group(1))
    raise PredictError(f"metric {name!r} is unknown; choose auc, ap or recall@K with an integer K >= 1")


def parse_metrics(spec):
    """a comma-separated string, or a sequence of names -> the list of names, in the order given: every name known, none given twice, at
    most MAX_CUTS distinct K"""
    names = [n.strip() for n in spec.split(",")] if isinstance(spec, str) else [str(n) for n in spec]
    if isinstance(spec, str) and names == [""]:
        raise PredictError("--metrics is empty; name auc, ap or recall@K")
    seen = []
    for n in names:
        kind, k = parse_metric(n)
        canon = n if kind != "recall" else f"recall@{k}"
        if canon in seen:
            raise PredictError(f"metric {canon!r} is given twice")
        seen.append(canon)
    if len(metric_cuts(seen)) > MAX_CUTS:
        raise PredictError(f"{len(metric_cuts(seen))} distinct K of recall@K are above the limit of {MAX_CUTS} in one evaluation")
    return seen


def metric_cuts(metrics):
    """the distinct K of the recall@K among metrics, in the order of first appearance"""
    ks = []
    for n in metrics:
        kind, k = parse_metric(n)
        if kind == "recall" and k not in ks:
            ks.append(k)
    return tuple(ks)


def metric_arrays(metrics, ks, auc, ap, hits, n_pos):
    """{name: fp64 [R]} in the order of metrics; recall@K = hits / P (the one division the kernel leaves to the caller), NaN where the
    kernel wrote NaN"""
    out = {}
    hits = np.asarray(hits, np.float64).reshape(len(auc), len(ks))
    for n in metrics:
        kind, k = parse_metric(n)
        if kind == "auc":
            out[n] = np.asarray(auc, np.float64)
        elif kind == "ap":
            out[n] = np.asarray(ap, np.float64)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                out[n] = hits[:, ks.index(k)] / np.asarray(n_pos, np.float64)
    return out


def format_metric_line(name, values):
    """the AUC line's f-string with the metric's name"""
    a = np.asarray(values, dtype=np.float64)
    return f"median {name}: {np.median(a)}, mean {name}: {a.mean()}"


def format_bootstrap_line(name, s, B, seed):
    """one line of --bootstrap from resample.bootstrap_summary's record of the metric"""
    return (f"bootstrap {name}: median [{s['median']['lo']}, {s['median']['hi']}], mean [{s['mean']['lo']}, {s['mean']['hi']}] "
            f"({B} resamples, seed {seed})")


def bootstrap_lines(res, B, level, seed, summary=None):
    """the lines of --bootstrap for Result res: the AUC and then every requested metric, over the AUC line's indications, all resampled
    together (csrc/resample.hip through resample.bootstrap_summary, or `summary` in its place)"""
    if summary is None:
        from .resample import bootstrap_summary as summary
    series = {"auc": res.auc[res.kept]}
    series.update({name: v[res.kept] for name, v in res.metrics.items()})
    return [format_bootstrap_line(name, s, B, seed) for name, s in summary(series, B, seed, level).items()]


def _device_inputs(who, scores, pos_ptr, pos_col):
    """the shape checks device_aucs and device_metrics share, on the host -> (scores, ptr, col)"""
    import torch
    if isinstance(scores, torch.Tensor):
        if scores.dim() != 2 or scores.dtype != torch.float64 or not scores.is_cuda:
            raise PredictError(f"{who}: device scores must be an fp64 matrix [R, C] on the GPU")
        s = scores.contiguous()
    else:
        s = np.ascontiguousarray(scores, dtype=np.float64)
    ptr = np.ascontiguousarray(pos_ptr, dtype=np.int32)
    col = np.ascontiguousarray(pos_col, dtype=np.int32)
    if len(s.shape) != 2 or s.shape[1] < 1 or ptr.shape != (s.shape[0] + 1,) or ptr[0] != 0 or np.any(np.diff(ptr) < 0) or ptr[-1] != len(col):
        raise PredictError(f"{who}: scores {s.shape} and the positives' row pointer ({len(ptr)} entries over {len(col)}) disagree")
    if s.shape[1] > MAX_COLS:
        raise PredictError(f"{s.shape[1]} drugs per indication is above the limit of {MAX_COLS} (one workgroup sorts a row in LDS)")
    return s, ptr, col


def check_cuts(who, ks):
    """-> the cut-offs as a host int32 array; at most MAX_CUTS, every one >= 1"""
    ks = [int(k) for k in ks]
    if len(ks) > MAX_CUTS:
        raise PredictError(f"{who}: {len(ks)} cut-offs are above the limit of {MAX_CUTS}")
    if any(k < 1 for k in ks):
        raise PredictError(f"{who}: cut-off {min(ks)} is below 1")
    return np.asarray(ks, dtype=np.int32)


def _row_buffers(dev, scores, ptr, col, nk=None):
    """what one launch of _launch_rows reads and writes, on device dev, under DeviceEvaluator's attribute names: the scores (a device
    tensor stays where it is), the positives' CSR and gss_auc_rows' outputs; with nk, room for nk cut-offs, also those of
    gss_rank_metrics_rows and its workspace, the sorted positives' parking space of csrc/rank_metrics.hip"""
    import torch
    R, C = scores.shape
    b = types.SimpleNamespace()
    b.d_scores = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(scores).to(dev)
    b.d_ptr = torch.from_numpy(ptr).to(dev)
    b.d_col = torch.from_numpy(col if len(col) else np.zeros(1, np.int32)).to(dev)   # no positive anywhere: a word nothing reads, not a null pointer
    b.d_auc = torch.empty(R, dtype=torch.float64, device=dev)
    b.d_pos = torch.empty(R, dtype=torch.int32, device=dev)
    b.d_neg = torch.empty(R, dtype=torch.int32, device=dev)
    if nk is not None:
        b.d_ap = torch.empty(R, dtype=torch.float64, device=dev)
        b.d_hits = torch.empty(R * max(nk, 1), dtype=torch.float64, device=dev)
        b.d_work = torch.empty(R * C, dtype=torch.int64, device=dev)
    return b


def _launch_rows(b, h_ks=None):
    """gss_auc_rows on the buffers b (_row_buffers, or a DeviceEvaluator), or with the cut-offs h_ks (check_cuts) gss_rank_metrics_rows.
    Both synchronise the stream; no CPU fallback"""
    from . import _lib
    lib = _lib.load()
    R, C = b.d_scores.shape
    rows = (R, C, _lib.ptr(b.d_scores), C, _lib.ptr(b.d_ptr), _lib.ptr(b.d_col))
    counts = (_lib.ptr(b.d_pos), _lib.ptr(b.d_neg))
    if h_ks is None:
        _lib.check(lib.gss_auc_rows(*rows, _lib.ptr(b.d_auc), *counts, _lib.current_stream()), "gss_auc_rows")
    else:
        _lib.check(lib.gss_rank_metrics_rows(*rows, len(h_ks), h_ks.ctypes.data if len(h_ks) else None, _lib.ptr(b.d_auc), _lib.ptr(b.d_ap),
                                             _lib.ptr(b.d_hits), *counts, _lib.ptr(b.d_work), b.d_work.numel() * 8, _lib.current_stream()),
                   "gss_rank_metrics_rows")


def _device_rows(who, scores, pos_ptr, pos_col, ks, timings):
    """device_metrics, and with ks = None device_aucs: the checks on the host, the upload, the one launch -> host (auc, ap, hits, n_pos,
    n_neg), ap and hits None without ks"""
    import torch

    from . import _lib
    s, ptr, col = _device_inputs(who, scores, pos_ptr, pos_col)
    h_ks = None if ks is None else check_cuts(who, ks)
    R, nk = s.shape[0], 0 if ks is None else len(h_ks)
    if R == 0:
        return np.zeros(0), np.zeros(0), np.zeros((0, nk)), np.zeros(0, np.int32), np.zeros(0, np.int32)
    t = {} if timings is None else timings
    _lib.load()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = _row_buffers(torch.device("cuda"), s, ptr, col, None if ks is None else nk)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _launch_rows(b, h_ks)
    t["upload_s"], t["kernel_s"] = t1 - t0, time.perf_counter() - t1
    ap, hits = (None, None) if ks is None else (b.d_ap.cpu().numpy(), b.d_hits[:R * nk].cpu().numpy().reshape(R, nk))
    return b.d_auc.cpu().numpy(), ap, hits, b.d_pos.cpu().numpy(), b.d_neg.cpu().numpy()


def device_metrics(scores, pos_ptr, pos_col, ks, timings=None):
    """device_aucs with average precision and the hits at every cut-off of ks beside the AUC, all in one launch (csrc/rank_metrics.hip):
    -> host (auc [R], ap [R], hits [R, len(ks)], n_pos [R], n_neg [R]); NaN in auc, ap and hits where a row has one class.  The AUCs are
    the bits device_aucs returns.  No CPU fallback; scores on the host or an fp64 device tensor; timings as device_aucs."""
    return _device_rows("device_metrics", scores, pos_ptr, pos_col, ks, timings)


def device_aucs(scores, pos_ptr, pos_col, timings=None):
    """one device launch: host scores fp64 [R, C] and the positives as a CSR -> host (auc [R], n_pos [R], n_neg [R]); NaN AUC where a
    row has one class.  No CPU fallback.  timings: upload_s / kernel_s (host clock around synchronised work).  Scores that are already a
    device tensor (fp64 [R, C], the negated output of gss_profile_dist) go into the kernel where they are."""
    auc, _, _, n_pos, n_neg = _device_rows("device_aucs", scores, pos_ptr, pos_col, None, timings)
    return auc, n_pos, n_neg


def device_metrics_strata(scores, pos_ptr, pos_col, str_ptr, sub_ptr, sub_col, ks, timings=None):
    """device_metrics per stratum of a row (csrc/rank_strata.hip, one launch): row r owns strata str_ptr[r] .. str_ptr[r + 1], stratum s
    has the positives sub_col[sub_ptr[s] .. sub_ptr[s + 1]), a subset of its row's, and is ranked against all of the row's negatives; the
    row's other positives are left out of it -> host (auc [S], ap [S], hits [S, len(ks)], s_pos [S], n_pos [R], n_neg [R]); NaN in auc, ap
    and hits where a stratum is empty or its row has no negative.  Every word is what device_metrics returns for the stratum gathered into
    a row of its own.  Shape checks on the host first; no CPU fallback; scores and timings as device_metrics takes them."""
    import torch

    from . import _lib
    who = "device_metrics_strata"
    s, ptr, col = _device_inputs(who, scores, pos_ptr, pos_col)
    h_ks = check_cuts(who, ks)
    sp, qp, qc = (np.ascontiguousarray(a, dtype=np.int32) for a in (str_ptr, sub_ptr, sub_col))
    (R, C), nk = s.shape, len(h_ks)
    if sp.shape != (R + 1,) or sp[0] != 0 or np.any(np.diff(sp) < 0):
        raise PredictError(f"{who}: the strata's row pointer ({len(sp)} entries) is not one over {R} rows")
    S = int(sp[-1])
    if qp.shape != (S + 1,) or qp[0] != 0 or np.any(np.diff(qp) < 0) or qp[-1] != len(qc):
        raise PredictError(f"{who}: the strata's pointer ({len(qp)} entries over {len(qc)} columns) is not one over {S} strata")
    if R == 0 or S == 0:
        n_pos = np.diff(ptr).astype(np.int32)
        return np.zeros(0), np.zeros(0), np.zeros((0, nk)), np.zeros(0, np.int32), n_pos, (C - n_pos).astype(np.int32)
    t = {} if timings is None else timings
    lib = _lib.load()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev = torch.device("cuda")
    b = _row_buffers(dev, s, ptr, col)
    d_sp, d_qp = torch.from_numpy(sp).to(dev), torch.from_numpy(qp).to(dev)
    d_qc = torch.from_numpy(qc if len(qc) else np.zeros(1, np.int32)).to(dev)
    d_out = torch.empty(S * (2 + max(nk, 1)), dtype=torch.float64, device=dev)       # auc [S], ap [S], hits [S][nk]
    d_cnt = torch.empty(2 * S, dtype=torch.int32, device=dev)                        # s_pos [S], s_neg [S]
    d_work = torch.empty(max(len(qc), 1), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    _lib.check(lib.gss_rank_metrics_strata(R, C, _lib.ptr(b.d_scores), C, _lib.ptr(b.d_ptr), _lib.ptr(b.d_col), S, _lib.ptr(d_sp), _lib.ptr(d_qp),
                                           _lib.ptr(d_qc), nk, h_ks.ctypes.data if nk else None, _lib.ptr(d_out), _lib.ptr(d_out[S:]),
                                           _lib.ptr(d_out[2 * S:]), _lib.ptr(d_cnt), _lib.ptr(d_cnt[S:]), _lib.ptr(b.d_pos), _lib.ptr(b.d_neg),
                                           _lib.ptr(d_work), d_work.numel() * 8, _lib.current_stream()), "gss_rank_metrics_strata")
    t["upload_s"], t["kernel_s"] = t1 - t0, time.perf_counter() - t1
    out = d_out.cpu().numpy()
    return (out[:S], out[S:2 * S], out[2 * S:2 * S + S * nk].reshape(S, nk), d_cnt[:S].cpu().numpy(), b.d_pos.cpu().numpy(),
            b.d_neg.cpu().numpy())


# ---- drug classes: the metrics per (indication, class) ----------------------------------------------------------------------------------

CLASS_HEADER = ["level", "class", "class_name", "drugs", "indications", "positives"]
PER_STRATUM_HEADER = ["level", "class", "indication", "name", "positives", "negatives", "auc"]


def class_columns(drugs, table_drugs, table):
    """classes.read_classes' table on the evaluation's drug columns -> ([(level, code, name, [columns, ascending])] by level, then code,
    of the classes with a member among `drugs`; how many of the table's drugs are no drug column)"""
    col_of = {d: k for k, d in enumerate(drugs)}
    out = []
    for level in sorted(table):
        for code in sorted(table[level]):
            name, members = table[level][code]
            cols = sorted(col_of[d] for d in members if d in col_of)
            if cols:
                out.append((level, code, name, cols))
    return out, sum(1 for d in table_drugs if d not in col_of)


def class_strata(pos_ptr, pos_col, classes, rows=None):
    """classes: [(level, code, name, [drug columns])] -> (str_ptr [R + 1], sub_ptr [S + 1], sub_col, owner [S] = (row, class index)): one
    stratum per (row, class) with a positive of the row among the class's columns, in row order, then class order; its columns in the
    order of the row's pos_col.  A drug in several classes is in several strata.  rows: the rows that get strata (default: every row)."""
    ptr, col = np.asarray(pos_ptr, np.int64), np.asarray(pos_col, np.int64)
    of_col = {}
    for k, cl in enumerate(classes):
        for c in dict.fromkeys(int(c) for c in cl[3]):
            of_col.setdefault(c, []).append(k)
    wanted = None if rows is None else {int(r) for r in rows}
    str_ptr, sub_ptr, sub_col, owner = [0], [0], [], []
    for r in range(len(ptr) - 1):
        if wanted is None or r in wanted:
            members = {}
            for c in col[ptr[r]:ptr[r + 1]]:
                for k in of_col.get(int(c), ()):
                    members.setdefault(k, []).append(int(c))
            for k in sorted(members):
                sub_col += members[k]
                sub_ptr.append(len(sub_col))
                owner.append((r, k))
        str_ptr.append(len(owner))
    return np.asarray(str_ptr, np.int32), np.asarray(sub_ptr, np.int32), np.asarray(sub_col, np.int32), owner


def class_metric_names(metrics):
    """the columns of the class tables: auc, then the requested metrics in order"""
    return ["auc"] + [n for n in metrics if n != "auc"]


class Strata:
    """the per-(indication, class) half of a Result: the classes [(level, code, name, [columns])], owner [S] = (row, class index), the
    strata's CSR, |Q_s| per stratum and {name: fp64 [S]} for auc and the requested metrics"""

    def __init__(self, levels, classes, unknown_drugs, str_ptr, sub_ptr, sub_col, owner, s_pos, values):
        self.levels, self.classes, self.unknown_drugs = list(levels), classes, unknown_drugs
        self.str_ptr, self.sub_ptr, self.sub_col, self.owner = str_ptr, sub_ptr, sub_col, owner
        self.s_pos, self.metrics = np.asarray(s_pos), values
        self.of_class = {}                        # class index -> its strata, in indication order
        for s, (_, k) in enumerate(owner):
            self.of_class.setdefault(k, []).append(s)
        self.line = None

    def class_rows(self, min_indications=1):
        """the per-class table: one row per class with at least min_indications strata, by level, then code"""
        rows = []
        for k, (level, code, name, cols) in enumerate(self.classes):
            idx = self.of_class.get(k, [])
            if len(idx) < max(min_indications, 1):
                continue
            row = [level, code, name, len(cols), len(idx), int(self.s_pos[idx].sum())]
            for v in self.metrics.values():
                row += [repr(float(np.median(v[idx]))), repr(float(v[idx].mean()))]
            rows.append(row)
        return rows


def stratify(res, classes, metrics, pos_ptr, pos_col, strata_source, err):
    """run()'s --by-class half: classes = classes.read_classes' (drugs, table) -> Strata of Result res, over the rows of res.kept alone"""
    table_drugs, table = classes
    cls, unknown = class_columns(res.drugs, table_drugs, table)
    if unknown:
        print(f"evaluate_auc: {unknown} drugs of the class table are not drug nodes of the graph; they are left out", file=err)
    str_ptr, sub_ptr, sub_col, owner = class_strata(pos_ptr, pos_col, cls, rows=res.kept)
    ks = metric_cuts(metrics)
    auc, ap, hits, s_pos, _, _ = strata_source(res.scores, pos_ptr, pos_col, str_ptr, sub_ptr, sub_col, ks)
    names = class_metric_names(metrics)
    values = metric_arrays(names, ks, auc, ap, hits, s_pos)
    return Strata(sorted(table), cls, unknown, str_ptr, sub_ptr, sub_col, owner, s_pos, values)


def write_class_tables(g, res, per_class, per_stratum, min_indications):
    """the two tables of --by-class -> the number of classes written to per_class"""
    st = res.strata
    rows = st.class_rows(min_indications)
    with open(per_class, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", lineterminator="\n")
        w.writerow(CLASS_HEADER + [f"{stat}_{n}" for n in st.metrics for stat in ("median", "mean")])
        w.writerows(rows)
    if per_stratum:
        with open(per_stratum, "w", newline="") as f:
            w = csv.writer(f, delimiter="\t", lineterminator="\n")
            w.writerow(PER_STRATUM_HEADER + list(st.metrics)[1:])
            for s, (r, k) in enumerate(st.owner):
                i = res.indications[r]
                w.writerow([st.classes[k][0], st.classes[k][1], i, display(g, i), int(st.s_pos[s]), int(res.n_neg[r])]
                           + [repr(float(v[s])) for v in st.metrics.values()])
    return len(rows)


# ---- scores and labels ---------------------------------------------------------------------------------------------------------------

def score_rows(s, g, seed):
    """-> (indications, drugs, scores fp64 [len(indications), len(drugs)]), both lists in the reference's node order.  With
    diffusion.compare = a metric the scores are minus the distance between the indication's profile and the drug's, a device tensor that
    never visits the host"""
    if s.method == "diffusion":
        nodelist, profiles = diffusion_profiles(s, g)
        drugs = [n for n in nodelist if g.type.get(n) == DRUG]
        inds = [n for n in nodelist if g.type.get(n) == INDICATION]
        if s.compare != "visit":
            for i in inds:
                if i not in profiles:
                    raise PredictError(f"indication {i!r} has no diffusion profile in {s.diffusion_dir!r}")
            return inds, drugs, -profile_distances(profiles, inds, drugs, s.compare)
        pos = {n: i for i, n in enumerate(nodelist)}
        didx = np.asarray([pos[d] for d in drugs], dtype=np.int64)
        rows = []
        for i in inds:                      # evaluate_auc.py:156-161: the indication's visit probability at each drug node
            if i not in profiles:
                raise PredictError(f"indication {i!r} has no diffusion profile in {s.diffusion_dir!r}")
            p = np.asarray(profiles[i], dtype=np.float64)
            if len(p) != len(nodelist):
                raise PredictError(f"the profile of {i!r} has {len(p)} entries, node2idx.pkl {len(nodelist)}")
            rows.append(p[didx])
    else:
        names, x = embedding_scores(s, g, seed)
        drugs = [n for n in g.names if g.type[n] == DRUG]
        inds = [n for n in g.names if g.type[n] == INDICATION]
        idx = {n: i for i, n in enumerate(names)}
        missing = [n for n in drugs + inds if n not in idx]
        if missing:
            raise PredictError(f"{s.n2v_file}: node {missing[0]!r} has no row ({len(missing)} drug / indication nodes are missing)")
        xd = x[[idx[d] for d in drugs]]
        rows = [np.matmul(xd, np.array(x[idx[i]])) for i in inds]   # predict_drug.py:55-58's arithmetic, one indication at a time
    scores = np.asarray(rows, dtype=np.float64).reshape(len(inds), len(drugs))
    return inds, drugs, scores


def label_rows(inds, drugs, positives):
    """-> (pos_ptr, pos_col, listed {indication: bool}, unknown pairs): the columns of the drugs listed for each indication; listed drugs
    that are not drug nodes of the graph are left out and counted"""
    col_of = {d: k for k, d in enumerate(drugs)}
    ptr, cols, listed, unknown = [0], [], {}, 0
    for i in inds:
        listed[i] = i in positives
        known = sorted(col_of[d] for d in positives.get(i, ()) if d in col_of)
        unknown += len(positives.get(i, ())) - len(known)
        cols += known
        ptr.append(len(cols))
    return np.asarray(ptr, np.int32), np.asarray(cols, np.int32), listed, unknown


class Result:
    def __init__(self, inds, auc, n_pos, n_neg, skipped, unknown, drugs=None, scores=None, ap=None, metrics=None):
        self.indications, self.auc, self.n_pos, self.n_neg = inds, auc, n_pos, n_neg
        self.ap = ap                               # average precision per indication when metrics were asked for, else None
        self.metrics = dict(metrics or {})         # {name: fp64 [indications]} of the requested metrics, in the order asked
        self.drugs, self.scores = drugs, scores    # what was ranked: scores [indications][drugs] (a device tensor under diffusion.compare = a metric)
        self.skipped, self.unknown_pairs = skipped, unknown
        self.kept = [k for k in range(len(inds)) if n_pos[k] > 0 and n_neg[k] > 0]
        self.strata = None                         # the Strata of run(classes=...)
        self.line = format_line(auc[self.kept])
        self.metric_lines = [format_metric_line(name, v[self.kept]) for name, v in self.metrics.items()]   # over the AUC line's indications


def skipped_by_reason(inds, listed, n_pos, n_neg):
    """the indications without an AUC, by reason: no positive (no row in the label table, or none of its listed drugs is a drug node) or
    no negative"""
    skipped = {"no_row": [], "no_known_drug": [], "all_positive": []}
    for k, i in enumerate(inds):
        if n_pos[k] == 0:
            skipped["no_known_drug" if listed[i] else "no_row"].append(i)
        elif n_neg[k] == 0:
            skipped["all_positive"].append(i)
    return skipped


def skip_report(res, labels):
    sk = res.skipped
    total = sum(len(v) for v in sk.values())
    lines = []
    if total:
        lines.append(f"evaluate_auc: skipped {total} of {len(res.indications)} indications: {len(sk['no_row'])} without a row in {labels}, "
                     f"{len(sk['no_known_drug'])} whose listed drugs are not drug nodes of the graph, {len(sk['all_positive'])} with every "
                     "drug listed (one class: ROC-AUC is undefined)")
    if res.unknown_pairs:
        lines.append(f"evaluate_auc: {res.unknown_pairs} listed (drug, indication) pairs name a drug that is not a drug node of the graph; "
                     "they are left out")
    return lines


def write_per_indication(path, g, res):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, delimiter="\t", lineterminator="\n")
        w.writerow(PER_INDICATION_HEADER + list(res.metrics))
        for k in res.kept:
            i = res.indications[k]
            w.writerow([i, display(g, i), int(res.n_pos[k]), int(res.n_neg[k]), repr(float(res.auc[k]))]
                       + [repr(float(v[k])) for v in res.metrics.values()])


def run(s, seed=0, per_indication=None, auc_source=device_aucs, timings=None, err=None, metrics=(), metric_source=device_metrics, classes=None,
        strata_source=device_metrics_strata, per_class="class_metrics.tsv", per_stratum=None, min_indications=1):
    """evaluate_auc.main on Settings s -> Result (per-indication AUCs, counts, skipped indications by reason, the stdout line).
    auc_source(scores, pos_ptr, pos_col) -> (auc, n_pos, n_neg), NaN where a row has one class.  With metrics (names parse_metrics
    accepts) the one call is metric_source(scores, pos_ptr, pos_col, ks) -> (auc, ap, hits [R, len(ks)], n_pos, n_neg) instead, and the
    Result carries ap, the metrics' arrays and one line per metric.  With classes (classes.read_classes' pair: the table's drugs and
    {level: {code: [name, drugs]}}) the Result also carries .strata, the AUC and the metrics of every (indication, class) pair with a listed
    drug in common, out of one call of strata_source (device_metrics_strata's arguments and results), and the two tables are written."""
    metrics = parse_metrics(metrics) if metrics else []
    err = sys.stderr if err is None else err
    t = {} if timings is None else timings
    t0 = time.perf_counter()
    g = MsiGraph().load(s.tables())
    if not os.path.exists(s.graph_out):      # before the diffusion branch weights g in place (evaluate_auc.py:123-129)
        g.write_unweighted_edgelist(s.graph_out)
    else:
        warnings.warn(f"graph struc file {s.graph_out} already exists. change this line if want to overwrite.")
    t1 = time.perf_counter()
    t["graph_s"] = t1 - t0
    with contextlib.redirect_stdout(err):    # progress text of the profile / embedding stage; stdout carries the result line alone
        inds, drugs, scores = score_rows(s, g, seed)
    if not drugs:
        raise PredictError("the graph has no drug node; there is nothing to rank")
    positives = read_drug_indication_tsv(s.labels)
    pos_ptr, pos_col, listed, unknown = label_rows(inds, drugs, positives)
    t2 = time.perf_counter()
    t["scores_s"] = t2 - t1
    ap = values = None
    if metrics:
        ks = metric_cuts(metrics)
        auc, ap, hits, n_pos, n_neg = metric_source(scores, pos_ptr, pos_col, ks)
        ap = np.asarray(ap, np.float64)
        values = metric_arrays(metrics, ks, auc, ap, hits, n_pos)
    else:
        auc, n_pos, n_neg = auc_source(scores, pos_ptr, pos_col)
    t["auc_s"] = time.perf_counter() - t2
    res = Result(inds, np.asarray(auc, np.float64), np.asarray(n_pos), np.asarray(n_neg), skipped_by_reason(inds, listed, n_pos, n_neg), unknown,
                 drugs, scores, ap, values)
    for line in skip_report(res, s.labels):
        print(line, file=err)
    if not res.kept:
        raise PredictError(f"no indication has both a listed drug and an unlisted one in {s.labels!r}; there is no AUC to report")
    if per_indication:
        write_per_indication(per_indication, g, res)
    if classes is not None:
        t3 = time.perf_counter()
        res.strata = stratify(res, classes, metrics, pos_ptr, pos_col, strata_source, err)
        t["strata_s"] = time.perf_counter() - t3
        n = write_class_tables(g, res, per_class, per_stratum, min_indications)
        res.strata.line = (f"classes: {n} classes of levels {','.join(str(k) for k in res.strata.levels)} over {len(res.strata.owner)} "
                           f"(indication, class) pairs: {per_class}")
    t["total_s"] = time.perf_counter() - t0
    return res


# ---- scoring embeddings where they lie: the trainer's model-selection signal ------------------------------------------------------------

class DeviceEvaluator:
    """The gcn / node2vec branch of run() for embeddings that are a device tensor: built once from the MSI tables (the directory of
    networks.protein_to_protein, as Settings.tables), networks.drug_to_indication and the node names of an embedding file (row k of the
    tensor is names[k]); score(emb) then runs gss_embedding_scores and gss_auc_rows on the device and brings back the AUCs and the counts
    alone (with metrics: gss_rank_metrics_rows in place of gss_auc_rows, and the average precisions and hits too).  The lists are run()'s:
    drugs and indications in g.names order, the positives of label_rows.  DESIGN.md sections 9.7 and 9.8.

    Everything that can be wrong with the inputs is found on the host, before upload() touches the GPU."""

    def __init__(self, ppi, labels, names, normalize=True, source="the embedding file", device=None, upload=True):
        self.labels, self.normalize, self.n = labels, bool(normalize), len(names)
        if not os.path.exists(labels):
            raise PredictError(f"networks.drug_to_indication {labels!r} does not exist")
        tables = {name: os.path.join(os.path.dirname(ppi), name + ".tsv") for name, _, _ in COMPONENTS}
        for name, path in tables.items():
            if not os.path.exists(path):
                raise PredictError(f"MSI table {name}: {path!r} does not exist")
        g = MsiGraph().load(tables)
        self.drugs = [n for n in g.names if g.type[n] == DRUG]
        self.indications = [n for n in g.names if g.type[n] == INDICATION]
        idx = {n: i for i, n in enumerate(names)}
        missing = [n for n in self.drugs + self.indications if n not in idx]
        if missing:
            raise PredictError(f"{source}: node {missing[0]!r} has no row ({len(missing)} drug / indication nodes are missing)")
        if not self.drugs:
            raise PredictError("the graph has no drug node; there is nothing to rank")
        if len(self.drugs) > MAX_COLS:
            raise PredictError(f"{len(self.drugs)} drugs per indication is above the limit of {MAX_COLS} (one workgroup sorts a row in LDS)")
        self.rows = np.asarray([idx[i] for i in self.indications], np.int32)
        self.cols = np.asarray([idx[d] for d in self.drugs], np.int32)
        self.pos_ptr, self.pos_col, self.listed, self.unknown_pairs = label_rows(self.indications, self.drugs, read_drug_indication_tsv(labels))
        n_pos = np.diff(self.pos_ptr)
        if not np.any((n_pos > 0) & (n_pos < len(self.drugs))):
            raise PredictError(f"no indication has both a listed drug and an unlisted one in {labels!r}; there is no AUC to report")
        self.device = None
        self.reported = False     # the trainer prints the skip report of the eval graph once
        if upload:
            self.upload(device)

    def upload(self, device=None):
        """the index lists, the positives and the output buffers onto the device (the current one by default)"""
        import torch
        dev = torch.device("cuda") if device is None else torch.device(device)
        R, C = len(self.rows), len(self.cols)
        self.d_rows, self.d_cols = torch.from_numpy(self.rows).to(dev), torch.from_numpy(self.cols).to(dev)
        # the buffers of _launch_rows as attributes of the evaluator: score() launches on itself.  Room for score(metrics=...) at MAX_CUTS cut-offs
        vars(self).update(vars(_row_buffers(dev, torch.empty(R, C, dtype=torch.float64, device=dev), self.pos_ptr, self.pos_col, MAX_CUTS)))
        self.device = self.d_rows.device      # with its index, as a tensor's device has it

    def check_tensor(self, emb, d=None):
        """-> d; refuses by name what score() cannot take.  Host only."""
        import torch
        if not isinstance(emb, torch.Tensor):
            raise PredictError(f"DeviceEvaluator.score: emb is a {type(emb).__name__}, not a torch tensor")
        if emb.dtype != torch.float32:
            raise PredictError(f"DeviceEvaluator.score: emb has dtype {emb.dtype}, not torch.float32")
        if emb.dim() != 2 or emb.shape[0] != self.n:
            raise PredictError(f"DeviceEvaluator.score: emb has shape {tuple(emb.shape)}, but the name list has {self.n} rows")
        if not emb.is_cuda:
            raise PredictError(f"DeviceEvaluator.score: emb is on device {emb.device}, not on the GPU")
        d = emb.shape[1] if d is None else int(d)
        if d < 1 or d > emb.shape[1]:
            raise PredictError(f"DeviceEvaluator.score: d = {d} is outside 1..{emb.shape[1]}, the width of emb")
        if emb.stride(1) != 1 or emb.stride(0) < emb.shape[1]:
            raise PredictError(f"DeviceEvaluator.score: emb has strides {tuple(emb.stride())}; its rows must be contiguous")
        return d

    def score(self, emb, d=None, timings=None, metrics=()):
        """emb: device fp32 [N, >= d], row k = names[k] (d: the leading columns that count; the zero padding behind them changes no bit)
        -> Result.  Result.scores is the evaluator's own device buffer [indications][drugs], which the next score() overwrites: clone it to
        keep it.  timings: scores_s / auc_s / host_s (host clock around synchronised calls).  metrics: names parse_metrics accepts; the
        Result then carries them (run()'s rules), out of one launch of gss_rank_metrics_rows in place of gss_auc_rows."""
        import torch

        from . import _lib
        metrics = parse_metrics(metrics) if metrics else []
        ks = metric_cuts(metrics)
        h_ks = check_cuts("DeviceEvaluator.score", ks)
        d = self.check_tensor(emb, d)
        if self.device is None:
            self.upload(emb.device)
        if emb.device != self.device:
            raise PredictError(f"DeviceEvaluator.score: emb is on device {emb.device}, the evaluator's lists on {self.device}")
        t = {} if timings is None else timings
        lib = _lib.load()
        R, C = len(self.rows), len(self.cols)
        t0 = time.perf_counter()
        with torch.cuda.device(self.device):     # the stream the launches go to is this device's, whichever is current outside
            _lib.check(lib.gss_embedding_scores(self.n, d, _lib.ptr(emb), emb.stride(0), R, _lib.ptr(self.d_rows), C, _lib.ptr(self.d_cols),
                                                int(self.normalize), _lib.ptr(self.d_scores), C, _lib.current_stream()), "gss_embedding_scores")
            t1 = time.perf_counter()
            _launch_rows(self, h_ks if metrics else None)
        t2 = time.perf_counter()
        auc, n_pos, n_neg = self.d_auc.cpu().numpy(), self.d_pos.cpu().numpy(), self.d_neg.cpu().numpy()
        ap = values = None
        if metrics:
            ap = self.d_ap.cpu().numpy()
            hits = self.d_hits[:R * len(ks)].cpu().numpy().reshape(R, len(ks))
            values = metric_arrays(metrics, ks, auc, ap, hits, n_pos)
        res = Result(self.indications, auc, n_pos, n_neg, skipped_by_reason(self.indications, self.listed, n_pos, n_neg), self.unknown_pairs,
                     self.drugs, self.d_scores, ap, values)
        t["scores_s"], t["auc_s"], t["host_s"] = t1 - t0, t2 - t1, time.perf_counter() - t2
        return res


def read_class_table(args):
    """--by-class and its companions, checked before anything touches the GPU -> classes.read_classes' pair, or None without --by-class"""
    from . import classes
    if args.min_indications < 1:
        raise PredictError(f"--min-indications {args.min_indications} must be at least 1")
    if args.by_class is None:
        for flag, value in (("--class-levels", args.class_levels), ("--per-class", args.per_class), ("--per-stratum", args.per_stratum)):
            if value is not None:
                raise PredictError(f"{flag} needs --by-class, the drug-class table")
        return None
    levels = classes.parse_levels("1,2,3,4" if args.class_levels is None else args.class_levels, flag="--class-levels")
    if not os.path.exists(args.by_class):
        raise PredictError(f"--by-class {args.by_class!r} does not exist")
    return classes.read_classes(args.by_class, levels, flag="--by-class")


def main(argv=None, auc_source=device_aucs, metric_source=device_metrics, strata_source=device_metrics_strata):
    """the command line; the three sources are run()'s (the host tests put their mirrors there)"""
    args = parse_args(argv)
    try:
        metrics = parse_metrics(args.metrics) if args.metrics is not None else []
        if args.bootstrap is not None and args.bootstrap < 2:
            raise PredictError(f"--bootstrap {args.bootstrap} must be at least 2")
        if not 0.0 < args.level < 1.0:
            raise PredictError(f"--level {args.level} must lie strictly between 0 and 1")
        by_class = read_class_table(args)
        s = Settings(load_config(args.config))
    except (PredictError, OSError, json.JSONDecodeError) as e:
        print(f"evaluate_auc: {e}", file=sys.stderr)
        sys.exit(2)
    try:
        res = run(s, args.seed, args.per_indication, auc_source=auc_source, metrics=metrics, metric_source=metric_source, classes=by_class,
                  strata_source=strata_source, per_class=args.per_class or "class_metrics.tsv", per_stratum=args.per_stratum,
                  min_indications=args.min_indications)
        extra = bootstrap_lines(res, args.bootstrap, args.level, args.seed) if args.bootstrap is not None else []
    except (PredictError, OSError) as e:
        print(f"evaluate_auc: {e}", file=sys.stderr)
        sys.exit(2)
    print(res.line)
    for line in res.metric_lines:
        print(line)
    for line in extra:
        print(line)
    if res.strata is not None:
        print(res.strata.line)
