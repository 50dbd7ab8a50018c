"""compare_methods.py: how sure are the per-indication numbers, and is one method better than another on this label table?  evaluate_auc.py
prints a median and a mean per method over the indications (evaluate_auc.py:170, point estimates only; the reference has no counterpart of
what follows).  Here every such number gets a bootstrap percentile interval over the indications, and two methods are compared on the
per-indication differences d = a - b: the mean and the median of d with their intervals, and a two-sided sign-flip test of either.

The resampling is a HIP kernel (csrc/resample.hip, gss_resample_stats; no CPU fallback): one workgroup per replicate gathers (bootstrap) or
flips (sign flip) the n values of every series, sorts them in LDS and writes their mean and median.  A replicate draws the same
indications in every series of a call, so the replicates of two methods and of their difference are paired.  What comes back is
[replicates][series][2]; the standard error, np.quantile for the interval and the count behind the p-value are host numpy.  DESIGN.md section
9.13 has the definitions, the cost model and the measurements."""
from __future__ import annotations

import argparse
import csv
import math
import sys

import numpy as np

from . import _lib
from .predict import PredictError, write_tsv

MAX_N = 16384                 # gss_resample_stats sorts a series in LDS
CHUNK_BYTES = 64 << 20        # the replicates come back in calls of at most this many bytes of statistics
MODES = {"plain": 0, "bootstrap": 1, "signflip": 2}
STATS = ("mean", "median")    # the order of the kernel's two outputs
HEADER = ["metric", "method", "baseline", "statistic", "n", "observed", "se", "lo", "hi", "level", "resamples", "p", "permutations", "wins",
          "losses", "ties"]


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------

def _mode(mode):
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"resample_stats: mode {mode!r} is unknown; choose one of {', '.join(MODES)}")
        return MODES[mode]
    return int(mode)


def _series(values, device):
    """-> the device fp64 matrix [S][n] the kernel reads: a device tensor in place, a host array uploaded"""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError(f"resample_stats: device {str(device)!r}: the resampling runs on the GPU only (no CPU fallback)")
    if isinstance(values, torch.Tensor):
        v = values if values.dim() != 1 else values[None, :]
        if not v.is_cuda:
            raise _lib.GssError(f"resample_stats: the tensor is on device {v.device}; the resampling runs on the GPU only (no CPU fallback)")
        if (v.dim() != 2 or v.dtype != torch.float64 or (v.shape[1] > 1 and v.stride(1) != 1) or (v.shape[0] > 1 and v.stride(0) < v.shape[1])):
            raise ValueError("resample_stats: a device tensor must be an fp64 matrix [S][n] with unit column stride and a row stride of at "
                             "least its width")
        return v
    host = np.ascontiguousarray(values, dtype=np.float64)
    if host.ndim == 1:
        host = host[None, :]
    if host.ndim != 2:
        raise ValueError(f"resample_stats: a host array must be [S][n] or [n], not {host.shape}")
    if not torch.cuda.is_available():
        raise _lib.GssError("resample_stats: the resampling runs on the GPU only (no CPU fallback)")
    return torch.from_numpy(host).to(dev)


def resample_stats(values, mode, seed, count, first=0, device="cuda"):
    """the mean and the median of `count` replicates first .. first + count - 1 of every series -> host fp64 [count][S][2] ([..., 0] the mean,
    [..., 1] the median).  values: a numpy array or a device fp64 tensor [S][n] (or [n]: one series); mode: 0 / "plain" (the values
    themselves: count = 1), 1 / "bootstrap" (n draws with replacement, the same places in every series), 2 / "signflip" (each place negated
    with probability 1/2, the same places in every series).  A replicate is a pure function of (seed, mode, its number, the series): a call
    equals the same replicates in any split through `first`, and a series has the same bits alone and among others (gss_resample_stats,
    include/gssgcn.h).  The replicates are computed in calls of at most CHUNK_BYTES of statistics through one device buffer.  No CPU
    fallback: a device other than cuda is refused."""
    import torch
    v = _series(values, device)
    S, n = int(v.shape[0]), int(v.shape[1])
    mode, count, first = _mode(mode), int(count), int(first)
    ld = v.stride(0) if S > 1 else max(n, 1)
    lib = _lib.load()
    out = np.empty((max(count, 0), S, 2), dtype=np.float64)
    step = max(1, min(max(count, 1), CHUNK_BYTES // (16 * max(S, 1))))
    with torch.cuda.device(v.device):
        buf = torch.empty(step, max(S, 1), 2, dtype=torch.float64, device=v.device)
        f = 0
        while True:      # at least one call: the refusals are the kernel's own, whatever the count
            c = min(step, count - f) if count >= 0 else count
            _lib.check(lib.gss_resample_stats(v.data_ptr(), ld, S, n, mode, _lib.seed64(seed), first + f, c, buf.data_ptr(),
                                              _lib.current_stream()), "gss_resample_stats")
            if c > 0:
                out[f:f + c] = buf[:c].cpu().numpy()
            f += max(c, 0)
            if f >= count:
                break
    return out


# ---- the statistics (host) -----------------------------------------------------------------------------------------------------------

def check_level(level):
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"level {level} must lie strictly between 0 and 1")
    return level


def percentile_interval(replicates, level):
    """the central `level` share of the replicates -> (lo, hi): np.quantile at (1 - level) / 2 and 1 - (1 - level) / 2, linear method"""
    a = (1.0 - check_level(level)) / 2.0
    lo, hi = np.quantile(np.asarray(replicates, dtype=np.float64), [a, 1.0 - a])
    return float(lo), float(hi)


def standard_error(replicates):
    """the standard deviation of the replicates (ddof 1); nan for fewer than two"""
    r = np.asarray(replicates, dtype=np.float64)
    return float(np.std(r, ddof=1)) if len(r) > 1 else float("nan")


def sign_flip_p(observed, null):
    """two-sided: p = (1 + #{r : |T_r| >= |T_obs|}) / (R + 1), the comparison exact in fp64 -- the p-value is a count"""
    null = np.asarray(null, dtype=np.float64)
    return (1 + int(np.count_nonzero(np.abs(null) >= abs(float(observed))))) / (len(null) + 1)


def summarize(observed, replicates, level):
    """observed [2] and replicates [B][2] of one series -> {"mean": {observed, se, lo, hi}, "median": {...}}"""
    out = {}
    for k, stat in enumerate(STATS):
        lo, hi = percentile_interval(replicates[:, k], level)
        out[stat] = {"observed": float(observed[k]), "se": standard_error(replicates[:, k]), "lo": lo, "hi": hi}
    return out


def wins_losses_ties(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return int(np.count_nonzero(a > b)), int(np.count_nonzero(a < b)), int(np.count_nonzero(a == b))


def _matrix(series, pairs):
    """the series and, behind them, the difference a - b of every pair (host fp64) -> [S + len(pairs)][n]"""
    names = list(series)
    rows = [np.asarray(series[k], dtype=np.float64).reshape(-1) for k in names]
    if not rows:
        raise ValueError("no series")
    n = len(rows[0])
    for k, r in zip(names, rows):
        if len(r) != n:
            raise ValueError(f"series {k!r} has {len(r)} values, {names[0]!r} has {n}")
    if n < 1 or n > MAX_N:
        raise ValueError(f"{n} values per series is outside [1, {MAX_N}] (the kernel sorts a series in LDS)")
    at = {k: i for i, k in enumerate(names)}
    return np.stack(rows + [rows[at[a]] - rows[at[b]] for a, b in pairs])


def analyse(series, pairs, B, R, seed, level=0.95, device="cuda", source=None):
    """series {name: [n]}, pairs [(a, b)] of names -> ({name: summary}, [paired record per pair]): every series and every difference a - b
    as one device matrix, one plain call, one bootstrap sequence over all rows (so a, b and a - b share their resamples) and one sign-flip
    sequence over the differences.  source: resample_stats (tests put a stub there)."""
    source = resample_stats if source is None else source
    level, B, R = check_level(level), int(B), int(R)
    if B < 2:
        raise ValueError(f"B={B} bootstrap resamples must be at least 2")
    if pairs and R < 1:
        raise ValueError(f"R={R} sign flips must be at least 1")
    names, S = list(series), len(series)
    m = _matrix(series, pairs)
    if source is resample_stats:
        m = _series(m, device)      # uploaded once for the three calls
    observed = source(m, 0, seed, 1, 0, device)[0]
    boot = source(m, 1, seed, B, 0, device)
    null = source(m[S:], 2, seed, R, 0, device) if pairs else None
    summaries = {k: {"n": int(m.shape[1]), **summarize(observed[i], boot[:, i], level)} for i, k in enumerate(names)}
    paired = []
    for j, (a, b) in enumerate(pairs):
        rec = {"a": a, "b": b, "n": int(m.shape[1]), **summarize(observed[S + j], boot[:, S + j], level)}
        for k, stat in enumerate(STATS):
            rec[stat]["p"] = sign_flip_p(observed[S + j, k], null[:, j, k])
        rec["wins"], rec["losses"], rec["ties"] = wins_losses_ties(series[a], series[b])
        paired.append(rec)
    return summaries, paired


def bootstrap_summary(series, B, seed, level=0.95, device="cuda"):
    """series {name: values [n]}, all of one length and in one order -> {name: {"n", "mean": {"observed", "se", "lo", "hi"}, "median": {...}}}:
    the statistic of the values themselves (mode 0), the standard deviation (ddof 1) of its B bootstrap replicates and their percentile
    interval at `level` (np.quantile, linear).  The series share their resamples."""
    return analyse(series, [], B, 0, seed, level, device)[0]


def paired_test(a, b, B, R, seed, level=0.95, device="cuda"):
    """two series over the same indications -> the paired record of d = a - b (host fp64): "n", "wins" / "losses" / "ties" (#a > b, #a < b,
    #a = b), and per statistic "observed", "se", "lo", "hi" (bootstrap, B resamples) and "p", the two-sided sign-flip p-value over R flips;
    under "a" and "b" the summaries of the two series from the same resamples"""
    summaries, paired = analyse({"a": a, "b": b}, [("a", "b")], B, R, seed, level, device)
    return {**paired[0], "a": summaries["a"], "b": summaries["b"]}


# ---- the program ---------------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Drug Repurposing: bootstrap intervals and paired tests of per-indication metrics (compare_methods.py)")
    p.add_argument("--tables", required=True, nargs="+", metavar="METHOD=TSV",
                   help="one table per method, as evaluate_auc.py --per-indication writes it")
    p.add_argument("--metrics", default="auc", type=str, help="comma-separated metric columns to compare (default: auc)")
    p.add_argument("--bootstrap", default=10000, type=int, help="bootstrap resamples of the indications (default: 10000)")
    p.add_argument("--permutations", default=10000, type=int, help="sign flips of the paired differences (default: 10000)")
    p.add_argument("--level", default=0.95, type=float, help="coverage of the percentile intervals (default: 0.95)")
    p.add_argument("--seed", default=0, type=int, help="seed of the resamples and the sign flips (default: 0)")
    p.add_argument("--baseline", default=None, type=str, help="the method every other one is tested against (default: the first table)")
    p.add_argument("--out", default=None, type=str, help="also write the numbers as a TSV: " + ", ".join(HEADER))
    return p.parse_args(argv)


def parse_tables(specs):
    """['method=path', ...] -> [(method, path)], every method once"""
    out = []
    for spec in specs:
        name, sep, path = str(spec).partition("=")
        if not sep or not name or not path:
            raise PredictError(f"--tables {spec!r} must be METHOD=TSV")
        if name in [m for m, _ in out]:
            raise PredictError(f"--tables names method {name!r} twice")
        out.append((name, path))
    return out


def check_args(tables, metrics, bootstrap, permutations, level, baseline):
    """every refusal that needs neither the tables nor the GPU -> (tables, metrics, baseline)"""
    from .evaluate import parse_metrics
    tables = parse_tables(tables)
    metrics = parse_metrics(metrics)
    if bootstrap < 2:
        raise PredictError(f"--bootstrap {bootstrap} must be at least 2")
    if permutations < 1:
        raise PredictError(f"--permutations {permutations} must be at least 1")
    if not 0.0 < level < 1.0:
        raise PredictError(f"--level {level} must lie strictly between 0 and 1")
    baseline = tables[0][0] if baseline is None else baseline
    if baseline not in [m for m, _ in tables]:
        raise PredictError(f"--baseline {baseline!r} is none of the methods {', '.join(m for m, _ in tables)}")
    return tables, metrics, baseline


def read_table(path, metrics):
    """a --per-indication table -> ([indication ids in file order], {metric: {indication: value}})"""
    with open(path, newline="") as f:
        rows = list(csv.reader(f, delimiter="\t"))
    if not rows:
        raise PredictError(f"--tables {path}: the table is empty")
    head = {h: i for i, h in enumerate(rows[0])}
    for col in ["indication"] + list(metrics):
        if col not in head:
            raise PredictError(f"--tables {path}: column {col!r} is missing")
    ids, values = [], {m: {} for m in metrics}
    seen = set()
    for r in rows[1:]:
        if not any(r):
            continue
        r = r + [""] * (len(rows[0]) - len(r))
        i = r[head["indication"]]
        if i in seen:
            raise PredictError(f"--tables {path}: indication {i!r} is duplicated")
        seen.add(i)
        ids.append(i)
        for m in metrics:
            try:
                x = float(r[head[m]])
            except ValueError:
                raise PredictError(f"--tables {path}: indication {i!r}: {m} {r[head[m]]!r} is not a number") from None
            if not math.isfinite(x):
                raise PredictError(f"--tables {path}: indication {i!r}: {m} {r[head[m]]!r} is not finite")
            values[m][i] = x
    return ids, values


def join_tables(tables, metrics, err=None):
    """[(method, path)] -> (the common indications in the first table's order, {metric: {method: fp64 [n]}}); the number of indications
    each table loses to the join goes to err"""
    err = sys.stderr if err is None else err
    read = [(name, path, *read_table(path, metrics)) for name, path in tables]
    common = set(read[0][2])
    for _, _, ids, _ in read[1:]:
        common &= set(ids)
    keep = [i for i in read[0][2] if i in common]
    if not keep:
        raise PredictError(f"the tables {', '.join(p for _, p in tables)} have no indication in common")
    for name, path, ids, _ in read:
        if len(ids) != len(keep):
            print(f"compare_methods: dropped {len(ids) - len(keep)} of {len(ids)} indications of {name} ({path}): not in every table", file=err)
    if len(keep) > MAX_N:
        raise PredictError(f"{len(keep)} common indications are above the limit of {MAX_N} (one workgroup sorts a series in LDS)")
    return keep, {m: {name: np.asarray([values[m][i] for i in keep], dtype=np.float64) for name, _, _, values in read} for m in metrics}


def _interval(s):
    return f"[{s['lo']}, {s['hi']}]"


def method_line(method, metric, s, B):
    return (f"{method} median {metric}: {s['median']['observed']} {_interval(s['median'])}, mean {metric}: {s['mean']['observed']} "
            f"{_interval(s['mean'])} ({s['n']} indications, {B} resamples)")


def paired_line(metric, rec, R):
    return (f"{rec['a']} - {rec['b']} median {metric} difference: {rec['median']['observed']} {_interval(rec['median'])} p = {rec['median']['p']}, "
            f"mean {metric} difference: {rec['mean']['observed']} {_interval(rec['mean'])} p = {rec['mean']['p']} "
            f"({rec['wins']} wins, {rec['losses']} losses, {rec['ties']} ties, {R} sign flips)")


def table_rows(metric, summaries, paired, level, B, R):
    """the rows of --out for one metric: one per (method, statistic), then one per (method against the baseline, statistic)"""
    rows = []
    for method, s in summaries.items():
        for stat in STATS[::-1]:
            rows.append([metric, method, None, stat, s["n"], s[stat]["observed"], s[stat]["se"], s[stat]["lo"], s[stat]["hi"], level, B, None, None, None, None, None])
    for rec in paired:
        for stat in STATS[::-1]:
            rows.append([metric, rec["a"], rec["b"], stat, rec["n"], rec[stat]["observed"], rec[stat]["se"], rec[stat]["lo"], rec[stat]["hi"], level, B,
                         rec[stat]["p"], R, rec["wins"], rec["losses"], rec["ties"]])
    return rows


def run(tables, metrics="auc", bootstrap=10000, permutations=10000, level=0.95, seed=0, baseline=None, out=None, err=None, source=None):
    """the command -> (the stdout lines, the rows of --out).  Every series of every metric and every difference against the baseline goes
    through one analyse(): one device matrix, one bootstrap sequence and one sign-flip sequence for the whole call"""
    tables, metrics, baseline = check_args(tables, metrics, bootstrap, permutations, level, baseline)
    _, values = join_tables(tables, metrics, err)
    methods = [m for m, _ in tables]
    key = lambda metric, method: metric + "\t" + method  # noqa: E731
    series = {key(metric, method): values[metric][method] for metric in metrics for method in methods}
    pairs = [(key(metric, method), key(metric, baseline)) for metric in metrics for method in methods if method != baseline]
    summaries, paired = analyse(series, pairs, bootstrap, permutations, seed, level, source=source)
    lines, rows = [], []
    for metric in metrics:
        of_metric = {method: summaries[key(metric, method)] for method in methods}
        tests = [{**rec, "a": rec["a"].split("\t")[1], "b": rec["b"].split("\t")[1]} for rec in paired if rec["a"].split("\t")[0] == metric]
        lines += [method_line(method, metric, s, bootstrap) for method, s in of_metric.items()]
        lines += [paired_line(metric, rec, permutations) for rec in tests]
        rows += table_rows(metric, of_metric, tests, level, bootstrap, permutations)
    if out:
        write_tsv(out, HEADER, rows)
    return lines, rows


def main(argv=None, source=None):
    args = parse_args(argv)
    try:
        lines, _ = run(args.tables, args.metrics, args.bootstrap, args.permutations, args.level, args.seed, args.baseline, args.out, source=source)
    except (PredictError, OSError) as e:
        print(f"compare_methods: {e}", file=sys.stderr)
        sys.exit(2)
    for line in lines:
        print(line)
