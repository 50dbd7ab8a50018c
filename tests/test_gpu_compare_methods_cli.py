"""GPU: compare_methods.py and evaluate_auc.py --bootstrap end to end on the small fixture (tests/golden/evaluate_msi_small: nine indications
with both classes).  The three --per-indication tables are written by the existing program, once; compare_methods.py then runs on them as a
program.  Its observed medians and means are the reference's recorded lines (expected.json), its intervals and p-values those of
resample.bootstrap_summary / paired_test called directly with the same seed -- a series has the same bits alone and among others -- and its
output is the same bytes run to run and through --out."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_fixture as F  # noqa: E402

from gcn_drug_repurposing_amd import evaluate as E  # noqa: E402
from gcn_drug_repurposing_amd import resample as R  # noqa: E402

pytestmark = pytest.mark.gpu

METHODS = ("diffusion", "node2vec", "gcn")
METRICS = ["auc", "ap", "recall@2"]
B, FLIPS, SEED, LEVEL = 300, 400, 5, 0.9
BOOT = 200          # evaluate_auc.py --bootstrap, on the gcn run


def program(name, args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, name)] + args, cwd=str(cwd), capture_output=True, text=True, env=env, timeout=600)


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """evaluate_auc.py --per-indication --metrics auc,ap,recall@2 for the three methods (gcn also with --bootstrap) -> {method: (table path,
    stdout, config path)}"""
    out = {}
    for method in METHODS:
        tmp = tmp_path_factory.mktemp(method)
        cfg = F.stage(tmp, method)
        extra = ["--bootstrap", str(BOOT), "--level", str(LEVEL), "--seed", str(SEED)] if method == "gcn" else []
        r = program("evaluate_auc.py", ["-c", cfg, "--per-indication", "per.tsv", "--metrics", ",".join(METRICS)] + extra, tmp)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        out[method] = (str(tmp / "per.tsv"), r.stdout, cfg)
    return out


def table_args(tables):
    return ["--tables"] + [f"{m}={tables[m][0]}" for m in METHODS]


def test_compare_methods_end_to_end(tables, tmp_path, capsys):
    args = table_args(tables) + ["--metrics", ",".join(METRICS), "--bootstrap", str(B), "--permutations", str(FLIPS), "--level", str(LEVEL),
                                 "--seed", str(SEED)]
    r = program("compare_methods.py", args + ["--out", "comparison.tsv"], tmp_path)
    assert r.returncode == 0 and "compare_methods:" not in r.stderr, r.stdout[-3000:] + r.stderr[-3000:]      # nothing dropped, nothing refused
    lines = r.stdout.split("\n")
    assert len(lines) == len(METRICS) * (3 + 2) + 1 and lines[-1] == ""

    # run to run: the same bytes, on stdout and in --out
    R.main(args + ["--out", str(tmp_path / "again.tsv")])
    assert capsys.readouterr().out == r.stdout
    text = (tmp_path / "comparison.tsv").read_text()
    assert text == (tmp_path / "again.tsv").read_text()

    # --out: the numbers of the lines, every float through repr; no NaN, no reversed interval
    rows = [dict(zip(R.HEADER, x.split("\t"))) for x in text.split("\n")[1:-1]]
    assert text.split("\n")[0].split("\t") == R.HEADER and len(rows) == len(METRICS) * 2 * (3 + 2)
    for rec in rows:
        for col in ("observed", "se", "lo", "hi", "p"):
            if rec[col] != "NA":
                assert repr(float(rec[col])) == rec[col] and np.isfinite(float(rec[col])), rec
        assert float(rec["lo"]) <= float(rec["hi"]) and rec["n"] == "9" and rec["resamples"] == str(B) and float(rec["level"]) == LEVEL
        which = f"{rec['method']} median" if rec["baseline"] == "NA" else f"{rec['method']} - diffusion median"
        line = next(x for x in lines if x.startswith(f"{which} {rec['metric']}"))
        diff = "" if rec["baseline"] == "NA" else " difference"
        assert f"{rec['statistic']} {rec['metric']}{diff}: {rec['observed']} [{rec['lo']}, {rec['hi']}]" in line, (rec, line)
        if rec["baseline"] != "NA":
            assert f"[{rec['lo']}, {rec['hi']}] p = {rec['p']}" in line and 1 / (FLIPS + 1) <= float(rec["p"]) <= 1.0
            assert round(float(rec["p"]) * (FLIPS + 1)) / (FLIPS + 1) == float(rec["p"])        # a count over R + 1
    get = lambda metric, method, baseline, stat: next(x for x in rows if (x["metric"], x["method"], x["baseline"], x["statistic"])  # noqa: E731
                                                      == (metric, method, baseline, stat))

    # the observed medians and means: the reference's recorded lines, and the existing program's own
    for method in METHODS:
        want = F.LINE.match(F.expected()[method]["line"])
        for stat, w in zip(("median", "mean"), want.groups()):
            assert abs(float(get("auc", method, "NA", stat)["observed"]) - float(w)) <= 1e-12, (method, stat)

    # the intervals and the p-values: resample.py called directly with the same seed
    _, values = R.join_tables([(m, tables[m][0]) for m in METHODS], METRICS)
    for metric in METRICS:
        summary = R.bootstrap_summary(values[metric], B, SEED, LEVEL)
        for method in METHODS:
            for stat in R.STATS:
                rec = get(metric, method, "NA", stat)
                assert {k: float(rec[k]) for k in ("observed", "se", "lo", "hi")} == summary[method][stat], (metric, method, stat)
        for method in METHODS[1:]:
            test = R.paired_test(values[metric][method], values[metric]["diffusion"], B, FLIPS, SEED, LEVEL)
            for stat in R.STATS:
                rec = get(metric, method, "diffusion", stat)
                assert {k: float(rec[k]) for k in ("observed", "se", "lo", "hi", "p")} == test[stat], (metric, method, stat)
            assert (int(rec["wins"]), int(rec["losses"]), int(rec["ties"])) == (test["wins"], test["losses"], test["ties"])
            assert test["wins"] + test["losses"] + test["ties"] == 9


def test_compare_methods_refusals(tables, tmp_path):
    per = tables["gcn"][0]
    head, *body = open(per).read().split("\n")[:-1]
    cut = head.split("\t").index("ap")
    (tmp_path / "no_ap.tsv").write_text("\n".join("\t".join(c for k, c in enumerate(x.split("\t")) if k != cut) for x in [head] + body) + "\n")
    (tmp_path / "twice.tsv").write_text("\n".join([head] + body + [body[2]]) + "\n")
    (tmp_path / "other.tsv").write_text("\n".join([head] + ["X" + x for x in body]) + "\n")
    repeated = body[2].split("\t")[0]
    for name, words in (("no_ap.tsv", "column 'ap' is missing"), ("twice.tsv", f"indication {repeated!r} is duplicated"),
                        ("other.tsv", "have no indication in common")):
        r = program("compare_methods.py", ["--tables", f"gcn={per}", f"x={tmp_path / name}", "--metrics", "auc,ap", "--out", "o.tsv"], tmp_path)
        assert r.returncode == 2 and r.stdout == "" and r.stderr.startswith("compare_methods: ") and r.stderr.count("\n") == 1, r.stderr
        assert words in r.stderr
    assert not os.path.exists(tmp_path / "o.tsv")


def test_evaluate_auc_prints_what_it_printed_and_the_bootstrap_lines(tables):
    for method in METHODS:
        per, stdout, cfg = tables[method]
        lines = stdout.split("\n")
        assert lines[-1] == ""
        F.check_line(lines[0], method)                                       # the reference's recorded line
        inds, aucs, rows = [r[0] for r in read_rows(per)], [float(r[4]) for r in read_rows(per)], read_rows(per)
        F.check_aucs(inds, aucs, method)
        # exactly the lines of the program without the flag: the AUC line and one line per metric, from the table's own values
        head = open(per).readline().rstrip("\n").split("\t")
        want = [E.format_line(aucs)] + [E.format_metric_line(m, [float(r[head.index(m)]) for r in rows]) for m in METRICS]
        assert lines[:4] == want
        if method != "gcn":
            assert len(lines) == 5                                           # nothing else without --bootstrap
            continue
        series = {"auc": np.asarray(aucs)}
        series.update({m: np.asarray([float(r[head.index(m)]) for r in rows]) for m in METRICS})
        summary = R.bootstrap_summary(series, BOOT, SEED, LEVEL)
        assert list(summary) == METRICS and len(lines) == 5 + len(METRICS)
        for line, (name, s) in zip(lines[4:], summary.items()):
            assert line == E.format_bootstrap_line(name, s, BOOT, SEED)
            lo, hi = re.match(r"^bootstrap \S+: median \[(\S+), (\S+)\], mean ", line).groups()
            assert float(lo) <= np.median(series[name]) <= float(hi)


def read_rows(path):
    return [x.split("\t") for x in open(path).read().split("\n")[1:-1]]
