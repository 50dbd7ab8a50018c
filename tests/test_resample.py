"""CPU: the host half of the bootstrap intervals and paired tests (resample.py) and the mirror the GPU tests hold the kernel to
(resample_mirror.py): the mirror against plain numpy, the range of the draw, the p-value and interval arithmetic on hand-made replicates, the
program's join and refusals with the mirror in the kernel's place, and the entry point's place in the header, the library and the binding."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import resample_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import evaluate as E  # noqa: E402
from gcn_drug_repurposing_amd import resample as R  # noqa: E402
from gcn_drug_repurposing_amd.predict import PredictError  # noqa: E402


def mirror_source(m, mode, seed, count, first=0, device=None):
    """resample.resample_stats' signature over the mirror: what the program's host half runs on without a GPU"""
    return M.resample_stats(m, mode, seed, count, first)


# ---- the mirror against plain numpy --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025))
def test_mirror_median_is_numpys_and_the_mean_is_inside_the_any_order_bound(n):
    rng = np.random.RandomState(n)
    v = rng.randn(n)
    v[rng.randint(0, n, n // 3)] = v[0]                 # ties
    for mode in (M.PLAIN, M.BOOTSTRAP, M.SIGN_FLIP):
        for b in range(1 if mode == M.PLAIN else 4):
            values = M.gathered(v, mode, 3, b)
            x = M.multiset(v, mode, 3, b)
            assert len(x) == n and np.all(np.diff(x) >= 0) and np.array_equal(np.sort(values + 0.0), x)
            mean, med = M.stats_of(x)
            assert np.array([med]).view(np.uint64)[0] == np.array([np.median(values) + 0.0]).view(np.uint64)[0]
            assert abs(mean - math.fsum(values) / n) <= M.mean_bound(values), (n, mode, b)
    assert np.array_equal(M.gathered(v, M.PLAIN, 0, 0), v)
    assert np.array_equal(np.abs(M.gathered(v, M.SIGN_FLIP, 3, 1)), np.abs(v))
    assert set(M.gathered(v, M.BOOTSTRAP, 3, 1)) <= set(v)


def test_mirror_sum_order_is_the_stated_one():
    x = np.sort(np.random.RandomState(1).randn(700))
    p = [0.0] * 256
    for i, t in enumerate(x):
        p[i % 256] += t                                  # lane-strided, ascending
    waves = []
    for w in range(4):
        q = p[64 * w:64 * w + 64]
        for o in (32, 16, 8, 4, 2, 1):
            q = [q[l] + q[l ^ o] for l in range(64)]
        waves.append(q[0])
    assert M.ordered_sum(x) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert M.ordered_sum(np.array([2.5])) == 2.5 and M.median(np.array([1.0, 2.0, 4.0, 8.0])) == 3.0 and M.median(np.array([1.0, 2.0, 4.0])) == 2.0


def test_draw_is_in_range_and_replicates_differ():
    for n in (1, 2, 3, 16384):
        for seed, b in ((0, 0), (2 ** 63 + 5, 1), (7, 2 ** 31 - 1)):
            idx = M.draw(seed, b, n)
            assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < n
    assert np.all(M.draw(9, 4, 1) == 0)
    assert not np.array_equal(M.draw(1, 0, 64), M.draw(1, 1, 64)) and not np.array_equal(M.draw(1, 0, 64), M.draw(2, 0, 64))
    assert not np.array_equal(M.flips(1, 0, 64), M.flips(1, 1, 64)) and M.flips(1, 0, 64).dtype == bool
    # printed, not asserted: how even 100,000 draws at n = 7 are, and the share of flipped signs
    counts = np.bincount(np.concatenate([M.draw(0, b, 7) for b in range(100000 // 7 + 1)])[:100000], minlength=7)
    print("draw frequencies over 100,000 draws at n = 7:", (counts / 100000).round(5).tolist())
    print("share of flipped signs over 100,000 places:", float(np.mean([M.flips(0, b, 100) for b in range(1000)])))


# ---- p-values and intervals on hand-made replicates ----------------------------------------------------------------------------------

def test_p_value_is_a_count():
    null = np.array([0.5, -0.5, 0.25, -1.0, 0.0, 0.75, -0.75, 0.1, 0.2])
    assert R.sign_flip_p(0.75, null) == (1 + 3) / 10          # -1.0, 0.75, -0.75: two-sided, ties count
    assert R.sign_flip_p(-0.75, null) == (1 + 3) / 10
    assert R.sign_flip_p(2.0, null) == 1 / 10                 # no replicate reaches the observed value
    assert R.sign_flip_p(0.0, np.zeros(99)) == 1.0            # d all zeros: every replicate ties
    assert R.sign_flip_p(np.nextafter(0.75, 1), null) == (1 + 1) / 10      # the comparison is exact in fp64


def test_intervals_and_standard_error():
    reps = np.arange(101, dtype=np.float64)[::-1].copy()
    assert R.percentile_interval(reps, 0.5) == (25.0, 75.0)
    lo, hi = R.percentile_interval(reps, 0.95)          # (1 - 0.95) / 2 is not 0.025 to the last bit: the quantile's own arithmetic
    assert abs(lo - 2.5) <= 1e-12 and abs(hi - 97.5) <= 1e-12 and (lo, hi) == tuple(np.quantile(reps, [(1 - 0.95) / 2, 1 - (1 - 0.95) / 2]))
    rng = np.random.RandomState(2)
    r = rng.randn(1000, 2)
    s = R.summarize(np.array([0.1, 0.2]), r, 0.9)
    for k, stat in enumerate(("mean", "median")):
        lo, hi = np.quantile(r[:, k], [0.05, 0.95])
        assert s[stat] == {"observed": 0.1 * (k + 1), "se": float(np.std(r[:, k], ddof=1)), "lo": float(lo), "hi": float(hi)}
        assert s[stat]["lo"] <= s[stat]["hi"]
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="strictly between 0 and 1"):
            R.percentile_interval(reps, bad)
    assert R.wins_losses_ties([1, 2, 3, 4], [0, 2, 5, 4]) == (1, 1, 2)


def test_analyse_pairs_the_series_through_the_replicates():
    rng = np.random.RandomState(4)
    a, b = rng.rand(30), rng.rand(30)
    summaries, paired = R.analyse({"a": a, "b": b}, [("a", "b")], 200, 300, 5, 0.9, source=mirror_source)
    boot = M.resample_stats(np.stack([a, b, a - b]), M.BOOTSTRAP, 5, 200)
    null = M.resample_stats(a - b, M.SIGN_FLIP, 5, 300)[:, 0]
    observed = M.resample_stats(np.stack([a, b, a - b]), M.PLAIN, 5, 1)[0]
    assert observed[0, 1] == np.median(a) and observed[2, 1] == np.median(a - b)
    for i, k in enumerate(("a", "b")):
        assert summaries[k] == {"n": 30, **R.summarize(observed[i], boot[:, i], 0.9)}
    rec = paired[0]
    for k, stat in enumerate(R.STATS):
        assert rec[stat]["p"] == (1 + int(np.sum(np.abs(null[:, k]) >= abs(observed[2, k])))) / 301
        assert (rec[stat]["lo"], rec[stat]["hi"]) == R.percentile_interval(boot[:, 2, k], 0.9)
    assert (rec["wins"], rec["losses"], rec["ties"]) == (int(np.sum(a > b)), int(np.sum(a < b)), 0) and rec["n"] == 30
    # the difference of the paired bootstrap means is the bootstrap mean of the difference, up to rounding: the same places were drawn
    assert np.max(np.abs((boot[:, 0, 0] - boot[:, 1, 0]) - boot[:, 2, 0])) <= 1e-15
    for call, words in ((lambda: R.analyse({"a": a}, [], 1, 0, 0, source=mirror_source), "B=1 bootstrap resamples must be at least 2"),
                        (lambda: R.analyse({"a": a, "b": b[:5]}, [], 10, 0, 0, source=mirror_source), "series 'b' has 5 values, 'a' has 30"),
                        (lambda: R.analyse({"a": a, "b": b}, [("a", "b")], 10, 0, 0, source=mirror_source), "R=0 sign flips must be at least 1"),
                        (lambda: R.analyse({"a": np.zeros(R.MAX_N + 1)}, [], 10, 0, 0, source=mirror_source), "outside [1, 16384]")):
        with pytest.raises(ValueError, match=re.escape(words)):
            call()


# ---- the program: join, lines and refusals, with the mirror in the kernel's place ----------------------------------------------------

def write_table(path, rows, metrics=("auc", "ap"), head=None):
    head = E.PER_INDICATION_HEADER[:4] + list(metrics) if head is None else head
    path.write_text("\t".join(head) + "\n" + "".join("\t".join(str(c) for c in r) + "\n" for r in rows))
    return str(path)


def table_rows(ids, seed):
    rng = np.random.RandomState(seed)
    return [[i, "name of " + i, 2, 9, repr(float(rng.rand())), repr(float(rng.rand()))] for i in ids]


def test_program_joins_the_tables_and_writes_what_it_prints(tmp_path, capsys):
    ids = [f"C{k:03d}" for k in range(12)]
    ta = write_table(tmp_path / "a.tsv", table_rows(ids, 1))
    tb = write_table(tmp_path / "b.tsv", table_rows(ids[2:][::-1] + ["C900"], 2))       # another order, two missing, one extra
    tc = write_table(tmp_path / "c.tsv", table_rows(ids[:11], 3))
    argv = ["--tables", f"diffusion={ta}", f"gcn={tb}", f"node2vec={tc}", "--metrics", "auc,ap", "--bootstrap", "50", "--permutations", "60",
            "--seed", "4", "--level", "0.9", "--baseline", "gcn", "--out", str(tmp_path / "out.tsv")]
    R.main(argv, source=mirror_source)
    cap = capsys.readouterr()
    assert cap.err.split("\n") == [f"compare_methods: dropped 3 of 12 indications of diffusion ({ta}): not in every table",
                                   f"compare_methods: dropped 2 of 11 indications of gcn ({tb}): not in every table",
                                   f"compare_methods: dropped 2 of 11 indications of node2vec ({tc}): not in every table", ""]
    lines = cap.out.split("\n")
    assert len(lines) == 2 * (3 + 2) + 1 and lines[-1] == ""
    keep = ids[2:11]                                                                    # the first table's order
    read = {name: R.read_table(p, ["auc", "ap"])[1] for name, p in (("diffusion", ta), ("gcn", tb), ("node2vec", tc))}
    for m, metric in enumerate(("auc", "ap")):
        series = {name: np.array([read[name][metric][i] for i in keep]) for name in read}
        for k, name in enumerate(series):
            s = R.analyse(series, [], 50, 0, 4, 0.9, source=mirror_source)[0][name]
            assert s["median"]["observed"] == np.median(series[name])
            assert lines[5 * m + k].startswith(f"{name} median {metric}: {s['median']['observed']} [") and lines[5 * m + k].endswith("(9 indications, 50 resamples)")
        for k, name in enumerate(("diffusion", "node2vec")):
            line = lines[5 * m + 3 + k]
            w, l, t = R.wins_losses_ties(series[name], series["gcn"])
            assert line.startswith(f"{name} - gcn median {metric} difference: {np.median(series[name] - series['gcn'])} [")
            assert line.endswith(f"({w} wins, {l} losses, {t} ties, 60 sign flips)")
    # --out: the header, one row per (metric, method or pair, statistic), every float repr'd -- and the numbers of the lines
    rows = [r.split("\t") for r in (tmp_path / "out.tsv").read_text().split("\n")[:-1]]
    assert rows[0] == R.HEADER and len(rows) == 1 + 2 * 2 * (3 + 2)
    for r in rows[1:]:
        rec = dict(zip(R.HEADER, r))
        for col in ("observed", "se", "lo", "hi", "level"):
            assert repr(float(rec[col])) == rec[col]
        assert float(rec["lo"]) <= float(rec["hi"]) and rec["n"] == "9" and rec["resamples"] == "50"
        if rec["baseline"] == "NA":
            assert rec["p"] == rec["wins"] == "NA"
            line = next(x for x in lines if x.startswith(f"{rec['method']} median {rec['metric']}: "))
        else:
            assert rec["baseline"] == "gcn" and repr(float(rec["p"])) == rec["p"] and rec["permutations"] == "60"
            line = next(x for x in lines if x.startswith(f"{rec['method']} - gcn median {rec['metric']} difference: "))
        assert f"{rec['statistic']} {rec['metric']}{'' if rec['baseline'] == 'NA' else ' difference'}: {rec['observed']} [{rec['lo']}, {rec['hi']}]" in line
    # the whole call is one matrix: every series of every metric and every difference share their resamples
    calls = []

    def counting(m, mode, seed, count, first=0, device=None):
        calls.append((np.asarray(m).shape, mode, count))
        return M.resample_stats(m, mode, seed, count, first)

    R.run([f"diffusion={ta}", f"gcn={tb}", f"node2vec={tc}"], "auc,ap", 50, 60, 0.9, 4, "gcn", err=open(os.devnull, "w"), source=counting)
    assert calls == [((10, 9), 0, 1), ((10, 9), 1, 50), ((4, 9), 2, 60)]


def test_program_refusals_exit_2_with_one_line(tmp_path, capsys):
    ids = [f"C{k:03d}" for k in range(5)]
    good = write_table(tmp_path / "a.tsv", table_rows(ids, 1))
    no_ap = write_table(tmp_path / "b.tsv", [r[:5] for r in table_rows(ids, 2)], metrics=("auc",))
    twice = write_table(tmp_path / "c.tsv", table_rows(ids + ["C002"], 3))
    other = write_table(tmp_path / "d.tsv", table_rows(["X1", "X2"], 4))
    nan = table_rows(ids, 5)
    nan[3][4] = "nan"
    bad = write_table(tmp_path / "e.tsv", nan)
    inf = table_rows(ids, 5)
    inf[1][5] = "inf"
    worse = write_table(tmp_path / "f.tsv", inf)
    word = table_rows(ids, 5)
    word[0][4] = "high"
    text = write_table(tmp_path / "g.tsv", word)
    for argv, words in ((["--tables", f"x={good}", f"y={no_ap}", "--metrics", "auc,ap"], f"--tables {no_ap}: column 'ap' is missing"),
                        (["--tables", f"x={good}", f"y={twice}"], f"--tables {twice}: indication 'C002' is duplicated"),
                        (["--tables", f"x={good}", f"y={bad}"], f"--tables {bad}: indication 'C003': auc 'nan' is not finite"),
                        (["--tables", f"x={good}", f"y={worse}", "--metrics", "ap"], f"--tables {worse}: indication 'C001': ap 'inf' is not finite"),
                        (["--tables", f"x={good}", f"y={text}"], f"--tables {text}: indication 'C000': auc 'high' is not a number"),
                        (["--tables", f"x={good}", f"y={other}"], "have no indication in common"),
                        (["--tables", f"x={good}", f"x={good}"], "--tables names method 'x' twice"),
                        (["--tables", good], "must be METHOD=TSV"),
                        (["--tables", f"x={good}", "--metrics", "f1"], "metric 'f1' is unknown"),
                        (["--tables", f"x={good}", "--bootstrap", "1"], "--bootstrap 1 must be at least 2"),
                        (["--tables", f"x={good}", "--permutations", "0"], "--permutations 0 must be at least 1"),
                        (["--tables", f"x={good}", "--level", "1.0"], "--level 1.0 must lie strictly between 0 and 1"),
                        (["--tables", f"x={good}", "--baseline", "y"], "--baseline 'y' is none of the methods x"),
                        (["--tables", f"x={tmp_path / 'none.tsv'}"], "none.tsv")):
        with pytest.raises(SystemExit) as e:
            R.main(argv + ["--out", str(tmp_path / "out.tsv")], source=mirror_source)
        cap = capsys.readouterr()
        assert e.value.code == 2 and cap.out == "" and cap.err.startswith("compare_methods: ") and cap.err.count("\n") == 1 and words in cap.err, cap.err
    assert not os.path.exists(tmp_path / "out.tsv")
    with pytest.raises(PredictError, match="have no indication in common"):
        R.join_tables([("x", good), ("y", other)], ["auc"], err=open(os.devnull, "w"))


def test_evaluate_bootstrap_lines_and_refusals(tmp_path, capsys):
    class Res:
        auc = np.array([0.5, np.nan, 0.75, 1.0, 0.25])
        kept = [0, 2, 3, 4]
        metrics = {"ap": np.array([0.1, np.nan, 0.2, 0.3, 0.4])}

    def summary(series, B, seed, level):
        return R.analyse(series, [], B, 0, seed, level, source=mirror_source)[0]

    lines = E.bootstrap_lines(Res, 40, 0.9, 3, summary=summary)
    want = summary({"auc": Res.auc[Res.kept], "ap": Res.metrics["ap"][Res.kept]}, 40, 3, 0.9)
    assert lines == [f"bootstrap {k}: median [{s['median']['lo']}, {s['median']['hi']}], mean [{s['mean']['lo']}, {s['mean']['hi']}] (40 resamples, seed 3)"
                     for k, s in want.items()] and len(lines) == 2
    for argv, words in ((["--bootstrap", "1"], "--bootstrap 1 must be at least 2"), (["--bootstrap", "10", "--level", "0"], "--level 0.0 must lie")):
        with pytest.raises(SystemExit) as e:
            E.main(["-c", str(tmp_path / "none.json")] + argv)
        assert e.value.code == 2 and words in capsys.readouterr().err


# ---- the entry point in the header, the library and the binding ----------------------------------------------------------------------

def test_abi_25_carries_the_entry_point():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    lib = pkg.load()
    header = open(os.path.join(ROOT, "include", "gssgcn.h")).read()
    assert "#define GSS_ABI_VERSION 25 " in header and " 25: the mean and the median of bootstrap resamples" in header
    assert pkg._lib.ABI_VERSION == lib.gss_abi_version() == 25
    assert re.search(r"\bint gss_resample_stats\(const double \*v, int64_t ld, int32_t S, int32_t n, int32_t mode, uint64_t seed, int64_t first, "
                     r"int64_t count, double \*out,\s+void \*stream\);", header)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T gss_resample_stats\n" in out
    restype, argtypes = pkg._lib.SIGNATURES["gss_resample_stats"]
    import ctypes as C
    assert restype is C.c_int and [C.sizeof(t) for t in argtypes] == [8, 8, 4, 4, 4, 8, 8, 8, 8, 8] and argtypes[5] is C.c_uint64
    assert lib.gss_resample_stats.argtypes == argtypes
    # the refusals that need no device: the arguments alone
    for args, words in (((0, 5, 1, 0, 1, 0, 0, 1, 0, 0), "n=0 is outside [1, 16384]"), ((0, 5, 1, 16385, 1, 0, 0, 1, 0, 0), "n=16385 is outside"),
                        ((0, 4, 1, 5, 1, 0, 0, 1, 0, 0), "ld=4 is below n=5"), ((0, 5, 1, 5, 3, 0, 0, 1, 0, 0), "mode=3 is unknown"),
                        ((0, 5, 1, 5, 0, 0, 0, 2, 0, 0), "mode 0 (plain) has one replicate"), ((0, 5, 1, 5, 1, 0, 2 ** 31, 1, 0, 0), "reach outside [0, 2^31]"),
                        ((0, 5, 1, 5, 1, 0, 0, 1, 0, 0), "v is null")):
        assert lib.gss_resample_stats(*args) == -22 and words in lib.gss_last_error().decode(), words
    assert lib.gss_resample_stats(0, 5, 1, 5, 1, 0, 7, 0, 0, 0) == 0      # count = 0: nothing to do, nothing read
    rng_h = open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "counter_rng.h")).read()
    assert f"kRngBootDraw = {M.TAG_BOOT_DRAW}," in rng_h and f"kRngSignFlip = {M.TAG_SIGN_FLIP}," in rng_h
