"""GPU: the layers above csrc/rank_metrics.hip -- evaluate.device_metrics on the small fixture against the reference's recorded AUCs,
sklearn and the host mirror; evaluate_auc.py --metrics for node2vec, gcn and diffusion with diffusion.compare set, against
DeviceEvaluator.score(metrics=...) and device_metrics; and train.py --eval-metric / --eval-stat: the trajectory is untouched, --keep-best,
--patience and --resume follow the selected statistic, another pair is refused on resume, and the defaults write what they wrote."""
import contextlib
import io
import os
import re
import shutil
import sys

import numpy as np
import pytest
from sklearn.metrics import average_precision_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluate_fixture as F  # noqa: E402
import rank_metrics_mirror as M  # noqa: E402
from test_gpu_train_eval import NEW_KEYS, Runs, _eval_lines, _fixture_evaluator, _flags, _read_log, _train  # noqa: E402
from test_train_eval import close_pairs, fixture_embeddings, fixture_lists, host_scores  # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ["ap", "recall@50", "recall@3"]
METRIC_LINE = re.compile(r"^median (\S+): (\S+), mean (\S+): (\S+)$")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- device_metrics --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case, normalize", [("gcn", 1), ("node2vec", 0)])
def test_device_metrics_on_the_fixture(case, normalize):
    import torch
    from gcn_drug_repurposing_amd import evaluate
    names, x32 = fixture_embeddings(case)
    inds, drugs, rows, cols, ptr, col = fixture_lists(names)
    scores = host_scores(x32, rows, cols, normalize)
    ks = (3, 50, 1)
    auc, ap, hits, n_pos, n_neg = evaluate.device_metrics(scores, ptr, col, ks)
    kept = [k for k in range(len(inds)) if n_pos[k] > 0 and n_neg[k] > 0]
    F.check_aucs([inds[k] for k in kept], auc[kept], case)
    a0, p0, q0 = evaluate.device_aucs(scores, ptr, col)
    assert np.array_equal(_bits(auc), _bits(a0)) and np.array_equal(n_pos, p0) and np.array_equal(n_neg, q0)
    m_auc, m_ap, m_hits, _, _ = M.mirror_metrics(scores, ptr, col, ks)
    assert np.array_equal(_bits(hits), _bits(m_hits)) and hits.shape == (len(inds), 3)
    C = scores.shape[1]
    for k in kept:
        y = np.zeros(C, int)
        y[col[ptr[k]:ptr[k + 1]]] = 1
        assert abs(ap[k] - m_ap[k]) <= (n_pos[k] + 3) * 2.0 ** -53 * m_ap[k]
        assert abs(ap[k] - average_precision_score(y, scores[k])) <= 1e-12
        order = np.argsort(-scores[k], kind="stable")
        if len(np.unique(scores[k])) == C:                       # no tie: the plain count of the sorted list
            assert [hits[k, j] for j in range(3)] == [float(y[order[:kk]].sum()) for kk in ks]
    if C <= 50:                                                  # a cut at or above C takes every positive
        assert np.array_equal(hits[kept, 1], n_pos[kept].astype(np.float64))
    # device scores go in where they are, and give the same bits
    again = evaluate.device_metrics(torch.from_numpy(scores).cuda(), ptr, col, ks)
    for x, y in zip((auc, ap, hits, n_pos, n_neg), again):
        assert x.tobytes() == y.tobytes()


# ---- evaluate_auc.py --metrics ---------------------------------------------------------------------------------------------------------------

def _main(tmp_path, cfg, extra):
    from gcn_drug_repurposing_amd import evaluate
    per = os.path.join(str(tmp_path), "per.tsv")
    out = io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
        evaluate.main(["-c", cfg, "--per-indication", per] + extra)
    lines = out.getvalue().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in open(per).read().split("\n")[:-1]]
    return lines[:-1], rows


def _check_cli(lines, rows, res):
    """stdout and the TSV of a run with --metrics against a Result with the same metrics: per indication and per line within 1e-12"""
    assert len(lines) == 1 + len(METRICS) and F.LINE.match(lines[0])
    assert rows[0] == ["indication", "name", "positives", "negatives", "auc"] + METRICS
    assert [r[0] for r in rows[1:]] == [res.indications[k] for k in res.kept]
    assert np.max(np.abs(np.asarray([float(r[4]) for r in rows[1:]]) - res.auc[res.kept])) <= 1e-12
    for j, name in enumerate(METRICS):
        colv = np.asarray([float(r[5 + j]) for r in rows[1:]])
        assert np.max(np.abs(colv - res.metrics[name][res.kept])) <= 1e-12, name
        got, want = METRIC_LINE.match(lines[1 + j]), METRIC_LINE.match(res.metric_lines[j])
        assert got and want and got.group(1) == got.group(3) == want.group(1) == name
        assert abs(float(got.group(2)) - float(want.group(2))) <= 1e-12 and abs(float(got.group(4)) - float(want.group(4))) <= 1e-12
        assert lines[1 + j] == f"median {name}: {np.median(colv)}, mean {name}: {colv.mean()}"
    for a, b in zip(F.LINE.match(lines[0]).groups(), F.LINE.match(res.line).groups()):
        assert abs(float(a) - float(b)) <= 1e-12


@pytest.mark.parametrize("case", ["node2vec", "gcn"])
def test_cli_metrics_agree_with_the_device_evaluator(tmp_path, case):
    """the CLI ranks host fp64 scores, the evaluator the device's: the fixture holds no listed / unlisted pair of scores near enough for
    the two to order differently (test_train_eval.py checks it), so every count, and with it every metric, is the same"""
    import torch
    cfg = F.stage(tmp_path, case)
    lines, rows = _main(tmp_path, cfg, ["--metrics", ",".join(METRICS)])
    F.check_line(lines[0], case)
    plain, plain_rows = _main(tmp_path, cfg, [])
    assert plain == lines[:1] and plain_rows == [r[:5] for r in rows]           # without --metrics: the first line and the first five columns
    names, x32 = fixture_embeddings(case)
    inds, drugs, r_, c_, ptr, col = fixture_lists(names)
    assert sum(close_pairs(host_scores(x32, r_, c_, case == "gcn"), ptr, col)) == 0
    ev = _fixture_evaluator(names, normalize=case == "gcn")
    res = ev.score(torch.from_numpy(x32).cuda(), metrics=METRICS)
    assert list(res.metrics) == METRICS and np.array_equal(_bits(res.ap), _bits(res.metrics["ap"]))
    _check_cli(lines, rows, res)
    base = ev.score(torch.from_numpy(x32).cuda())
    assert np.array_equal(_bits(base.auc), _bits(res.auc)) and base.metrics == {} and base.metric_lines == [] and base.ap is None
    scores = res.scores.cpu().numpy()
    _, m_ap, m_hits, _, _ = M.mirror_metrics(scores, ev.pos_ptr, ev.pos_col, (50, 3))
    for k in res.kept:
        assert abs(res.ap[k] - m_ap[k]) <= (res.n_pos[k] + 3) * 2.0 ** -53 * m_ap[k]
        assert res.metrics["recall@50"][k] == m_hits[k, 0] / res.n_pos[k] and res.metrics["recall@3"][k] == m_hits[k, 1] / res.n_pos[k]


def test_cli_metrics_under_diffusion_compare(tmp_path):
    import torch
    from gcn_drug_repurposing_amd import evaluate
    cfg = F.stage(tmp_path, "diffusion", diffusion={"eval_diffusion_embs_dir": str(tmp_path / "dp"), "compare": "correlation"})
    lines, rows = _main(tmp_path, cfg, ["--metrics", ",".join(METRICS)])
    res = evaluate.run(evaluate.Settings(evaluate.load_config(cfg)), metrics=METRICS, err=io.StringIO())      # the saved profiles this time
    assert isinstance(res.scores, torch.Tensor) and res.scores.is_cuda
    scores = res.scores.cpu().numpy()
    ptr, col = evaluate.label_rows(res.indications, res.drugs, evaluate.read_drug_indication_tsv(os.path.join(F.D, "drug_indication_df.tsv")))[:2]
    m_auc, m_ap, m_hits, _, _ = M.mirror_metrics(scores, ptr, col, (50, 3))
    assert np.array_equal(_bits(res.auc), _bits(m_auc))
    for k in res.kept:
        assert abs(res.ap[k] - m_ap[k]) <= (res.n_pos[k] + 3) * 2.0 ** -53 * m_ap[k]
        assert res.metrics["recall@3"][k] == m_hits[k, 1] / res.n_pos[k]
    # the CLI's own run computed its profiles on the device; the second run loaded what it saved.  Where no listed / unlisted pair of
    # the scores is nearer than 1e-9 the two rank alike
    if sum(close_pairs(scores, ptr, col)) == 0:
        _check_cli(lines, rows, res)
    else:
        assert len(lines) == 1 + len(METRICS) and rows[0][5:] == METRICS


# ---- train.py --eval-metric / --eval-stat ----------------------------------------------------------------------------------------------------

AP_MEAN = ("--log-loss", "--eval-metric", "ap", "--eval-stat", "mean")
LOSS = re.compile(r"^iter (\d+) loss (\S+) time")
AP_LINE = re.compile(r"^eval (\d+) median ap: (\S+), mean ap: (\S+)$")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("train_eval_metrics"), lr=0.02)


def _read_metric_log(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "epoch\tmedian_auc\tmean_auc\tindications\tseconds\tmedian_ap\tmean_ap" and lines[-1] == ""
    return [(int(r[0]), float(r[1]), float(r[2]), int(r[3]), float(r[5]), float(r[6])) for r in (l.split("\t") for l in lines[1:-1])]


def _losses(stdout):
    return [m.groups() for m in map(LOSS.match, stdout.split("\n")) if m]


def test_selecting_by_mean_ap_leaves_the_trajectory_alone(runs):
    import torch
    base, sel = runs.evaluated(4, ("--log-loss",)), runs.evaluated(4, AP_MEAN)
    assert len(_losses(base["stdout"])) == 4 and _losses(base["stdout"]) == _losses(sel["stdout"])
    assert open(base["out"], "rb").read() == open(sel["out"], "rb").read() and torch.equal(base["emb"], sel["emb"])
    za, zb = np.load(base["ckpt"]), np.load(sel["ckpt"])
    assert set(zb.files) - set(za.files) == {"eval_metric", "eval_stat"} and set(za.files) <= set(zb.files)
    assert (str(zb["eval_metric"]), str(zb["eval_stat"])) == ("ap", "mean")
    for k in set(za.files) - NEW_KEYS:
        assert za[k].tobytes() == zb[k].tobytes(), k
    # the AUC line stays, the metric's line follows it
    assert _eval_lines(base["stdout"]) == _eval_lines(sel["stdout"])
    out = sel["stdout"].split("\n")
    log = _read_metric_log(sel["log"])
    assert [r[:4] for r in log] == [r[:4] for r in _read_log(base["log"])]
    for e, median, mean in ((r[0], r[4], r[5]) for r in log):
        k = out.index(f"eval {e} median ap: {median!r}, mean ap: {mean!r}")
        assert out[k - 1].startswith(f"eval {e} median auc: ") and out[k - 2].startswith(f"iter {e} ")
    assert not any(AP_LINE.match(l) for l in base["stdout"].split("\n"))
    # the last row is the evaluator's word on the tensor the run ended with
    names, _ = fixture_embeddings("gcn")
    res = _fixture_evaluator(names).score(sel["emb"], 8, metrics=("ap",))
    v = res.metrics["ap"][res.kept]
    assert log[-1][4:] == (float(np.median(v)), float(v.mean()))
    assert float(zb["eval_best_median"]) == max(r[5] for r in log)


def test_keep_best_and_patience_follow_the_mean_ap(runs):
    long = runs.evaluated(4, AP_MEAN)
    means = [r[5] for r in _read_metric_log(long["log"])]
    best = 1 + int(np.argmax(means))                                # the first of equal maxima
    print(f"mean ap by epoch {means}, best epoch {best}")
    assert open(long["best"], "rb").read() == open(runs.plain(best)["out"], "rb").read()
    assert int(np.load(long["ckpt"])["eval_best_epoch"]) == best
    stop = next((e for e in range(2, 5) if means[e - 1] <= max(means[:e - 1])), None)
    run = runs.evaluated(4, AP_MEAN + ("--patience", "1"))
    evals = sorted(_eval_lines(run["stdout"]))
    if stop is None or stop == 4:
        assert evals == [1, 2, 3, 4] and "early stop" not in run["stdout"]
    else:
        assert evals == list(range(1, stop + 1)) and run["stdout"].rstrip("\n").split("\n")[-1] == f"early stop at iter {stop}"
    assert [r[0] for r in _read_metric_log(run["log"])] == evals
    assert open(run["out"], "rb").read() == open(runs.plain(evals[-1])["out"], "rb").read()


def test_resume_continues_the_best_so_far_and_refuses_another_pair(runs, tmp_path):
    two, long = runs.evaluated(2, AP_MEAN), runs.evaluated(4, AP_MEAN)
    ckpt = str(tmp_path / "resume.npz")
    shutil.copy(two["ckpt"], ckpt)
    common = _flags(4, runs.lr) + ["--out", str(tmp_path / "out.txt"), "--eval-config", runs.config]
    _, out, _ = _train(common + ["--checkpoint", ckpt, "--resume", ckpt, "--eval-log", str(tmp_path / "log.tsv")] + list(AP_MEAN))
    assert [l for l in out.split("\n") if AP_LINE.match(l)] == [l for l in long["stdout"].split("\n") if AP_LINE.match(l) and int(l.split()[1]) > 2]
    z, zl = np.load(ckpt), np.load(long["ckpt"])
    assert all(z[k].tobytes() == zl[k].tobytes() for k in NEW_KEYS | {"eval_metric", "eval_stat"})
    assert (tmp_path / "out.txt").read_bytes() == open(long["out"], "rb").read()
    assert [r[0] for r in _read_metric_log(str(tmp_path / "log.tsv"))] == [3, 4]
    # another metric or statistic cannot continue that best value
    for other, text in ((["--eval-metric", "ap"], "--eval-metric ap --eval-stat median"), ([], "--eval-metric auc --eval-stat median"),
                        (["--eval-metric", "recall@3", "--eval-stat", "mean"], "--eval-metric recall@3 --eval-stat mean")):
        with pytest.raises(Exception, match="was written with --eval-metric ap --eval-stat mean") as e:
            _train(common + ["--resume", two["ckpt"]] + other)
        assert text in str(e.value)
    # and a checkpoint of the defaults is refused under another pair
    with pytest.raises(Exception, match="was written with --eval-metric auc --eval-stat median"):
        _train(common + ["--resume", runs.evaluated(2)["ckpt"]] + list(AP_MEAN))


def test_the_defaults_write_what_they_wrote(runs):
    a, b = runs.plain(2), runs.evaluated(2)
    _read_log(b["log"])                                             # today's header, exactly
    za, zb = np.load(a["ckpt"]), np.load(b["ckpt"])
    assert set(zb.files) - set(za.files) == NEW_KEYS
    explicit = runs.evaluated(2, ("--eval-metric", "auc", "--eval-stat", "median"))
    ze = np.load(explicit["ckpt"])
    assert set(ze.files) == set(zb.files) and all(ze[k].tobytes() == zb[k].tobytes() for k in zb.files)
    assert open(explicit["log"]).read().split("\n")[0] == open(b["log"]).read().split("\n")[0]
    told = [[l for l in r["stdout"].split("\n") if l.startswith(("iter ", "eval "))] for r in (explicit, b)]
    assert told[0] == told[1] and len(told[0]) == 4
    # the mean AUC as the selected statistic: no new line or column, the pair recorded
    mean = runs.evaluated(4, ("--eval-stat", "mean"))
    log = _read_log(mean["log"])
    zm = np.load(mean["ckpt"])
    assert (str(zm["eval_metric"]), str(zm["eval_stat"])) == ("auc", "mean")
    assert float(zm["eval_best_median"]) == max(r[2] for r in log) and int(zm["eval_best_epoch"]) == 1 + int(np.argmax([r[2] for r in log]))
