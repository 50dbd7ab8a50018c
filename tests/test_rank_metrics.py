"""CPU: the host mirror of csrc/rank_metrics.hip (rank_metrics_mirror.py) against sklearn's average precision, against a stable argsort
and against every tie-breaking order of a small group; the mirror's AP in the kernel's order of additions against its exact value;
the metric-name parser; evaluate_auc.py --metrics end to end on the
evaluate_msi_small fixture with the mirror in place of the device; and the trainer's --eval-metric / --eval-stat checks that need no GPU.
The device side is in test_gpu_rank_metrics.py and test_gpu_evaluate_metrics.py."""
import io
import itertools
import os
import sys
from contextlib import redirect_stderr, redirect_stdout
from fractions import Fraction

import numpy as np
import pytest
from sklearn.metrics import average_precision_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluate_fixture as F  # noqa: E402
import rank_metrics_mirror as M  # noqa: E402


def tied_row(rng, C, levels):
    s = rng.randint(-levels, levels + 1, C) * 0.5
    zero = s == 0
    s[zero] = np.where(rng.rand(int(zero.sum())) < 0.5, -0.0, 0.0)      # mixed signed zeros: one tie group
    mask = np.zeros(C, bool)
    mask[rng.choice(C, rng.randint(1, C), replace=False)] = True
    return s, mask


def test_mirror_ap_against_sklearn_on_heavily_tied_rows():
    """bound 4 C 2^-53 absolute: sklearn's own rounding -- C thresholds, two roundings in each recall difference.  The mirror's value is
    the exact rational rounded once."""
    rng = np.random.RandomState(11)
    worst = 0.0
    for _ in range(300):
        C = rng.randint(2, 400)
        s, mask = tied_row(rng, C, rng.randint(1, 12))
        got = float(M.ap_exact(s, mask))
        want = average_precision_score(mask.astype(int), s)
        worst = max(worst, abs(got - want) / (4 * C * 2.0 ** -53))
        assert abs(got - want) <= 4 * C * 2.0 ** -53, (C, got, want)
    print(f"worst |mirror - sklearn| / bound: {worst:.3f}")


def _ordered_against_exact(s, mask):
    """-> |ap_ordered - ap_exact| over the bound (P + 3) 2^-53 ap: P - 1 additions of positive, correctly rounded terms in any order (each
    term one rounding, each addition one), and the final division"""
    P = int(mask.sum())
    exact = M.ap_exact(s, mask)
    got = M.ap_ordered_row(s, mask)
    bound = (P + 3) * 2.0 ** -53 * float(exact)
    assert abs(Fraction(got) - exact) <= Fraction(bound), (P, got, float(exact))
    return float(abs(Fraction(got) - exact)) / bound


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_mirror_ap_in_the_kernels_order_against_the_exact_value(P):
    """the ordered statement of AP (thread-serial, wave butterfly, four waves) across the wave's and the workgroup's thread counts, on
    heavily tied rows with both signed zeros and on a row without ties"""
    rng = np.random.RandomState(200 + P)
    worst = 0.0
    for levels in (1, 3, 12, 0):
        C = P + rng.randint(1, 2 * P + 40)
        s = rng.randint(-levels, levels + 1, C) * 0.5 if levels else rng.permutation(C) * 0.25 - 7.0
        zero = s == 0
        s[zero] = np.where(rng.rand(int(zero.sum())) < 0.5, -0.0, 0.0)
        mask = np.zeros(C, bool)
        mask[rng.choice(C, P, replace=False)] = True
        worst = max(worst, _ordered_against_exact(s, mask))
    print(f"P={P}: worst |ordered - exact| / ((P + 3) 2^-53 ap) = {worst:.3f}")


def test_mirror_ap_in_the_kernels_order_at_the_column_limit_with_mostly_positives():
    rng = np.random.RandomState(3)
    s = np.round(rng.randn(16384), 2)
    s[s == 0] = np.where(rng.rand(int((s == 0).sum())) < 0.5, -0.0, 0.0)
    assert np.any(np.signbit(s) & (s == 0)) and np.any(~np.signbit(s) & (s == 0))
    mask = np.zeros(16384, bool)
    mask[rng.choice(16384, 12000, replace=False)] = True
    print(f"C=16384, P=12000: |ordered - exact| / ((P + 3) 2^-53 ap) = {_ordered_against_exact(s, mask):.3f}")


def test_mirror_ap_in_the_kernels_order_by_hand():
    """P = 2 over three tie groups: thread 0 holds the upper positive, thread 1 the lower; the butterfly's last step adds lane 1 to lane 0"""
    s = np.array([1.0, 0.5, 0.25, 0.25])
    mask = np.array([True, False, True, False])
    assert M.ap_ordered_row(s, mask) == (1.0 / 1.0 + 2.0 / 4.0) / 2.0 == float(M.ap_exact(s, mask))
    tied = np.array([0.0, -0.0, 0.0, -1.0])                              # one group of two positives and a negative: one term, 2 * 2 / 3
    assert M.ap_ordered_row(tied, np.array([True, True, False, False])) == (4.0 / 3.0) / 2.0


def test_mirror_hits_on_tie_free_rows_is_the_argsort_count():
    rng = np.random.RandomState(12)
    for _ in range(100):
        C = rng.randint(2, 300)
        s = rng.permutation(C) * 0.25 - 7.0                              # distinct
        mask = np.zeros(C, bool)
        mask[rng.choice(C, rng.randint(1, C), replace=False)] = True
        order = np.argsort(-s, kind="stable")
        for k in (1, 2, C // 2 + 1, C - 1, C, C + 5):
            want = int(mask[order[:min(k, C)]].sum())
            got = M.hits_value(M.hits_parts(s, mask, k))
            assert got == want and M.hits_parts(s, mask, k)[3] == 1


def test_mirror_hits_on_tied_rows_is_the_average_over_every_tie_breaking_order():
    """a group of g <= 6 items straddles the cut: the mean, over all g! orders of the group, of the positives among the top k -- compared
    in exact rationals before the final rounding, then the contract's two fp64 operations on top"""
    rng = np.random.RandomState(13)
    straddled = 0
    for _ in range(200):
        g = rng.randint(2, 7)
        n_above, n_below = rng.randint(0, 6), rng.randint(0, 6)
        s = np.concatenate([3.0 + np.arange(n_above), np.zeros(g), -1.0 - np.arange(n_below)])
        s[n_above:n_above + g] = np.where(rng.rand(g) < 0.5, -0.0, 0.0)
        mask = rng.rand(len(s)) < 0.5
        if not mask.any() or mask.all():
            continue
        perm = rng.permutation(len(s))
        s, mask = s[perm], mask[perm]
        k = n_above + rng.randint(1, g + 1)
        A, pos_g, slots, size = M.hits_parts(s, mask, k)
        assert (slots, size) == (k - n_above, g)
        fixed = [i for i in np.argsort(-(s + 0.0), kind="stable") if s[i] > 0]
        group = [i for i in range(len(s)) if s[i] == 0]
        assert A == int(mask[fixed].sum()) and pos_g == int(mask[group].sum())
        total, orders = 0, 0
        for order in itertools.permutations(group):
            total += int(mask[fixed].sum()) + sum(int(mask[i]) for i in order[:slots])
            orders += 1
        assert Fraction(total, orders) == A + Fraction(pos_g * slots, size)
        want = float(A + pos_g) if slots == size else float(A) + float(pos_g * slots) / float(size)
        assert M.hits_value((A, pos_g, slots, size)) == want
        straddled += slots < size
    assert straddled >= 50


def test_mirror_one_class_rows_and_auc_column():
    s = np.array([[0.5, 0.25, 0.25, 1.0], [1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]])
    ptr, col = M.csr([[1, 3], [], [0, 1, 2, 3]])
    auc, ap, hits, n_pos, n_neg = M.mirror_metrics(s, ptr, col, (1, 3, 9))
    assert list(n_pos) == [2, 0, 4] and list(n_neg) == [2, 4, 0]
    assert np.isnan(auc[1:]).all() and np.isnan(ap[1:]).all() and np.isnan(hits[1:]).all()
    assert auc[0] == F.mirror_aucs(s, ptr, col)[0][0] == 0.625
    # ranks: 1.0 (+), 0.5 (-), then {0.25 (+), 0.25 (-)}: AP = (1/2) (1/1 + 2/4); hits@1 = 1, hits@3 = 1 + 1/2, hits@9 = hits@C = 2
    assert ap[0] == 0.75 and list(hits[0]) == [1.0, 1.5, 2.0]


@pytest.mark.parametrize("C", M.RANK_IDENTITY_WIDTHS)
def test_auc_is_the_positives_average_tie_ranks(C):
    """the rank mirror (profile_rank_mirror.mirror_rank) and the AUC mirror state one ordering: the identity of M.auc_from_ranks, bit for bit"""
    import profile_rank_mirror as PR
    s, rows = M.tied_rows(C)
    ptr, col = M.csr(rows)
    want, n_pos, n_neg = F.mirror_aucs(s, ptr, col)
    assert np.all(n_pos >= 1) and np.all(n_neg >= 1)
    got = np.array([M.auc_from_ranks(PR.mirror_rank(s[r]), rows[r]) for r in range(len(rows))])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)


def test_metric_name_parser():
    from gcn_drug_repurposing_amd import evaluate
    from gcn_drug_repurposing_amd.predict import PredictError
    assert evaluate.parse_metric("ap") == ("ap", None) and evaluate.parse_metric("auc") == ("auc", None)
    assert evaluate.parse_metric("recall@1") == ("recall", 1) and evaluate.parse_metric("recall@50") == ("recall", 50)
    assert evaluate.parse_metrics("ap,recall@50,recall@1") == ["ap", "recall@50", "recall@1"]
    assert evaluate.metric_cuts(["ap", "recall@50", "auc", "recall@1"]) == (50, 1)
    for bad in ("recall@0", "recall@x", "map", "recall@", "recall@-1", "recall@1.5", "AP", ""):
        with pytest.raises(PredictError, match="is unknown") as e:
            evaluate.parse_metric(bad)
        assert repr(bad) in str(e.value)
    with pytest.raises(PredictError, match="'ap' is given twice"):
        evaluate.parse_metrics("ap,recall@5,ap")
    with pytest.raises(PredictError, match="'recall@5' is given twice"):
        evaluate.parse_metrics(["recall@5", "recall@05"])
    eight = [f"recall@{k}" for k in range(1, 9)]
    assert evaluate.parse_metrics(["ap"] + eight) == ["ap"] + eight
    with pytest.raises(PredictError, match="9 distinct K"):
        evaluate.parse_metrics(eight + ["recall@9"])


def test_metric_arrays_divide_hits_by_the_positives():
    from gcn_drug_repurposing_amd import evaluate
    auc, ap = np.array([0.5, np.nan]), np.array([0.25, np.nan])
    hits = np.array([[1.5, 3.0], [np.nan, np.nan]])
    v = evaluate.metric_arrays(["recall@10", "ap", "recall@2", "auc"], (2, 10), auc, ap, hits, np.array([3, 0], np.int32))
    assert list(v) == ["recall@10", "ap", "recall@2", "auc"]
    assert v["recall@10"][0] == 3.0 / 3.0 and v["recall@2"][0] == 1.5 / 3.0 and v["ap"][0] == 0.25 and v["auc"][0] == 0.5
    assert all(np.isnan(a[1]) for a in v.values())
    assert evaluate.format_metric_line("recall@2", [0.5, 0.75, 1.0]) == "median recall@2: 0.75, mean recall@2: 0.75"


# ---- evaluate_auc.py --metrics with the mirror in place of the device --------------------------------------------------------------------

def _main(tmp_path, method, extra, **sources):
    """evaluate.main in this process -> (stdout, the --per-indication file's text)"""
    from gcn_drug_repurposing_amd import evaluate
    if method == "diffusion":
        F.stage_reference_profiles(tmp_path)
    cfg = F.stage(tmp_path, method)
    per = tmp_path / "per.tsv"
    out = io.StringIO()
    with redirect_stdout(out), redirect_stderr(io.StringIO()):
        evaluate.main(["-c", cfg, "--per-indication", str(per)] + extra, **sources)
    return out.getvalue(), per.read_text()


def _no_device(*a, **k):
    pytest.fail("the other source was called")


@pytest.mark.parametrize("method", ["node2vec", "gcn", "diffusion"])
def test_cli_with_metrics_on_the_fixture(tmp_path, method):
    from gcn_drug_repurposing_amd import evaluate
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    calls = []

    def source(scores, ptr, col, ks):
        calls.append(tuple(ks))
        return M.mirror_metrics(scores, ptr, col, ks)

    plain, plain_tsv = _main(tmp_path / "a", method, [], auc_source=F.mirror_aucs, metric_source=_no_device)
    out, tsv = _main(tmp_path / "b", method, ["--metrics", "ap,recall@5,recall@2"], auc_source=_no_device, metric_source=source)
    assert calls == [(5, 2)]
    # without --metrics: the reference's line alone and today's columns
    assert plain.count("\n") == 1 and F.LINE.match(plain.rstrip("\n"))
    F.check_line(plain.rstrip("\n"), method)
    assert plain_tsv.split("\n")[0] == "indication\tname\tpositives\tnegatives\tauc"
    # with it: the same line first, then one line per metric in the order given
    lines = out.split("\n")
    assert lines[0] + "\n" == plain and lines[-1] == "" and len(lines) == 5
    rows = [l.split("\t") for l in tsv.split("\n")[:-1]]
    assert rows[0] == ["indication", "name", "positives", "negatives", "auc", "ap", "recall@5", "recall@2"]
    assert ["\t".join(r[:5]) for r in rows] == plain_tsv.split("\n")[:-1]          # the first five columns are the run's without --metrics
    for j, name in enumerate(["ap", "recall@5", "recall@2"]):
        col = np.asarray([float(r[5 + j]) for r in rows[1:]])
        assert [repr(float(v)) for v in col] == [r[5 + j] for r in rows[1:]]
        assert lines[1 + j] == f"median {name}: {np.median(col)}, mean {name}: {col.mean()}" == evaluate.format_metric_line(name, col)
        assert np.all((col >= 0) & (col <= 1))
    # the columns are the mirror's on the scores that were ranked, indication by indication, and sklearn's
    s = evaluate.Settings(evaluate.load_config(str(tmp_path / "b" / "config.json")))
    res = evaluate.run(s, metrics=["ap", "recall@5", "recall@2"], metric_source=M.mirror_metrics, err=io.StringIO())
    assert res.metric_lines == lines[1:4] and res.line == lines[0] and list(res.metrics) == ["ap", "recall@5", "recall@2"]
    ptr, col_ = evaluate.label_rows(res.indications, res.drugs, evaluate.read_drug_indication_tsv(s.labels))[:2]
    scores = np.asarray(res.scores)
    for n, k in enumerate(res.kept):
        y = np.zeros(scores.shape[1], int)
        y[col_[ptr[k]:ptr[k + 1]]] = 1
        assert float(rows[1 + n][5]) == res.ap[k] == res.metrics["ap"][k]
        assert abs(res.ap[k] - average_precision_score(y, scores[k])) <= 4 * scores.shape[1] * 2.0 ** -53
        assert float(rows[1 + n][6]) == M.hits_value(M.hits_parts(scores[k], y.astype(bool), 5)) / y.sum()


def test_without_metrics_nothing_changes(tmp_path):
    """no --metrics: stdout and the TSV are, byte for byte, those of a run through the auc_source path, and metric_source is not called"""
    from gcn_drug_repurposing_amd import evaluate
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    out, tsv = _main(tmp_path / "a", "gcn", [], auc_source=F.mirror_aucs, metric_source=_no_device)
    s = evaluate.Settings(evaluate.load_config(F.stage(tmp_path / "b", "gcn")))
    res = evaluate.run(s, per_indication=str(tmp_path / "b" / "per.tsv"), auc_source=F.mirror_aucs, err=io.StringIO())
    assert out == res.line + "\n" and tsv == (tmp_path / "b" / "per.tsv").read_text()
    assert res.metric_lines == [] and res.metrics == {} and res.ap is None
    assert tsv.split("\n")[0] == "\t".join(evaluate.PER_INDICATION_HEADER)


def test_cli_refuses_a_bad_metric_by_name(tmp_path, capsys):
    from gcn_drug_repurposing_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["-c", F.stage(tmp_path, "gcn"), "--metrics", "ap,map"], auc_source=_no_device, metric_source=_no_device)
    assert e.value.code == 2 and "metric 'map' is unknown" in capsys.readouterr().err


def test_device_metrics_checks_come_before_the_gpu(monkeypatch):
    """the shape and cut-off checks are made on the host: loading the library is an error here"""
    from gcn_drug_repurposing_amd import _lib, evaluate
    from gcn_drug_repurposing_amd.predict import PredictError
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the refusal"))
    s = np.zeros((2, 5))
    with pytest.raises(PredictError, match="device_metrics: scores .* disagree"):
        evaluate.device_metrics(s, [0, 1], [0], (1,))
    with pytest.raises(PredictError, match="device_metrics: 9 cut-offs are above the limit of 8"):
        evaluate.device_metrics(s, [0, 1, 2], [0, 1], range(1, 10))
    with pytest.raises(PredictError, match="device_metrics: cut-off 0 is below 1"):
        evaluate.device_metrics(s, [0, 1, 2], [0, 1], (3, 0))
    with pytest.raises(PredictError, match="above the limit of 16384"):
        evaluate.device_metrics(np.zeros((1, 16385)), [0, 1], [0], ())


# ---- the trainer's flags -------------------------------------------------------------------------------------------------------------------

BASE = ["--beta-percentile", "98", "--hidden-units", "8", "--num-layers", "2", "--emb-file", "x"]


def test_trainer_flags_parse():
    from gcn_drug_repurposing_amd import trainer
    a = trainer.parse_args(BASE + ["--eval-config", "c.json", "--eval-metric", "recall@050", "--eval-stat", "mean"])
    assert (a.eval_metric, a.eval_stat) == ("recall@50", "mean")
    a = trainer.parse_args(BASE + ["--eval-config", "c.json"])
    assert (a.eval_metric, a.eval_stat) == ("auc", "median")
    assert trainer.eval_log_header("auc") == trainer.EVAL_LOG_HEADER == ["epoch", "median_auc", "mean_auc", "indications", "seconds"]
    assert trainer.eval_log_header("ap") == trainer.EVAL_LOG_HEADER + ["median_ap", "mean_ap"]


@pytest.mark.parametrize("extra, text", [
    (["--eval-metric", "ap"], "--eval-metric needs --eval-config"),
    (["--eval-stat", "mean"], "--eval-stat needs --eval-config"),
    (["--eval-config", "c.json", "--eval-metric", "map"], "metric 'map' is unknown"),
    (["--eval-config", "c.json", "--eval-metric", "recall@0"], "metric 'recall@0' is unknown"),
    (["--eval-config", "c.json", "--eval-metric", "ap,auc"], "metric 'ap,auc' is unknown"),
    (["--eval-config", "c.json", "--eval-stat", "max"], "invalid choice: 'max'"),
])
def test_trainer_flag_refusals(extra, text, capsys):
    from gcn_drug_repurposing_amd import trainer
    with pytest.raises(SystemExit) as e:
        trainer.main(BASE + extra)
    assert e.value.code == 2 and text in capsys.readouterr().err


def test_an_eval_log_with_another_header_is_refused_before_the_gpu_check(tmp_path, capsys, monkeypatch):
    import torch
    from test_train_eval import _config
    from gcn_drug_repurposing_amd import trainer
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("GSS_FORCE_SHARDED", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU check ran before the refusal"))
    log = tmp_path / "log.tsv"
    log.write_text("\t".join(trainer.EVAL_LOG_HEADER) + "\n1\t0.5\t0.5\t20\t0.01\n")
    args = ["--beta-percentile", "98", "--hidden-units", "8", "--num-layers", "2", "--emb-file", os.path.join(F.D, "n2v.embs.txt"),
            "--adj-file", os.path.join(F.D, "eval.weighted.edgelist"), "--eval-config", _config(tmp_path), "--eval-log", str(log)]
    with pytest.raises(SystemExit) as e:
        trainer.main(args + ["--eval-metric", "ap"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "log.tsv exists with the header" in err and "median_ap" in err and "--eval-metric ap" in err
    log.write_text("\t".join(trainer.eval_log_header("ap")) + "\n")
    with pytest.raises(SystemExit) as e:
        trainer.main(args)                                               # and the other way round
    assert e.value.code == 2 and "--eval-metric auc" in capsys.readouterr().err
