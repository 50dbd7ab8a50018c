"""GPU: gss_embedding_scores (csrc/scores.hip) bit for bit against its numpy mirror (embedding_scores_mirror.py), its refusals,
evaluate.DeviceEvaluator against the reference's recorded AUCs, and train.py --eval-config: the eval line of epoch e is what
evaluate_auc.py says about the graph_embs.txt of a run with --epochs e, the trajectory is untouched, --keep-best / --patience do what the
log predicts, the single-GPU shard path evaluates in node order and sharded runs are refused."""
import contextlib
import io
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import embedding_scores_mirror as M  # noqa: E402
import evaluate_fixture as F  # noqa: E402
from test_train_eval import GAP, _config, close_pairs, fixture_embeddings, fixture_lists  # noqa: E402

pytestmark = pytest.mark.gpu

EVAL_LINE = re.compile(r"^eval (\d+) (median auc: \S+, mean auc: \S+)$")
NEW_KEYS = {"eval_best_median", "eval_best_epoch", "eval_stale"}


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------

def _call(x, d, rows, cols, normalize, ld_out=None, n=None, ld=None, emb_ptr=None, out_ptr=None, rows_ptr=None, cols_ptr=None, nr=None, nc=None):
    """-> (rc, out [nr, nc] host fp64, error text); x: device fp32 [n, ld]"""
    import torch
    from gcn_drug_repurposing_amd import _lib
    lib = _lib.load()
    dr = torch.as_tensor(np.asarray(rows, np.int32)).cuda()
    dc = torch.as_tensor(np.asarray(cols, np.int32)).cuda()
    nr, nc = len(rows) if nr is None else nr, len(cols) if nc is None else nc
    ldo = max(nc, 1) if ld_out is None else ld_out
    out = torch.full((max(nr, 1), max(ldo, 1)), 7.0, dtype=torch.float64, device="cuda")
    rc = lib.gss_embedding_scores(x.shape[0] if n is None else n, d, _lib.ptr(x) if emb_ptr is None else emb_ptr,
                                  x.stride(0) if ld is None else ld, nr, _lib.ptr(dr) if rows_ptr is None else rows_ptr, nc,
                                  _lib.ptr(dc) if cols_ptr is None else cols_ptr, normalize, _lib.ptr(out) if out_ptr is None else out_ptr,
                                  ldo, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[:nr, :nc], lib.gss_last_error().decode()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("case, normalize", [("gcn", 1), ("gcn", 0), ("node2vec", 0), ("node2vec", 1)])
def test_kernel_is_bit_equal_to_the_mirror_on_the_fixture(case, normalize):
    import torch
    names, x32 = fixture_embeddings(case)
    _, _, rows, cols, _, _ = fixture_lists(names)
    padded = np.concatenate([x32, np.zeros((len(names), 8), np.float32)], axis=1)      # the plan's tensor: d = 8 padded to 16
    for d in (8, 16):
        rc, got, err = _call(torch.from_numpy(padded).cuda(), d, rows, cols, normalize)
        assert rc == 0, err
        assert np.array_equal(_bits(got), _bits(M.scores(x32, 8, rows, cols, normalize)))   # the zero padding changes no bit


@pytest.mark.parametrize("d", [8, 48, 128, 256])
def test_kernel_is_bit_equal_to_the_mirror_on_random_matrices(d):
    import torch
    rng = np.random.RandomState(d)
    n, ld = 300, d + 5
    x = (rng.randn(n, ld) * np.exp(rng.randn(n, 1))).astype(np.float32)
    x[17] = 0                                                      # a zero row: its norm divides by 1
    x[:, d:] = 99.0                                                # ld > d: what lies behind d is never read into a sum
    rows = np.concatenate([[17, 5, 5, 299, 0], rng.randint(0, n, 70)])         # repeated and unordered
    cols = np.concatenate([rng.permutation(n)[:130], [17, 5]])
    dx = torch.from_numpy(x).cuda()
    for normalize in (0, 1):
        want = M.scores(x, d, rows, cols, normalize)
        rc, got, err = _call(dx, d, rows, cols, normalize, ld_out=len(cols) + 3)
        assert rc == 0, err
        assert np.array_equal(_bits(got), _bits(want)), (d, normalize, np.abs(got - want).max())
        assert np.all(got[0] == 0) and np.all(got[:, 130] == 0)
        rc, again, _ = _call(dx, d, rows, cols, normalize)
        assert np.array_equal(_bits(again), _bits(got))            # run to run
        rc, swapped, err = _call(dx, d, cols, rows, normalize)
        assert rc == 0 and np.array_equal(_bits(swapped), _bits(got.T))        # rows and columns swapped: the transposed result
        rc, sub, err = _call(dx, d, rows[3:9], cols[60:131], normalize)
        assert rc == 0 and np.array_equal(_bits(sub), _bits(got[3:9, 60:131]))  # a sub-list gives equal bits
        rc, one, err = _call(dx, d, rows[40:41], cols[7:8], normalize)
        assert rc == 0 and np.array_equal(_bits(one), _bits(got[40:41, 7:8]))


def test_kernel_refusals():
    import torch
    from gcn_drug_repurposing_amd import _lib
    rng = np.random.RandomState(1)
    x = torch.from_numpy(rng.randn(50, 24).astype(np.float32)).cuda()
    rows, cols = [1, 2, 3], [4, 5, 6, 7]
    for kw, text in [({"emb_ptr": 0}, "emb is null"), ({"rows_ptr": 0}, "rows is null"), ({"cols_ptr": 0}, "cols is null"),
                     ({"out_ptr": 0}, "out is null"), ({"ld": 15}, "ld=15 is below d=16"), ({"ld_out": 3}, "ld_out=3 is below nc=4")]:
        rc, _, err = _call(x, 16, rows, cols, 1, **kw)
        assert rc == -22 and text in err, (kw, err)
    rc, _, err = _call(x, 16, rows, cols, 1, nr=0)
    assert rc == -22 and "nr=0 rows must be >= 1" in err, err
    rc, _, err = _call(x, 16, rows, cols, 1, nc=-1)
    assert rc == -22 and "nc=-1 cols must be >= 1" in err, err
    # an index outside [0, n): named by list and position; the row is never read
    rc, _, err = _call(x, 16, [1, 50, 3, -2], cols, 1)
    assert rc == -22 and "rows[1] = 50 is not a row index in [0, 50)" in err, err
    rc, _, err = _call(x, 16, rows, [4, 5, -1, 7], 0)
    assert rc == -22 and "cols[2] = -1 is not a row index in [0, 50)" in err, err
    # a NaN / an infinity planted in a listed row: named by row; in a row no list names it is not looked at
    bad = x.clone()
    bad[6, 3] = float("nan")
    rc, _, err = _call(bad, 16, rows, cols, 1)
    assert rc == -22 and "row 6 of emb holds a NaN or infinite value" in err, err
    bad = x.clone()
    bad[2, 15] = float("inf")
    bad[40, 0] = float("nan")
    bad[1, 20] = float("nan")                                      # behind d
    rc, _, err = _call(bad, 16, rows, cols, 0)
    assert rc == -22 and "row 2 of emb holds a NaN or infinite value" in err, err
    rc, _, err = _call(bad, 16, [1, 3], cols, 0)
    assert rc == 0, err


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------------

def _fixture_evaluator(names, **kw):
    from gcn_drug_repurposing_amd import evaluate
    return evaluate.DeviceEvaluator(os.path.join(F.TABLES_DIR, "protein_to_protein.tsv"), os.path.join(F.D, "drug_indication_df.tsv"), names, **kw)


@pytest.mark.parametrize("case", ["gcn", "node2vec"])
def test_evaluator_reproduces_the_recorded_aucs(case):
    import torch
    names, x32 = fixture_embeddings(case)
    ev = _fixture_evaluator(names, normalize=case == "gcn")
    padded = np.concatenate([x32, np.zeros((len(names), 8), np.float32)], axis=1)
    for emb, d in ((torch.from_numpy(padded).cuda(), 8), (torch.from_numpy(padded).cuda(), None), (torch.from_numpy(x32).cuda(), None)):
        res = ev.score(emb, d)
        assert not any(res.skipped.values()) and res.unknown_pairs == 0
        F.check_aucs([res.indications[k] for k in res.kept], res.auc[res.kept], case)
        F.check_line(res.line, case)
        assert res.scores.is_cuda and res.scores.shape == (len(ev.indications), len(ev.drugs))
    from gcn_drug_repurposing_amd.predict import PredictError
    with pytest.raises(PredictError, match="dtype torch.float64"):
        ev.score(torch.from_numpy(x32).cuda().double())
    with pytest.raises(PredictError, match="the name list has 111 rows"):
        ev.score(torch.from_numpy(x32[:100]).cuda())
    with pytest.raises(PredictError, match="not on the GPU"):
        ev.score(torch.from_numpy(x32))


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------

def _train(args):
    """trainer.main in this process -> (engine, stdout, stderr)"""
    from gcn_drug_repurposing_amd import trainer
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        engine = trainer.main(args)
    return engine, out.getvalue(), err.getvalue()


def _flags(epochs, lr=None):
    flags = ["--emb-file", os.path.join(F.D, "n2v.embs.txt"), "--adj-file", os.path.join(F.D, "eval.weighted.edgelist"), "--hidden-units", "8",
             "--num-layers", "2", "--seed", "7", "--batch-size", "32", "--epochs", str(epochs), "--beta-percentile", "98"]
    return flags + (["--lr", str(lr)] if lr is not None else [])


def _eval_lines(stdout):
    lines = stdout.split("\n")
    found = {}
    for k, line in enumerate(lines):
        m = EVAL_LINE.match(line)
        if m:
            assert lines[k - 1].startswith(f"iter {m.group(1)}")       # right after the unchanged iter line
            found[int(m.group(1))] = m.group(2)
    return found


def _read_log(path):
    lines = open(path).read().split("\n")
    assert lines[0] == "epoch\tmedian_auc\tmean_auc\tindications\tseconds" and lines[-1] == ""
    return [(int(r[0]), float(r[1]), float(r[2]), int(r[3]), float(r[4])) for r in (l.split("\t") for l in lines[1:-1])]


class Runs:
    """the runs the trainer tests share, made on first use: plain(e) = --epochs e without an eval flag, evaluated(e) = the same with
    --eval-config --eval-every 1 (+ --eval-log, --keep-best); both write --out and --checkpoint"""

    def __init__(self, tmp, lr=None):
        self.tmp, self.lr, self.cache = tmp, lr, {}
        self.config = _config(tmp)

    def _run(self, kind, e, extra=()):
        key = (kind, e) + tuple(extra)
        if key not in self.cache:
            stem = os.path.join(str(self.tmp), "_".join(str(k).strip("-") for k in key))
            args = _flags(e, self.lr) + ["--out", stem + ".txt", "--checkpoint", stem + ".npz"] + list(extra)
            if kind == "eval":
                args += ["--eval-config", self.config, "--eval-every", "1", "--eval-log", stem + ".log.tsv", "--keep-best", stem + ".best.txt"]
            engine, out, err = _train(args)
            self.cache[key] = {"stem": stem, "out": stem + ".txt", "ckpt": stem + ".npz", "log": stem + ".log.tsv", "best": stem + ".best.txt",
                               "stdout": out, "stderr": err, "emb": engine.gather_embeddings().clone()}
        return self.cache[key]

    def plain(self, e):
        return self._run("plain", e)

    def evaluated(self, e, extra=()):
        return self._run("eval", e, extra)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("train_eval"))


@pytest.fixture(scope="module")
def fast_runs(tmp_path_factory):
    return Runs(tmp_path_factory.mktemp("train_eval_fast"), lr=0.02)       # a learning rate at which the median moves between epochs


def _evaluate_auc(tmp, gcn_file):
    """evaluate_auc.py's run on a graph_embs.txt (host scores, device AUC kernel) -> (Result, the indications and AUCs of its
    --per-indication file)"""
    from gcn_drug_repurposing_amd import evaluate
    os.makedirs(str(tmp), exist_ok=True)
    cfg = F.stage(tmp, "gcn", gcn={"embs": "node2vec", "emb_file": gcn_file})
    per = os.path.join(str(tmp), "per.tsv")
    res = evaluate.run(evaluate.Settings(evaluate.load_config(cfg)), per_indication=per, err=io.StringIO())
    inds, aucs, _ = F.read_per_indication(per)
    return res, inds, np.asarray(aucs)


def test_eval_line_is_what_evaluate_auc_says_about_a_run_of_that_many_epochs(runs, tmp_path):
    """the defining property, for e = 1..4.  The AUCs of the two sides agree within 1e-12, except where the host scores of an indication
    hold a listed / unlisted pair closer than 1e-9 and not equal: such an indication may differ by 1 / (P N) per such pair; at most 5 % of
    the indications may be exempted that way."""
    names, _ = fixture_embeddings("gcn")
    ev = _fixture_evaluator(names)
    long = runs.evaluated(4)
    lines = _eval_lines(long["stdout"])
    assert sorted(lines) == [1, 2, 3, 4]
    log = _read_log(long["log"])
    assert [r[0] for r in log] == [1, 2, 3, 4]
    exempted_total = 0
    for e in range(1, 5):
        host, host_inds, host_aucs = _evaluate_auc(tmp_path / f"host{e}", runs.plain(e)["out"])
        # the trainer's side, per indication: the evaluator on the tensor a run of e epochs ends with -- the same bits the eval line of
        # epoch e of the long run was made from (that run's own last eval line says so too)
        res = ev.score(runs.evaluated(e)["emb"], 8)
        assert lines[e] == res.line == _eval_lines(runs.evaluated(e)["stdout"])[e]
        assert [res.indications[k] for k in res.kept] == host_inds
        assert np.array_equal(res.n_pos, host.n_pos) and np.array_equal(res.n_neg, host.n_neg)
        ptr, col = ev.pos_ptr, ev.pos_col
        close = close_pairs(np.asarray(host.scores), ptr, col)
        diff = np.abs(res.auc[res.kept] - host_aucs)
        exempt = 0
        for k, dk in zip(res.kept, diff):
            bound = 1e-12 + close[k] / (float(res.n_pos[k]) * float(res.n_neg[k]))
            exempt += close[k] > 0
            assert dk <= bound, (e, res.indications[k], dk, close[k])
        print(f"epoch {e}: {exempt} of {len(res.kept)} indications exempted (a listed / unlisted pair of host scores within {GAP}); "
              f"max |auc difference| {diff.max():.3e}")
        assert exempt <= 0.05 * len(res.kept)
        exempted_total += exempt
        if exempt == 0:
            got, want = F.LINE.match(res.line), F.LINE.match(host.line)
            assert all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(got.groups(), want.groups())), (res.line, host.line)
        assert log[e - 1][1:4] == (float(np.median(res.auc[res.kept])), float(res.auc[res.kept].mean()), len(res.kept))
    print(f"exempted in all: {exempted_total}")


def test_trajectory_is_untouched(runs):
    """with and without --eval-config: the same --out and the same checkpoint after every epoch, byte for byte, apart from the new keys"""
    for e in range(1, 5):
        a, b = runs.plain(e), runs.evaluated(e)
        assert open(a["out"], "rb").read() == open(b["out"], "rb").read()
        za, zb = np.load(a["ckpt"]), np.load(b["ckpt"])
        assert set(zb.files) - set(za.files) == NEW_KEYS and set(za.files) <= set(zb.files) and not NEW_KEYS & set(za.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), (e, k)
        assert int(zb["eval_best_epoch"]) >= 1 and float(zb["eval_best_median"]) == max(r[1] for r in _read_log(b["log"]))
        assert not any(l.startswith("eval") for l in a["stdout"].split("\n")) and not os.path.exists(a["log"]) and not os.path.exists(a["best"])


def test_keep_best_holds_the_first_epoch_with_the_highest_median(runs, fast_runs):
    for r in (runs, fast_runs):
        long = r.evaluated(4)
        medians = [row[1] for row in _read_log(long["log"])]
        best = 1 + int(np.argmax(medians))                          # argmax: the first of equal maxima
        print(f"lr {r.lr}: medians {medians}, best epoch {best}")
        assert open(long["best"], "rb").read() == open(r.plain(best)["out"], "rb").read()
        assert open(long["out"], "rb").read() == open(r.plain(4)["out"], "rb").read()     # --out still gets the last epoch


def test_patience_stops_where_the_log_predicts(fast_runs):
    medians = [row[1] for row in _read_log(fast_runs.evaluated(4)["log"])]
    stop = next((e for e in range(2, 5) if medians[e - 1] <= max(medians[:e - 1])), None)   # the first epoch without a strict improvement
    run = fast_runs.evaluated(4, ("--patience", "1"))
    evals = sorted(_eval_lines(run["stdout"]))
    if stop is None or stop == 4:
        assert evals == [1, 2, 3, 4] and "early stop" not in run["stdout"]
    else:
        assert evals == list(range(1, stop + 1)) and run["stdout"].rstrip("\n").split("\n")[-1] == f"early stop at iter {stop}"
    last = evals[-1]
    assert open(run["out"], "rb").read() == open(fast_runs.plain(last)["out"], "rb").read()   # --out: that epoch's embeddings
    assert [row[0] for row in _read_log(run["log"])] == evals


def test_resume_continues_the_best_so_far(fast_runs, tmp_path):
    import shutil
    two = fast_runs.evaluated(2)
    ckpt = str(tmp_path / "resume.npz")
    shutil.copy(two["ckpt"], ckpt)
    _, out, _ = _train(_flags(4, fast_runs.lr) + ["--out", str(tmp_path / "out.txt"), "--checkpoint", ckpt, "--resume", ckpt, "--eval-config",
                                                fast_runs.config, "--eval-log", str(tmp_path / "log.tsv")])
    long = fast_runs.evaluated(4)
    assert _eval_lines(out) == {e: line for e, line in _eval_lines(long["stdout"]).items() if e > 2}
    z, zl = np.load(ckpt), np.load(long["ckpt"])
    assert all(z[k].tobytes() == zl[k].tobytes() for k in NEW_KEYS)
    assert (tmp_path / "out.txt").read_bytes() == open(long["out"], "rb").read()
    # a checkpoint from before the keys existed loads as before
    z2 = np.load(two["ckpt"])
    old = {k: z2[k] for k in z2.files if k not in NEW_KEYS}
    np.savez(str(tmp_path / "old.npz"), **old)
    _, out, _ = _train(_flags(3, fast_runs.lr) + ["--out", str(tmp_path / "out3.txt"), "--resume", str(tmp_path / "old.npz"), "--eval-config",
                                                fast_runs.config])
    assert sorted(_eval_lines(out)) == [3]


def test_sharded_runs_refuse_eval_config(runs, monkeypatch, capsys):
    from gcn_drug_repurposing_amd import trainer
    monkeypatch.setenv("GSS_FORCE_SHARDED", "1")
    with pytest.raises(SystemExit) as e:
        trainer.main(_flags(1) + ["--eval-config", runs.config])
    assert e.value.code == 2 and "--eval-config is not supported on sharded runs" in capsys.readouterr().err


def test_shard_path_evaluates_in_node_order(tmp_path):
    """n >= RELABEL_MIN_NODES: the single-GPU run goes through the shard builder with its hub-first relabelling; the eval line is
    consumer.indication_aucs on the gathered embeddings (the tolerance of test_full_size_equals_consumer_indication_aucs)"""
    from test_gpu_evaluate import _standin
    from gcn_drug_repurposing_amd import consumer, embio, evaluate
    from gcn_drug_repurposing_amd.msi import COMPONENTS, MsiGraph
    from gcn_drug_repurposing_amd.shards import RELABEL_MIN_NODES
    data, labels = _standin(tmp_path)
    g = MsiGraph().load({name: os.path.join(data, name + ".tsv") for name, _, _ in COMPONENTS})
    names, d = g.names, 16
    assert len(names) >= RELABEL_MIN_NODES
    rng = np.random.RandomState(5)
    order = rng.permutation(len(names))
    x = rng.randn(len(names), d) / 4
    emb_file = tmp_path / "standin.embs.txt"
    with open(emb_file, "w") as f:
        f.write(f"{len(names)} {d}\n")
        f.writelines(names[i] + " " + " ".join(repr(float(v)) for v in x[i]) + "\n" for i in order)
    config = tmp_path / "eval.json"
    config.write_text(json.dumps({"networks": {"protein_to_protein": os.path.join(data, "protein_to_protein.tsv"), "drug_to_indication": labels}}))
    engine, out, err = _train(["--emb-file", str(emb_file), "--hidden-units", str(d), "--num-layers", "2", "--seed", "7", "--batch-size", "2048",
                               "--epochs", "2", "--beta-percentile", "98", "--k", "5", "--out", str(tmp_path / "out.txt"), "--eval-config",
                               str(config), "--eval-every", "2"])
    assert engine.node_map is not None                                  # the relabelled path
    lines = _eval_lines(out)
    assert sorted(lines) == [2]
    assert "skipped 1 of 841 indications" in err and err.count("skipped") == 1
    file_names = [names[i] for i in order]
    drugs = [n for n in names if g.type[n] == "drug"]
    inds = [n for n in names if g.type[n] == "indication"]
    emb = engine.gather_embeddings().cpu().numpy()[:, :d].astype(np.float64)
    want, used = consumer.indication_aucs(emb, file_names, drugs, inds, consumer.read_drug_indication_tsv(labels))
    assert len(used) == 840
    names_file, _ = embio.read_embs(str(emb_file))
    res = evaluate.DeviceEvaluator(os.path.join(data, "protein_to_protein.tsv"), labels, names_file).score(engine.gather_embeddings(), d)
    assert [res.indications[k] for k in res.kept] == used and res.line == lines[2]
    assert np.max(np.abs(res.auc[res.kept] - want)) <= 1e-12               # indication by indication: the rows are in node order
    got, ref = F.LINE.match(lines[2]), F.LINE.match(evaluate.format_line(want))
    assert all(abs(float(a) - float(b)) <= 1e-12 for a, b in zip(got.groups(), ref.groups())), (lines[2], evaluate.format_line(want))
