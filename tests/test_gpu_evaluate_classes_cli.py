"""GPU: evaluate_auc.py --by-class on the small fixture (tests/golden/evaluate_msi_small: 12 drugs) under diffusion, diffusion with
diffusion.compare set (device scores) and gcn, the class table written by test_rank_strata.py's write_table.  The strata source is
evaluate.device_metrics_strata itself, wrapped only to keep what it was given: from those scores and lists every stratum is recomputed
through the host mirror (rank_strata_mirror.py) -- auc and recall@K as text, ap within (|Q| + 3) 2^-53 relative -- and every cell of the
per-class table from the per-stratum table's own columns with np.median and ndarray.mean."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import evaluate_fixture as F  # noqa: E402
import rank_strata_mirror as RS  # noqa: E402
from test_rank_strata import MEMBERS, METRICS, read_table, write_table  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["diffusion", "diffusion-correlation", "gcn"])
def test_by_class_tables_are_the_mirrors_on_the_programs_own_scores(tmp_path, monkeypatch, case):
    from gcn_drug_repurposing_amd import evaluate
    method = case.split("-")[0]
    over = {"diffusion": {"eval_diffusion_embs_dir": str(tmp_path / "dp"), "compare": "correlation"}} if case.endswith("correlation") else {}
    cfg = F.stage(tmp_path, method, **over)
    table = write_table(tmp_path / "atc.tsv")
    given = []

    def source(*args):
        given.append(args)
        return evaluate.device_metrics_strata(*args)

    monkeypatch.chdir(tmp_path)
    out = io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
        evaluate.main(["-c", cfg, "--metrics", ",".join(METRICS), "--per-indication", "per.tsv", "--by-class", table, "--per-stratum", "strata.tsv",
                       "--class-levels", "1,2"], strata_source=source)
    lines = out.getvalue().split("\n")
    assert len(given) == 1 and len(lines) == 3 + len(METRICS) and lines[-1] == ""
    scores, ptr, col, sp, qp, qc, ks = given[0]
    assert tuple(ks) == (3, 1)
    if case == "diffusion-correlation":
        import torch
        assert isinstance(scores, torch.Tensor) and scores.is_cuda
    auc, ap, hits, s_pos, n_pos, n_neg = RS.mirror_strata(scores, ptr, col, sp, qp, qc, ks)
    S = len(s_pos)
    per = read_table(tmp_path / "per.tsv")
    kept = [k for k in range(len(n_pos)) if n_pos[k] > 0 and n_neg[k] > 0]
    assert [int(r[2]) for r in per[1:]] == [int(n_pos[k]) for k in kept] and all(sp[k + 1] == sp[k] for k in range(len(n_pos)) if k not in kept)

    # the long table: one row per stratum, in indication order, then level and code
    strata = read_table(tmp_path / "strata.tsv")
    assert strata[0] == ["level", "class", "indication", "name", "positives", "negatives", "auc"] + METRICS and len(strata) == 1 + S and S > 20
    owner = [r for r in range(len(n_pos)) for _ in range(sp[r], sp[r + 1])]
    inds = [r[0] for r in per[1:]]
    drugs_of = {}                                                                  # (level, code) -> the class's drug columns, from the strata themselves
    for s, row in enumerate(strata[1:]):
        level, code = int(row[0]), row[1]
        assert row[2] == inds[kept.index(owner[s])] and row[3] == "n_" + row[2]
        assert (int(row[4]), int(row[5])) == (int(s_pos[s]), int(n_neg[owner[s]])) and s_pos[s] > 0
        assert row[6] == repr(float(auc[s])), (s, row[6], auc[s])
        assert abs(float(row[7]) - ap[s]) <= (int(s_pos[s]) + 3) * 2.0 ** -53 * ap[s], (s, row[7], ap[s])
        assert row[8] == repr(float(hits[s, 0] / s_pos[s])) and row[9] == repr(float(hits[s, 1] / s_pos[s]))
        drugs_of.setdefault((level, code), set()).update(int(c) for c in qc[qp[s]:qp[s + 1]])
    keys = [(int(r[0]), r[1], r[2]) for r in strata[1:]]
    assert [(inds.index(k[2]), k[0], k[1]) for k in keys] == sorted((inds.index(k[2]), k[0], k[1]) for k in keys) and len(set(keys)) == S

    # the per-class table from the long table's own columns
    got = read_table(tmp_path / "class_metrics.tsv")
    assert got[0][:6] == ["level", "class", "class_name", "drugs", "indications", "positives"]
    assert got[0][6:] == [f"{stat}_{m}" for m in ["auc"] + METRICS for stat in ("median", "mean")]
    assert [(int(r[0]), r[1]) for r in got[1:]] == sorted(drugs_of)
    for r in got[1:]:
        mine = [x for x in strata[1:] if (x[0], x[1]) == (r[0], r[1])]
        assert r[2] == "the " + r[1] + " drugs" and int(r[3]) == len(MEMBERS[int(r[0])][r[1]]) >= len(drugs_of[(int(r[0]), r[1])])
        assert (int(r[4]), int(r[5])) == (len(mine), sum(int(x[4]) for x in mine))
        for j in range(1 + len(METRICS)):
            v = np.asarray([float(x[6 + j]) for x in mine], np.float64)
            assert r[6 + 2 * j:8 + 2 * j] == [repr(float(np.median(v))), repr(float(v.mean()))], (r[:2], j)
    assert lines[-2] == f"classes: {len(got) - 1} classes of levels 1,2 over {S} (indication, class) pairs: class_metrics.tsv"
    assert lines[0].startswith("median auc: ") and [l.split(":")[0] for l in lines[1:1 + len(METRICS)]] == ["median " + m for m in METRICS]
