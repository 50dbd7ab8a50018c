"""GPU: the "spearman" profile distance = gss_profile_rank followed by the correlation distance.  Because the ranks are exact, the composed
distance is held bit for bit to the correlation kernels run on scipy's ranks, and within the project's derived bound (profile_dist_mirror.py:
8 gamma(n + 8) absolute, for inputs that pass check_spread) to scipy's cdist on those ranks; then the programs end to end on the SAVED
reference profiles of the small fixture.  Saved, not device-made: a rank is discontinuous, so two entries of a profile that differ by less
than the device profiles' 1e-13 may swap ranks, and expectations here are formed from the very vectors the run used."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist, correlation
from scipy.stats import rankdata, spearmanr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_fixture as EF  # noqa: E402
import predict_fixture as PF  # noqa: E402
import profile_dist_mirror as M  # noqa: E402
from conftest import record_measured  # noqa: E402

from gcn_drug_repurposing_amd.diffusion import compare_profile_pairs, compare_profiles  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def scipy_corr(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return cdist(a, b, "correlation")


def scipy_corr_pairs(r, ca, cb):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray([correlation(r[a], r[b]) for a, b in zip(ca, cb)])


@pytest.mark.parametrize("n", [111, 1000, 29960])
@pytest.mark.parametrize("shape", [(1, 1), (17, 300), (128, 128)])
def test_against_correlation_of_scipys_ranks(n, shape):
    na, nb = shape
    p = M.synthetic(n + 7 * na + nb, na + nb, n, lognormal=(n == 1000))
    assert (p == 0).mean() > 0.05                                              # heavy ties: a tenth of every profile is exactly 0
    r = rankdata(p, axis=1)
    M.check_spread(r)
    a, b = np.arange(na), np.arange(na, na + nb)
    x = torch.from_numpy(p).cuda().t().contiguous()
    got = compare_profiles(x, a, b, "spearman").cpu().numpy()
    assert np.array_equal(bits(got), bits(compare_profiles(r, a, b, "correlation").cpu().numpy()))   # exact ranks: the same bits
    assert np.array_equal(bits(got), bits(compare_profiles(p, a, b, "spearman").cpu().numpy()))      # host [K][N] input
    worst = M.compare(got, scipy_corr(r[a], r[b]), "correlation", n)
    record_measured(f"spearman.synthetic.n{n}.{na}x{nb}", worst_in_bounds=worst)
    print(n, shape, "worst / bound", worst)
    rho = spearmanr(p[0], p[na]).correlation
    assert abs(got[0, 0] - (1.0 - rho)) <= M.dot_abs_bound(n)


@pytest.mark.parametrize("T", [1, 65, 1000])
def test_pairs(T):
    n, k = 1000, 40
    p = M.synthetic(3 + T, k, n, lognormal=True)
    r = rankdata(p, axis=1)
    M.check_spread(r)
    rng = np.random.RandomState(T)
    ca, cb = rng.randint(0, k, size=T), rng.randint(0, k, size=T)
    if T > 1:
        ca[-1], cb[-1] = ca[0], cb[0]                                          # a repeated pair
        ca[1], cb[1] = cb[0], ca[0]                                            # and the pair the other way round
    x = torch.from_numpy(p).cuda().t().contiguous()
    got = compare_profile_pairs(x, ca, cb, "spearman").cpu().numpy()
    assert got.shape == (T,)
    assert np.array_equal(bits(got), bits(compare_profile_pairs(r, ca, cb, "correlation").cpu().numpy()))
    worst = M.compare(got, scipy_corr_pairs(r, ca, cb), "correlation", n)
    record_measured(f"spearman.pairs.T{T}", worst_in_bounds=worst)
    if T > 1:
        assert bits(got)[-1] == bits(got)[0] == bits(got)[1]
    rho = spearmanr(p[ca[0]], p[cb[0]]).correlation
    assert abs(got[0] - (1.0 - rho)) <= M.dot_abs_bound(n)


def test_degenerate_profiles_give_nan_in_exactly_their_rows_and_columns():
    n, k = 500, 9
    p = M.synthetic(17, k, n)
    p[2] = 0.125                                                               # constant: every rank (n + 1) / 2
    p[6, 77] = np.nan                                                          # a NaN: every rank NaN
    got = compare_profiles(p, None, None, "spearman").cpu().numpy()
    bad = np.zeros((k, k), bool)
    bad[[2, 6]] = True
    bad[:, [2, 6]] = True
    assert np.array_equal(np.isnan(got), bad)
    keep = [0, 1, 3, 4, 5, 7, 8]
    r = rankdata(p[keep], axis=1)
    M.compare(got[np.ix_(keep, keep)], scipy_corr(r, r), "correlation", n)
    pairs = compare_profile_pairs(p, [0, 2, 6, 3, 2], [1, 0, 3, 6, 6], "spearman").cpu().numpy()
    assert np.array_equal(np.isnan(pairs), [False, True, True, True, True])


def test_symmetry_bit_for_bit():
    p = M.synthetic(7, 450, 1000)
    x = torch.from_numpy(p).cuda().t().contiguous()
    a, b = np.arange(300), np.random.RandomState(1).permutation(450)[:300]
    ab, again, ba = (compare_profiles(x, u, v, "spearman").cpu().numpy() for u, v in ((a, b), (a, b), (b, a)))
    assert not np.isnan(ab).any()
    assert np.array_equal(bits(ab), bits(again)) and np.array_equal(bits(ab), bits(ba.T))
    one = compare_profiles(x, [a[137]], [b[64]], "spearman").cpu().numpy()   # a pair alone == the pair inside the 300 x 300 call
    assert bits(one)[0, 0] == bits(ab)[137, 64]


# ---- the programs on the saved reference profiles of the small fixture ---------------------------------------------------------------------

def stage_saved_profiles(tmp):
    """a profile directory holding the reference's 21 vectors and node order (tests/golden/diffusion_msi_small.npz), as the programs save
    them -> (path, the profiles' names, their ranks [21][111] by scipy, the node order)"""
    z = np.load(os.path.join(HERE, "golden", "diffusion_msi_small.npz"))
    d = os.path.join(str(tmp), "dp")
    os.makedirs(d)
    with open(os.path.join(d, "node2idx.pkl"), "wb") as f:
        pickle.dump({str(n): i for i, n in enumerate(z["nodelist"])}, f)
    names = [str(s) for s in z["starts"]]
    for s, p in zip(names, np.asarray(z["profiles"], np.float64)):
        np.save(os.path.join(d, s + "_p_visit_array.npy"), p)
    return d, names, rankdata(np.asarray(z["profiles"], np.float64), axis=1), [str(n) for n in z["nodelist"]]


def expected_distances(names, ranks, rows, cols):
    """scipy's correlation distance of the saved vectors' ranks; the nearest-first order of every row must not hang on a rounding"""
    M.check_spread(ranks)
    d = scipy_corr(ranks[[names.index(r) for r in rows]], ranks[[names.index(c) for c in cols]])
    for i, r in enumerate(rows):
        row = np.sort(d[i][[c != r for c in cols]])
        assert np.diff(row).min() > 4 * M.dot_abs_bound(ranks.shape[1]), r
    return d


def _run(script, args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=str(cwd), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_evaluate_auc_ranks_by_spearman(tmp_path):
    from gcn_drug_repurposing_amd import evaluate
    dp, names, ranks, _ = stage_saved_profiles(tmp_path)
    cfg = EF.stage(tmp_path, "diffusion", diffusion={"eval_diffusion_embs_dir": dp, "compare": "spearman"})
    s = evaluate.Settings(evaluate.load_config(cfg))
    res = evaluate.run(s, err=open(os.devnull, "w"))
    assert isinstance(res.scores, torch.Tensor) and res.scores.is_cuda
    want = expected_distances(names, ranks, res.indications, res.drugs)
    worst = M.compare(-res.scores.cpu().numpy(), want, "correlation", 111)
    record_measured("spearman.evaluate", worst_in_bounds=worst)
    pos_ptr, pos_col, _, _ = evaluate.label_rows(res.indications, res.drugs, evaluate.read_drug_indication_tsv(s.labels))
    auc, n_pos, n_neg = EF.mirror_aucs(-want, pos_ptr, pos_col)               # the order is safe from rounding: the AUCs are those of scipy's distances
    assert np.array_equal(res.n_pos, n_pos) and np.array_equal(res.n_neg, n_neg)
    assert np.array_equal(res.auc[res.kept], auc[res.kept]) and len(res.kept) >= 2
    r = _run("evaluate_auc.py", ["-c", cfg, "--per-indication", "per.tsv"], tmp_path)
    inds, aucs, _ = EF.read_per_indication(tmp_path / "per.tsv")
    assert inds == [res.indications[k] for k in res.kept] and np.array_equal(aucs, auc[res.kept])
    got = EF.LINE.match(r.stdout.strip())
    assert got and abs(float(got.group(1)) - np.median(auc[res.kept])) <= 1e-12 and abs(float(got.group(2)) - auc[res.kept].mean()) <= 1e-12


def test_predict_drug_and_compare_profiles_rank_by_spearman(tmp_path):
    dp, names, ranks, nodelist = stage_saved_profiles(tmp_path)
    drugs = [n for n in nodelist if n in names and n.startswith("DB")]        # the programs list drugs in node order
    assert len(drugs) == 12
    g = PF.msi_graph(False)
    cfg = PF.stage(tmp_path, "diffusion", diffusion={"diffusion_embs_dir": dp, "compare": "spearman"})
    _run("predict_drug.py", ["-c", cfg], tmp_path)
    want_row = expected_distances(names, ranks, ["NodeCovid"], drugs)[0]
    order = np.argsort(want_row, kind="stable")
    rows = PF.read_tsv(tmp_path / "drugs.tsv")
    assert [r[0] for r in rows] == [PF.display(g, drugs[i]) for i in order[:PF.TOPK]]
    M.compare(-np.asarray([float(r[1]) for r in rows]), want_row[order[:PF.TOPK]], "correlation", 111)
    _run("compare_profiles.py", ["-c", cfg, "--metric", "spearman", "--rows", "drugs", "--cols", "drugs", "--top", "3", "--matrix", "D.npy"], tmp_path)
    want = expected_distances(names, ranks, drugs, drugs)
    D = np.load(tmp_path / "D.npy")
    worst = M.compare(D, want, "correlation", 111)
    record_measured("spearman.compare_profiles", worst_in_bounds=worst)
    got = PF.read_tsv(tmp_path / "neighbours.tsv")
    near = M.nearest(want, drugs, drugs, 3)
    assert [(r[0], int(r[2]), r[3]) for r in got] == [(r, k, c) for r, k, c, _ in near] and len(got) == 3 * len(drugs)
    lookup = {(r, c): D[i, j] for i, r in enumerate(drugs) for j, c in enumerate(drugs)}
    assert all(r[5] == repr(float(lookup[(r[0], r[3])])) for r in got)       # repr-exact fp64


def _spy_on_pairs(monkeypatch):
    """every compare_profile_pairs call knockout.py makes: the profile tensor it ran on pulled to the host, the lists and what came back"""
    from gcn_drug_repurposing_amd import diffusion
    seen, real = [], diffusion.compare_profile_pairs

    def spy(x, col_a, col_b, metric, device="cuda"):
        d = real(x, col_a, col_b, metric, device)
        seen.append((x.detach().cpu().numpy().copy(), list(col_a), list(col_b), metric, d.cpu().numpy().copy()))
        return d
    monkeypatch.setattr(diffusion, "compare_profile_pairs", spy)
    return seen


def _check_knockouts(seen, records):
    """the distances of a run against scipy on the ranks of the very profile tensor the run produced -> the worst error in bounds"""
    assert seen and records
    worst, values = 0.0, []
    for x, ca, cb, metric, dist in seen:
        assert metric == "spearman"
        used = sorted(set(ca) | set(cb))
        ranks = np.zeros((x.shape[1], x.shape[0]))
        ranks[used] = rankdata(x[:, used].T, axis=1)
        M.check_spread(ranks[used])
        worst = max(worst, M.compare(dist, scipy_corr_pairs(ranks, ca, cb), "correlation", x.shape[0]))
        values += [float(v) for v in dist]
    for r in records:
        for h in ("dist_before", "dist_after", "shift_drug", "shift_indication"):
            assert any(r[h] == v or (r[h] != r[h] and v != v) for v in values), (h, r)
        assert r["delta"] == r["dist_after"] - r["dist_before"] or r["delta"] != r["delta"]
    return worst


def test_knockout_by_spearman_in_both_modes(tmp_path, monkeypatch, capsys):
    from gcn_drug_repurposing_amd import knockout as K
    seen = _spy_on_pairs(monkeypatch)
    cfg = EF.stage(tmp_path, "diffusion", with_embs=False)
    rows = [("DB00003", "C0000000", "151"), ("DB00003", "C0000004", "151"), ("DB00003", "NodeCovid", "151"), ("DB00003", "C0000000", "104")]
    table = tmp_path / "triples.tsv"
    table.write_text("drug\tindication\tgene\n" + "".join("\t".join(r) + "\n" for r in rows))
    out = str(tmp_path / "ko.tsv")
    K.main(["-c", cfg, "--triples", str(table), "--metric", "spearman", "--out", out])
    assert capsys.readouterr().out.strip() == f"spearman: 4 knock-outs: {out}"
    got = PF.read_tsv(out)
    assert [tuple(x[:3]) for x in got] == rows
    records = [dict(zip(K.HEADER, x[:4] + [float(v) for v in x[4:9]] + [int(v) for v in x[9:]])) for x in got]
    worst = _check_knockouts(seen, records)
    del seen[:]
    genes = ["151", "104", "118", "119", "158"]
    (tmp_path / "genes.txt").write_text("\n".join(genes) + "\n")
    rec = K.run(cfg, drug="DB00003", indication="C0000000", genes=str(tmp_path / "genes.txt"), metric="spearman", out=str(tmp_path / "s.tsv"))
    assert sorted(x["gene"] for x in rec) == sorted(genes)
    worst = max(worst, _check_knockouts(seen, rec))
    assert [x[2] for x in PF.read_tsv(tmp_path / "s.tsv")] == [x["gene"] for x in rec]
    record_measured("spearman.knockout", worst_in_bounds=worst)
    print("knock-out distances, worst / bound", worst)
