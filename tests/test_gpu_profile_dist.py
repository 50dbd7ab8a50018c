"""GPU: gss_profile_dist (csrc/profile_dist.hip) against scipy's cdist within the derived bounds of profile_dist_mirror.py, its order-stability
contract bit for bit, its refusals by name, the device profiles of PprEngine.run compared in place, and the four programs end to end on the
small fixtures with diffusion.compare set."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_fixture as EF  # noqa: E402
import predict_fixture as PF  # noqa: E402
import profile_dist_mirror as M  # noqa: E402
from conftest import record_measured  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import compare_profiles  # noqa: E402

pytestmark = pytest.mark.gpu
END_TO_END = 1e-8     # device profiles differ from the reference's by <= 1e-13; worst propagation (Canberra) 3.5e-9 relative, times three


def dist(profiles, rows, cols, metric):
    return compare_profiles(profiles, rows, cols, metric).cpu().numpy()


def scipy_dist(a, b, metric):
    with np.errstate(invalid="ignore", divide="ignore"):
        return cdist(a, b, metric)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_reference_profiles_all_pairs_and_through_permuted_repeated_lists():
    fx = M.fixture()
    names, prof = M.reference_profiles()
    M.check_spread(prof)
    drugs = [i for i, n in enumerate(names) if n.startswith("DB")]
    inds = [i for i, n in enumerate(names) if not n.startswith("DB")]
    rng = np.random.RandomState(0)
    rows = list(rng.permutation(drugs)) + [drugs[3], drugs[3], drugs[0]]
    cols = list(rng.permutation(inds)) + [inds[-1], inds[2]]
    for m in M.METRICS:
        worst = M.compare(dist(prof, None, None, m), fx["d_" + m], m, 111)
        worst = max(worst, M.compare(dist(prof, rows, cols, m), fx["d_" + m][np.ix_(rows, cols)], m, 111))
        record_measured("profile_dist.reference_profiles." + m, worst_in_bounds=worst)
        print(m, "worst / bound", worst)


@pytest.mark.parametrize("n", [111, 1000, 29960])
@pytest.mark.parametrize("shape", [(1, 1), (1, 65), (17, 300), (128, 128)])
def test_synthetic_profiles_against_cdist(n, shape):
    na, nb = shape
    p = M.synthetic(n + 7 * na + nb, na + nb, n, lognormal=(n == 1000))
    M.check_spread(p)
    assert (p == 0).mean() > 0.05
    x = torch.from_numpy(p).cuda().t().contiguous()
    for m in M.METRICS:
        got = dist(x, range(na), range(na, na + nb), m)
        worst = M.compare(got, scipy_dist(p[:na], p[na:], m), m, n)
        record_measured(f"profile_dist.synthetic.{m}.n{n}.{na}x{nb}", worst_in_bounds=worst)
        print(m, n, shape, "worst / bound", worst)


def _call(n, x, ld, na, ca, nb, cb, metric, out, ld_out):
    lib = _lib.load()
    rc = lib.gss_profile_dist(n, _lib.ptr(x), ld, na, _lib.ptr(ca), nb, _lib.ptr(cb), metric, _lib.ptr(out), ld_out, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, lib.gss_last_error().decode(errors="replace")


def test_ld_larger_than_the_column_count():
    k, n = 37, 203
    p = M.synthetic(11, k, n)
    x = torch.full((n, k + 9), float("nan"), dtype=torch.float64, device="cuda")
    x[:, :k] = torch.from_numpy(p).cuda().t()
    out = torch.full((k, k + 5), -7.0, dtype=torch.float64, device="cuda")
    for mi, m in enumerate(M.METRICS):
        rc, msg = _call(n, x, k + 9, k, None, k, None, mi, out, k + 5)
        assert rc == 0, msg
        M.compare(out[:, :k].cpu().numpy(), scipy_dist(p, p, m), m, n)
        assert bool((out[:, k:] == -7.0).all())          # nothing is written beyond nb


def test_one_row():
    p = np.random.RandomState(5).rand(6, 1)
    p[[1, 4]] = 0.0
    for m in M.METRICS:
        got = dist(p, None, None, m)
        want = scipy_dist(p, p, m)
        if m == "correlation":
            assert np.isnan(want).all()
        M.compare(got, want, m, 1)


def test_degenerate_case():
    fx = M.fixture()
    for m in M.METRICS:
        M.compare(dist(M.DEGENERATE, None, None, m), fx["deg_" + m], m, 4)


def test_order_stability_bit_for_bit():
    p = M.synthetic(7, 450, 1000)
    x = torch.from_numpy(p).cuda().t().contiguous()
    rng = np.random.RandomState(1)
    a, b = np.arange(300), rng.permutation(450)[:300]
    for m in M.METRICS:
        ab, again, ba = dist(x, a, b, m), dist(x, a, b, m), dist(x, b, a, m)
        assert not np.isnan(ab).any()
        assert np.array_equal(bits(ab), bits(again)), m                      # two runs
        assert np.array_equal(bits(ab), bits(ba.T)), m                       # out(a, b) == out(b, a)
        for i, j in ((0, 0), (299, 299), (137, 64), (63, 255), (64, 17)):   # a pair alone == the pair inside the 300 x 300 call
            one = dist(x, [a[i]], [b[j]], m)
            assert bits(one)[0, 0] == bits(ab)[i, j], (m, i, j)
        if m in M.DIFF_CLASS:
            aa = dist(x, b, b, m)
            assert np.array_equal(np.diag(aa), np.zeros(300)) and not np.signbit(np.diag(aa)).any(), m


def test_refusals_by_name():
    x = torch.rand(8, 6, dtype=torch.float64, device="cuda")
    out = torch.zeros(6, 6, dtype=torch.float64, device="cuda")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device="cuda")   # noqa: E731
    cases = [((8, None, 6, 6, None, 6, None, 0, out, 6), "x is null"),
             ((8, x, 6, 6, None, 6, None, 0, None, 6), "out is null"),
             ((0, x, 6, 6, None, 6, None, 0, out, 6), "n=0"),
             ((8, x, 6, 6, None, 6, None, 5, out, 6), "metric 5 is unknown"),
             ((8, x, 6, 6, None, 6, None, -1, out, 6), "metric -1 is unknown"),
             ((8, x, 0, 6, None, 6, None, 0, out, 6), "ld=0"),
             ((8, x, 3, 6, None, 2, None, 0, out, 6), "ld=3 is below na=6"),
             ((8, x, 3, 2, None, 6, None, 0, out, 6), "ld=3 is below nb=6"),
             ((8, x, 6, 6, None, 6, None, 0, out, 2), "ld_out=2 is below nb=6"),
             ((8, x, 6, 2, i32([0, 6]), 6, None, 3, out, 6), "cols_a[1] = 6 is outside [0, ld=6)"),
             ((8, x, 6, 6, None, 3, i32([1, 2, -1]), 1, out, 6), "cols_b[2] = -1 is outside [0, ld=6)")]
    for args, message in cases:
        rc, msg = _call(*args)
        assert rc == -22 and message in msg, (message, rc, msg)
    assert bool((out == 0).all())                                            # no refused call wrote anything
    rc, msg = _call(8, x, 6, 2, i32([5, 0]), 6, None, 0, out, 6)
    assert rc == 0, msg
    M.compare(out[:2].cpu().numpy(), scipy_dist(x.cpu().numpy().T[[5, 0]], x.cpu().numpy().T, "cityblock"), "cityblock", 8)
    # lists of more than one 256-thread block of the check: the least offending position is named, cols_a's before cols_b's, nothing is
    # written, and the status words are armed again by every call
    n, ld, L = 70, 8, 300
    x = torch.rand(n, ld, dtype=torch.float64, device="cuda")
    h = x.cpu().numpy().T
    rng = np.random.RandomState(3)
    ga, gb = rng.randint(0, ld, L), rng.randint(0, ld, L)

    def with_bad(v, *entries):
        w = v.copy()
        for at, e in entries:
            w[at] = e
        return i32(w)
    out = torch.full((L, L), -7.0, dtype=torch.float64, device="cuda")
    for ca, cb, message in ((with_bad(ga, (290, 8), (270, -3)), i32(gb), "cols_a[270] = -3 is outside [0, ld=8)"),
                            (with_bad(ga, (290, 8)), with_bad(gb, (5, 9)), "cols_a[290] = 8 is outside [0, ld=8)"),
                            (i32(ga), with_bad(gb, (299, 8)), "cols_b[299] = 8 is outside [0, ld=8)"),
                            (None, with_bad(gb, (299, -1)), "cols_b[299] = -1 is outside [0, ld=8)")):
        rc, msg = _call(n, x, ld, L if ca is not None else ld, ca, L, cb, 0, out, L)
        assert rc == -22 and msg.startswith("profile_dist: ") and message in msg, (message, rc, msg)
        assert bool((out == -7.0).all()), message
    rc, msg = _call(n, x, ld, L, i32(ga), L, i32(gb), 0, out, L)             # the same buffers, valid lists
    assert rc == 0, msg
    M.compare(out.cpu().numpy(), scipy_dist(h[ga], h[gb], "cityblock"), "cityblock", n)
    every = i32(np.arange(ld))
    for mi in range(len(M.METRICS)):                                         # a null list beside a given one == the explicit 0 .. ld - 1, bit for bit
        explicit = torch.empty(ld, L, dtype=torch.float64, device="cuda")
        null_a, null_b = torch.empty(ld, L, dtype=torch.float64, device="cuda"), torch.empty(L, ld, dtype=torch.float64, device="cuda")
        assert _call(n, x, ld, ld, every, L, i32(gb), mi, explicit, L)[0] == 0 and _call(n, x, ld, ld, None, L, i32(gb), mi, null_a, L)[0] == 0
        assert torch.equal(null_a.view(torch.int64), explicit.view(torch.int64)), mi
        explicit = torch.empty(L, ld, dtype=torch.float64, device="cuda")
        assert _call(n, x, ld, L, i32(ga), ld, every, mi, explicit, ld)[0] == 0 and _call(n, x, ld, L, i32(ga), ld, None, mi, null_b, ld)[0] == 0
        assert torch.equal(null_b.view(torch.int64), explicit.view(torch.int64)), mi


def _gold():
    z = np.load(os.path.join(HERE, "golden", "diffusion_msi_small.npz"))
    nodes = [str(v) for v in z["nodelist"]]
    idx = {n: i for i, n in enumerate(nodes)}
    m0 = sp.csr_matrix((z["m_data"], z["m_indices"], z["m_indptr"]), shape=(len(nodes),) * 2)
    starts = np.array([idx[str(s)] for s in z["starts"]])
    prot = {idx[str(s)]: [idx[p] for p in str(ps).split()] for s, ps in zip(z["starts"], z["proteins_of"])}
    return m0, starts, prot, (float(z["alpha"]), float(z["tol"]), int(z["max_iter"]))


def test_device_profiles_go_into_the_comparison_in_place():
    from gcn_drug_repurposing_amd.diffusion import PprEngine, PprProblem
    fx = M.fixture()
    m0, starts, prot, (alpha, tol, max_iter) = _gold()
    eng = PprEngine(PprProblem(m0, starts, prot))
    x, _ = eng.run(alpha, tol, max_iter)
    k = len(starts)
    host = x[:, :k].t().contiguous().cpu().numpy()
    for m in M.METRICS:
        in_place = dist(x, range(k), range(k), m)
        assert np.array_equal(bits(in_place), bits(dist(host, None, None, m))), m
        _end_to_end(in_place, fx["d_" + m], m)


def _end_to_end(got, want, metric):
    err = np.abs(got - want)
    worst = float(err.max() if metric not in M.DIFF_CLASS else (err / np.where(want > 0, want, 1.0)).max())
    print(metric, "against the fixture's matrix", worst)
    assert worst <= END_TO_END, (metric, worst)
    return worst


def _run(script, args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=str(cwd), capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _saved(dp, nodes):
    return np.stack([np.load(os.path.join(str(dp), n + "_p_visit_array.npy")) for n in nodes])


@pytest.mark.parametrize("metric", M.METRICS)
def test_evaluate_auc_with_each_metric(tmp_path, metric):
    from gcn_drug_repurposing_amd import evaluate
    fx = M.fixture()
    names = [str(n) for n in fx["names"]]
    dp = tmp_path / "dp"
    cfg = EF.stage(tmp_path, "diffusion", diffusion={"eval_diffusion_embs_dir": str(dp), "compare": metric})
    assert not dp.exists()                                   # the device makes the profiles and the program saves them
    res = evaluate.run(evaluate.Settings(evaluate.load_config(cfg)), err=open(os.devnull, "w"))
    assert isinstance(res.scores, torch.Tensor) and res.scores.is_cuda          # the scores never visited the host
    used = -res.scores.cpu().numpy()
    assert res.drugs == [str(d) for d in fx["drugs"]]
    worst = M.compare(used, scipy_dist(_saved(dp, res.indications), _saved(dp, res.drugs), metric), metric, 111)
    record_measured("profile_dist.evaluate." + metric, worst_in_bounds=worst)
    want = fx["d_" + metric][np.ix_([names.index(i) for i in res.indications], [names.index(d) for d in res.drugs])]
    _end_to_end(used, want, metric)
    r = _run("evaluate_auc.py", ["-c", cfg, "--per-indication", "per.tsv"], tmp_path)
    inds, aucs, _ = EF.read_per_indication(tmp_path / "per.tsv")
    assert inds == [str(i) for i in fx["auc_indications"]]
    assert np.max(np.abs(np.asarray(aucs) - fx["auc_" + metric])) <= 1e-12
    got = EF.LINE.match(r.stdout.strip())
    assert got, r.stdout
    assert abs(float(got.group(1)) - np.median(fx["auc_" + metric])) <= 1e-12 and abs(float(got.group(2)) - fx["auc_" + metric].mean()) <= 1e-12


def test_predict_interpret_and_compare_profiles_rank_by_correlation(tmp_path):
    fx = M.fixture()
    names = [str(n) for n in fx["names"]]
    drugs = [str(d) for d in fx["drugs"]]
    g = PF.msi_graph(False)
    dp = tmp_path / "dp"
    cfg = PF.stage(tmp_path, "diffusion", diffusion={"diffusion_embs_dir": str(dp), "compare": "correlation"})
    _run("predict_drug.py", ["-c", cfg], tmp_path)
    want_row = fx["d_correlation"][names.index("NodeCovid"), [names.index(d) for d in drugs]]
    order = np.argsort(want_row, kind="stable")
    rows = PF.read_tsv(tmp_path / "drugs.tsv")
    assert [r[0] for r in rows] == [PF.display(g, drugs[i]) for i in order[:PF.TOPK]]
    used = -np.asarray([float(r[1]) for r in rows])
    _end_to_end(used, want_row[order[:PF.TOPK]], "correlation")
    saved = scipy_dist(_saved(dp, ["NodeCovid"]), _saved(dp, [drugs[i] for i in order[:PF.TOPK]]), "correlation")[0]
    M.compare(used, saved, "correlation", 111)
    _run("interpret.py", ["-c", cfg, "--top", "3"], tmp_path)
    assert [r[1] for r in PF.read_tsv(tmp_path / "trace.tsv")] == [PF.display(g, drugs[i]) for i in order[:3]]
    _run("compare_profiles.py", ["-c", cfg, "--metric", "correlation", "--rows", "drugs", "--cols", "drugs", "--top", "3", "--matrix", "D.npy"],
         tmp_path)
    di = [names.index(d) for d in drugs]
    want = M.nearest(fx["d_correlation"][np.ix_(di, di)], drugs, drugs, 3)
    got = PF.read_tsv(tmp_path / "neighbours.tsv")
    assert [(r[0], int(r[2]), r[3]) for r in got] == [(r, k, c) for r, k, c, _ in want] and len(got) == 3 * len(drugs)
    assert all(r[0] != r[3] for r in got)
    assert [r[1] for r in got] == ["NA" if g.node2name.get(r[0]) is None else g.node2name[r[0]] for r in got]
    _end_to_end(np.asarray([float(r[5]) for r in got]), np.asarray([d for _, _, _, d in want]), "correlation")
    D = np.load(tmp_path / "D.npy")
    M.compare(D, scipy_dist(_saved(dp, drugs), _saved(dp, drugs), "correlation"), "correlation", 111)
    lookup = {(r, c): D[i, j] for i, r in enumerate(drugs) for j, c in enumerate(drugs)}
    assert all(r[5] == repr(float(lookup[(r[0], r[3])])) for r in got)       # repr-exact fp64
