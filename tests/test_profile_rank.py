"""CPU: the numpy mirror of csrc/profile_rank.hip (keys, chunked sort, two searches per chunk, (acc + 1) / 2) bit for bit against
scipy.stats.rankdata, the workspace formula, and "spearman" as a sixth metric name in the settings, the command lines and the API.  The
device kernel is checked in test_gpu_profile_rank.py, the composed distance in test_gpu_spearman.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.stats import rankdata

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_fixture as EF  # noqa: E402
import predict_fixture as PF  # noqa: E402
import profile_dist_mirror as M  # noqa: E402
import profile_rank_mirror as R  # noqa: E402

SIX = M.METRICS + ("spearman",)


def test_mirror_constants_are_the_kernels():
    csrc = os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc")
    text = open(os.path.join(csrc, "profile_rank.hip")).read() + open(os.path.join(csrc, "profile_front.h")).read()   # the shared front end
    for name, value in (("kRkChunk", R.CHUNK), ("kKeyPanel", R.PANEL), ("kStatusBytes", R.STATUS_BYTES)):
        assert [int(v) for v in re.findall(r"constexpr int %s = (\d+);" % name, text)] == [value]                  # stated once


def test_keys_order_as_ieee_comparison_orders():
    v = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 2.2e-308, 1.0, 1e300, np.inf])
    k = R.keys(v)
    assert k[4] == k[5]                                                       # -0.0 and +0.0 are one value
    assert np.all(np.diff(np.delete(k, 4).astype(object)) > 0)               # everything else strictly ascending
    assert np.all(k < R.BEHIND) and R.keys(np.array([np.nan, -np.nan]))[0] == R.BEHIND == R.keys(np.array([np.nan, -np.nan]))[1]


@pytest.mark.parametrize("n", R.SIZES)
def test_mirror_is_bit_equal_to_rankdata(n):
    for j, kind in enumerate(R.KINDS):
        v = R.column(kind, n, 1000 * n + j)
        want = rankdata(v, method="average")
        got = R.mirror_rank(v)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.int64), want.view(np.int64)), (n, kind)
        assert np.all(got * 2 == np.round(got * 2))                           # integers and half-integers
    if n >= 64:
        v = R.column("zeros_and_tails", n, n)
        assert (v == 0).mean() > 0.4 and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
        assert np.isinf(v).sum() >= 2 and (np.abs(v) == 5e-324).sum() >= 2
        assert np.array_equal(R.mirror_rank(v, 64), rankdata(v))              # another chunk length: the scheme, not the constant


def test_mirror_propagates_a_nan():
    v = R.column("uniform", 70, 3)
    v[17] = np.nan
    assert np.isnan(R.mirror_rank(v)).all() and np.isnan(rankdata(v, nan_policy="propagate")).all()


@pytest.fixture(scope="module")
def lib():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    return pkg.load()


def test_library_exports_the_two_entry_points_and_the_workspace_formula(lib):
    import gcn_drug_repurposing_amd as pkg
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("gss_profile_rank", "gss_profile_rank_workspace_bytes"):
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert name in pkg._lib.SIGNATURES
    for n, nc in ((1, 1), (63, 17), (29960, 1), (29960, 511), (29960, 512), (29960, 513), (29960, 2502), (1 << 24, 3), (5, 0)):
        assert lib.gss_profile_rank_workspace_bytes(n, nc) == R.workspace_bytes(n, nc), (n, nc)
    assert lib.gss_profile_rank_workspace_bytes(29960, 2502) == lib.gss_profile_rank_workspace_bytes(29960, 512)   # a panel, not nc
    assert lib.gss_profile_rank_workspace_bytes(0, 4) == 0 and lib.gss_profile_rank_workspace_bytes(4, -1) == 0


def test_refusals_that_come_before_the_gpu(lib):
    """argument checks that return before any HIP call (no device here): the pointers are never dereferenced"""
    def call(n, x, ld, nc, r, ld_r, ws, ws_bytes):
        rc = lib.gss_profile_rank(n, x, ld, nc, None, r, ld_r, ws, ws_bytes, None)
        return rc, lib.gss_last_error().decode()
    need = R.workspace_bytes(8, 4)
    cases = [((0, 8, 4, 4, 8, 4, 8, need), "n=0"), (((1 << 24) + 1, 8, 4, 4, 8, 4, 8, need), "quadratic in n / chunk"),
             ((8, 8, 4, -1, 8, 4, 8, need), "nc=-1"), ((8, 8, 0, 4, 8, 4, 8, need), "ld=0"), ((8, 8, 4, 4, 8, 3, 8, need), "ld_r=3 is below nc=4"),
             ((8, None, 4, 4, 8, 4, 8, need), "x is null"), ((8, 8, 4, 4, None, 4, 8, need), "r is null"),
             ((8, 8, 4, 4, 8, 4, None, need), "workspace is null"), ((8, 8, 3, 4, 8, 4, 8, need), "ld=3 is below nc=4"),
             ((8, 8, 4, 4, 8, 4, 12, need), "not 8-byte aligned"), ((8, 8, 4, 4, 8, 4, 8, need - 1), f"below the {need} that n=8, nc=4 need")]
    for args, message in cases:
        rc, msg = call(*args)
        assert rc == -22 and msg.startswith("profile_rank: ") and message in msg, (message, rc, msg)
    assert call(8, None, 4, 0, None, 0, None, 0)[0] == 0                      # nc = 0: a no-op


def test_metric_names():
    from gcn_drug_repurposing_amd import _lib, diffusion
    assert diffusion.METRICS == M.METRICS and len(diffusion.METRICS) == 5
    assert diffusion.RANK_METRICS == ("spearman",) and diffusion.ALL_METRICS == SIX
    assert diffusion.check_metric("spearman") == diffusion.METRICS.index("correlation")      # composed: no metric id of its own
    for fn in (lambda m: diffusion.compare_profiles(np.ones((2, 3)), None, None, m),
               lambda m: diffusion.compare_profile_pairs(np.ones((2, 3)), [0], [1], m)):
        with pytest.raises(ValueError, match="'kendall' is unknown") as e:
            fn("kendall")
        assert all(name in str(e.value) for name in SIX)
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        diffusion.compare_profiles(np.ones((2, 3)), None, None, "spearman", device="cpu")
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        diffusion.rank_profiles(np.ones((2, 3)), device="cpu")


def test_settings_accept_spearman_for_diffusion_only(tmp_path):
    from gcn_drug_repurposing_amd import evaluate, predict
    dp = {"diffusion_embs_dir": str(tmp_path / "dp"), "eval_diffusion_embs_dir": str(tmp_path / "dp")}
    for mod, fix in ((predict, PF), (evaluate, EF)):
        assert mod.Settings(fix.config(tmp_path, "diffusion", diffusion=dict(dp, compare="spearman"))).compare == "spearman"
        with pytest.raises(predict.PredictError, match="diffusion.compare = 'spearman' .* needs method = 'diffusion', not 'node2vec'"):
            mod.Settings(fix.config(tmp_path, "node2vec", diffusion=dict(dp, compare="spearman")))
        with pytest.raises(predict.PredictError, match="diffusion.compare = 'manhattan' is unknown") as e:
            mod.Settings(fix.config(tmp_path, "diffusion", diffusion=dict(dp, compare="manhattan")))
        assert all(name in str(e.value) for name in SIX + ("'visit'",))


def test_command_lines_accept_spearman(tmp_path):
    from gcn_drug_repurposing_amd import compare, knockout
    assert compare.parse_args(["--metric", "spearman"]).metric == "spearman"
    compare.check_args("spearman", "indications", "drugs", None, None, 10)
    with pytest.raises(compare.PredictError, match="--metric 'manhattan' is unknown") as e:
        compare.check_args("manhattan", "indications", "drugs", None, None, 10)
    assert all(name in str(e.value) for name in SIX)
    assert knockout.parse_args(["--metric", "spearman", "--triples", "t.tsv"]).metric == "spearman"
    cfg = EF.stage(tmp_path, "diffusion", with_embs=False)
    with pytest.raises(knockout.KnockoutError, match="give either --triples"):      # the metric passed; the next check speaks
        knockout.run(cfg, metric="spearman")
    with pytest.raises(knockout.KnockoutError, match="'chebyshev' is unknown") as e:
        knockout.run(cfg, triples="t.tsv", metric="chebyshev")
    assert all(name in str(e.value) for name in SIX)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = "-1"
    for script in ("compare_profiles.py", "knockout.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], cwd=str(tmp_path), capture_output=True, text=True, env=env,
                           timeout=300)
        assert r.returncode == 0 and all(name in r.stdout for name in SIX), script
