"""CPU: the mirror of DIAMOnD's growth (tests/diamond_mirror.py) against scipy.stats.hypergeom over ALL candidates at every step of every
case of tests/diamond_cases.py, that every case has the property it was built for and keeps the winner MIN_GAP away from the runner-up,
the hold-out draws and the writers of diamond.py, and that header, library and binding hold gss_diamond_grow.

The bounds: the mirror's logp is lt0 + log(S) with lt0 a sum of nine lgamma values of magnitude up to about 1e5 (cancellation: a relative
1e-10 of the result covers it; 7e-12 was measured on the 2016 network) and S a sum of positive terms; scipy's logsf is the reference.
The node the two-stage rule picks must attain the minimum of logsf over all candidates to within 1e-9 relative."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import diamond_cases as K  # noqa: E402
import diamond_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import diamond, diamond_cli  # noqa: E402
from gcn_drug_repurposing_amd.proximity import ProximityError  # noqa: E402



@pytest.mark.parametrize("name", K.CASES)
def test_the_choice_attains_the_minimum_of_scipys_logsf_over_all_candidates(name):
    from scipy.stats import hypergeom
    c = K.case(name)
    want = K.mirror(name)
    worst_pick, worst_logp = 0.0, 0.0
    for u, seeds in enumerate(c.units):
        steps = []
        M.grow(c.rowptr, c.col, seeds, c.n_add, c.alpha, on_step=lambda st: steps.append((st.N, st.s) + st.candidates()))
        live = int((want["node"][u] >= 0).sum())
        assert len(steps) == min(live + 1, c.n_add) and all(len(s[2]) > 0 for s in steps[:live]), (name, u)
        for t in range(live):
            N, s, v, k, kb = steps[t]
            pairs, where = np.unique(np.stack([k, kb], axis=1), axis=0, return_inverse=True)   # candidates with the same (k', kb') share a tail
            ref = hypergeom.logsf(pairs[:, 1] - 1, N, s, pairs[:, 0])[where.reshape(-1)]
            j = int(np.flatnonzero(v == want["node"][u, t])[0])
            assert (k[j], kb[j]) == (want["k"][u, t], want["kb"][u, t])
            low = ref.min()
            pick = abs(ref[j] - low) / max(abs(low), 1e-300)
            err = abs(want["logp"][u, t] - ref[j]) / max(abs(ref[j]), 1e-300)
            worst_pick, worst_logp = max(worst_pick, pick), max(worst_logp, err)
            assert pick <= 1e-9, (name, u, t, pick)
            assert err <= 1e-10, (name, u, t, err)
    print(f"{name}: the pick is within {worst_pick:.3g} of the minimum, logp within {worst_logp:.3g} of logsf (relative)")


@pytest.mark.parametrize("name", K.CASES)
def test_every_step_keeps_the_runner_up_away(name):
    r = K.mirror(name)
    gap = np.where(r["node"] >= 0, r["gap"], np.inf)
    assert gap.min() > K.MIN_GAP, (name, np.argwhere(gap <= K.MIN_GAP)[:5])
    after = r["node"] < 0                                                       # once -1, -1 and zeros to the end
    assert np.array_equal(after, np.maximum.accumulate(after, axis=1))
    for f in ("k", "kb", "lt0", "S", "logp"):
        assert (r[f][after] == 0).all()
    assert (r["S"][~after] >= 1.0).all() and (r["logp"][~after] <= 1e-12).all()
    for u, seeds in enumerate(K.case(name).units):                              # nothing added twice, no seed added
        got = r["node"][u][r["node"][u] >= 0]
        assert len(set(got.tolist())) == len(got) and not np.isin(got, seeds).any()


def test_every_case_has_the_property_it_was_built_for():
    for name in ("n40_a1", "n300_a1", "n1500"):
        assert K.case(name).n % 64 != 0
    assert K.case("n1500").n > K.THREADS and (K.mirror("n40_a1")["node"] >= 0).all()
    star = K.case("star")
    deg = np.diff(star.rowptr)
    assert deg[K.HUB] == K.HUB_DEG > K.THREADS and K.HUB in star.units[0] and K.HUB not in star.units[1]
    assert K.mirror("star")["node"][1, 0] == K.HUB and K.mirror("star")["kb"][1, 0] == 30         # the hub's row is walked as a winner's
    assert K.mirror("tail")["terms"].max() >= 500 and len(K.case("tail").units[0]) == 600
    odd = K.mirror("odd")
    assert sorted(odd["node"][0, :4].tolist()) == [0, 2, 4, 5] and (odd["node"][0, 4:] == -1).all()   # the path is used up after 4 steps
    assert np.diff(K.case("odd").rowptr)[26] == 0
    assert (odd["node"][1] == -1).all() and (odd["node"][4] == -1).all() and (odd["node"][5] == -1).all()
    assert (odd["node"][2] >= 0).all() and (odd["node"][3] >= 0).all()
    assert K.case("ring").n == K.MAX_NODES == diamond.MAX_NODES and (np.diff(K.case("ring").rowptr) == 2).all()
    assert set(K.mirror("ring")["kb"].ravel().tolist()) == {1, 2}
    assert len(K.case("many").units) > K.MAX_BLOCKS
    for name in ("n40_a3", "n300_a2", "odd_a2"):
        assert K.case(name).alpha > 1
    assert not np.array_equal(K.mirror("n40_a1")["node"], K.mirror("n40_a3")["node"])             # the weight changes the growth


def test_the_tail_in_log_space_does_not_underflow():
    """P(X >= 400) of 400 draws out of 20,000 with 400 marked is far below the smallest fp64; its log is an ordinary number"""
    from scipy.stats import hypergeom
    lg = M.lgamma_table(20002)
    lt0, S, logp, terms = M.tail(lg, 20000, 400, 400, 400)
    assert terms == 0 and S == 1.0 and logp == lt0 < -1800
    assert abs(logp - hypergeom.logsf(399, 20000, 400, 400)) <= 1e-10 * abs(logp) and hypergeom.sf(399, 20000, 400, 400) == 0.0
    assert np.array_equal(diamond.lgamma_table(500), M.lgamma_table(500))


def test_header_library_and_binding_hold_the_export():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    header = open(os.path.join(ROOT, "include", "gssgcn.h")).read()
    assert re.search(r"^int gss_diamond_grow\(", header, flags=re.M)
    assert int(re.search(r"#define GSS_ABI_VERSION (\d+)", header).group(1)) == pkg._lib.ABI_VERSION == 25
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r" T gss_diamond_grow$", out, flags=re.M)
    res, args = pkg._lib.SIGNATURES["gss_diamond_grow"]
    assert len(args) == 19 and pkg._lib.load().gss_diamond_grow.argtypes == args
    assert "diamond.hip" in open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "Makefile")).read()


# ---- the host side of diamond.py -------------------------------------------------------------------------------------------------------

def test_holdout_draws():
    sets = [np.arange(10, 30, dtype=np.int32), np.array([3], np.int32), np.array([], np.int32), np.array([5, 9], np.int32)]
    draws = diamond.holdout_draws(sets, 0.25, 7, 3)
    again = diamond.holdout_draws(sets, 0.25, 7, 3)
    assert [len(r) for r in draws] == [7, 7, 7, 7]
    for s, reps, reps2 in zip(sets, draws, again):
        for (kept, held), (kept2, held2) in zip(reps, reps2):
            assert np.array_equal(kept, kept2) and np.array_equal(held, held2)
            assert np.array_equal(np.sort(np.concatenate([kept, held])), s) and kept.dtype == held.dtype == np.int32
            assert (np.diff(kept) > 0).all()
    assert {len(h) for _, h in draws[0]} == {5} and len({tuple(h) for _, h in draws[0]}) > 1
    assert all(len(h) == 0 for _, h in draws[1] + draws[2]) and all(len(h) == 1 and len(k) == 1 for k, h in draws[3])
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(draws[0], diamond.holdout_draws(sets, 0.25, 7, 4)[0]))
    for kw, words in ((dict(holdout=0.0), "holdout=0.0 must be in"), (dict(holdout=1.0), "holdout=1.0 must be in"),
                      (dict(repeats=0), "repeats=0 must be >= 1")):
        with pytest.raises(ProximityError, match=words):
            diamond.holdout_draws(sets, **{"holdout": 0.25, "repeats": 2, "seed": 0, **kw})


def test_grow_refusals_need_no_device():
    eng = diamond.DiamondEngine.__new__(diamond.DiamondEngine)
    eng.net = type("Net", (), {"n": 100})()
    eng.max_deg = 870
    eng._rowptr = eng._col = eng._lg = eng._torch = None                      # what close() leaves; __del__ closes again
    ok = [np.array([1, 2], np.int32)]
    for args, words in (((ok, 0, 1), "n_add=0 must be >= 1"), ((ok, 5, 0), "alpha=0 must be >= 1"), (([], 5, 1), "node_sets must not be empty"),
                        (([np.arange(4097)], 5, 1), "a set has 4097 seeds; at most 4096"), ((ok, 5, 76), "alpha=76 x the largest degree 870 is over 65535")):
        with pytest.raises(ProximityError, match=words):
            eng.check(*args)
    assert eng.check([np.arange(4000)], 200, 1)[1] == 4000                 # a node's links are bounded by its degree, 870
    eng.max_deg = 5000
    with pytest.raises(ProximityError, match="a node can have 4199 weighted links"):
        eng.check([np.arange(4000)], 200, 1)
    eng.net.n = diamond.MAX_NODES + 1
    with pytest.raises(ProximityError, match="a network of 30721 nodes; between 1 and 30720"):
        eng.check(ok, 5, 1)
    with pytest.raises(ProximityError, match="the engine is closed"):
        eng.grow(ok)


def test_writers_and_arguments(tmp_path, capsys):
    res = {"node": np.array([[2, 0, -1], [1, -1, -1]]), "k": np.array([[5, 3, 0], [2, 0, 0]]), "kb": np.array([[2, 1, 0], [1, 0, 0]]),
           "logp": np.array([[-3.5, -0.25, 0.0], [-1.0, 0.0, 0.0]]), "p": np.array([[np.exp(-3.5), np.exp(-0.25), np.nan], [np.exp(-1.0), np.nan, np.nan]])}
    diamond_cli.write_modules(tmp_path / "m.tsv", ["a", "b c"], ["g0", "g1", "g2"], res)
    assert (tmp_path / "m.tsv").read_text() == ("set\trank\tgene\tk\tkb\tlogp\tp\n" f"a\t1\tg2\t5\t2\t-3.5\t{float(np.exp(-3.5))!r}\n"
                                                f"a\t2\tg0\t3\t1\t-0.25\t{float(np.exp(-0.25))!r}\n" f"b c\t1\tg1\t2\t1\t-1.0\t{float(np.exp(-1.0))!r}\n")
    diamond_cli.write_summary(tmp_path / "s.tsv", ["a", "b c"], [4, 1], [2, 1], [3, 1], [6, 2])
    assert (tmp_path / "s.tsv").read_text() == "set\tn.seeds\tn.added\tlcc.seeds\tlcc.module\na\t4\t2\t3\t6\nb c\t1\t1\t1\t2\n"
    diamond_cli.write_recovery(tmp_path / "r.tsv", ["a"], {"recovered": np.array([[0, 2, 3]]), "held": np.array([8])})
    assert (tmp_path / "r.tsv").read_text() == "set\trank\trecovered\theld\na\t1\t0\t8\na\t2\t2\t8\na\t3\t3\t8\n"
    (tmp_path / "seeds.tsv").write_text("# a comment\none\tA\tB\n\ntwo\tC\none\tD\t\n")
    assert diamond_cli.load_seed_sets(tmp_path / "seeds.tsv") == {"one": {"A", "B", "D"}, "two": {"C"}}
    base = ["--network", "n.sif"]
    for args, words in ((base, "one of the arguments --diseases --drugs --seeds is required"),
                        (base + ["--seeds", "s", "--drugs", "t"], "not allowed with argument"),
                        (base + ["--seeds", "s", "--n-add", "0"], "--n-add 0 must be >= 1"), (base + ["--seeds", "s", "--alpha", "0"], "--alpha 0 must be >= 1"),
                        (base + ["--seeds", "s", "--holdout", "1.5"], "--holdout 1.5 must be in"),
                        (base + ["--seeds", "s", "--repeats", "0"], "--repeats 0 must be >= 1")):
        with pytest.raises(SystemExit) as e:
            diamond_cli.parse_args(args)
        assert e.value.code == 2 and words in capsys.readouterr().err, args
    a = diamond_cli.parse_args(base + ["--diseases", "d.tsv", "--set", "x", "--set", "y"])
    assert (a.n_add, a.alpha, a.out, a.summary, a.holdout, a.repeats, a.seed, a.recovery, a.set) == (200, 1, "modules.tsv", None, None, 100, 0,
                                                                                                  "recovery.tsv", ["x", "y"])
