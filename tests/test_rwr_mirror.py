"""CPU: the mirror of the random walk with restart (tests/rwr_mirror.py) held to linear algebra, and the cases (tests/rwr_cases.py) to
what each was built for.  The device tests (tests/test_gpu_rwr_ops.py, tests/test_gpu_rwr.py) compare the kernels with this mirror bit
for bit, so whatever is shown here about the mirror holds for the kernels."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rwr_cases as K  # noqa: E402
import rwr_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _sets_cli, diamond, proximity as P  # noqa: E402

NET = os.path.join(HERE, "golden", "diamond_toy.sif")
SEEDS = os.path.join(HERE, "golden", "diamond_toy_seeds.tsv")
SMALL = [name for name in K.CASES if K.case(name).n <= 2100 and name != "many"]


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def exact(c, seeds):
    """p = r (I - (1 - r) W)^-1 p0 with W[i, j] = 1 / deg[j] on the edges"""
    deg = np.diff(c.rowptr).astype(np.float64)
    W = np.zeros((c.n, c.n))
    rows = np.repeat(np.arange(c.n), np.diff(c.rowptr))
    W[rows, c.col] = 1.0 / deg[c.col]
    p0 = np.zeros(c.n)
    p0[seeds] = 1.0 / len(seeds)
    return np.linalg.solve(np.eye(c.n) - (1.0 - c.restart) * W, c.restart * p0)


@pytest.mark.parametrize("name", SMALL)
def test_fixed_point_iterations_and_mass(name):
    c, got = K.case(name), K.mirror(name)
    for u, seeds in enumerate(c.units):
        if len(seeds) == 0:
            assert got["iters"][u] == 0 and np.isnan(got["p"][u]).all() and (got["node"][u] == -1).all() and np.isnan(got["score"][u]).all()
            continue
        p = got["p"][u]
        assert abs(p.sum() - 1.0) <= c.n * 2.0 ** -52, (name, u, p.sum() - 1.0)
        assert (p >= 0).all()
        if 0 < c.tol < 1:                                  # converged: the contraction's own bound
            off = np.abs(p - exact(c, seeds)).sum()
            assert off <= (1.0 - c.restart) / c.restart * c.tol + 1e-14, (name, u, off)
            assert got["iters"][u] <= M.iteration_bound(c.restart, c.tol), (name, u, got["iters"][u])
        elif c.tol == 0:
            assert got["iters"][u] == c.max_iter
        cand = np.setdiff1d(np.arange(c.n), seeds)
        k = min(c.n_add, len(cand))
        node = got["node"][u]
        assert (node[:k] >= 0).all() and (node[k:] == -1).all() and not np.isin(node[:k], seeds).any()
        s = got["score"][u]
        assert np.array_equal(bits(s[:k]), bits(p[node[:k]])) and np.isnan(s[k:]).all()
        assert all(s[i] > s[i + 1] or (s[i] == s[i + 1] and node[i] < node[i + 1]) for i in range(k - 1))
        assert k == len(cand) or s[k - 1] >= np.delete(p, np.concatenate([seeds, node[:k]])).max()


@pytest.mark.parametrize("name", ["classes", "star", "path", "n1025", "sizes", "ring", "k65", "lattice", "iter2", "strict"])
def test_the_array_form_is_the_literal_form_bit_for_bit(name):
    c, want = K.case(name), K.mirror(name)
    units = c.units[:3] if name != "sizes" else c.units
    got = M.table(c.rowptr, c.col, units, c.n_add, c.restart, c.tol, c.max_iter, literal=True)
    for f in ("p", "score"):
        assert np.array_equal(bits(got[f]), bits(want[f][:len(units)])), (name, f)
    assert np.array_equal(got["node"], want["node"][:len(units)]) and np.array_equal(got["iters"], want["iters"][:len(units)])


def test_every_case_has_the_property_it_was_built_for():
    c = K.case("classes")
    deg = np.diff(c.rowptr)
    assert tuple(deg[:9]) == K.CLASS_DEGREES and M.LONG_ROW in deg and M.LONG_ROW + 1 in deg and deg[9:].max() <= 12
    c = K.case("star")
    assert np.diff(c.rowptr)[0] == K.HUB_DEG >= 1150 > M.THREADS and 0 in c.units[0] and 0 not in c.units[1]
    assert K.mirror("star")["node"][1, 0] == 0             # ... and the hub is the best candidate of the unit beside it
    assert set(np.diff(K.case("path").rowptr)) == {1, 2}
    assert [K.case(f"n{n}").n for n in (1023, 1024, 1025, 2047, 2048, 2049)] == [1023, 1024, 1025, 2047, 2048, 2049]
    assert K.case("limit").n == M.MAX_NODES and K.case("n2049").n_add == M.MAX_ADD
    c = K.case("sizes")
    assert [len(u) for u in c.units[:4]] == [0, 1, c.n - 1, c.n] and c.n_add > c.n
    got = K.mirror("sizes")
    assert (got["node"][3] == -1).all() and got["iters"][3] > 0 and got["node"][2, 0] == 13 and (got["node"][2, 1:] == -1).all()
    assert len(K.case("wide").units[0]) == M.MAX_SEEDS and K.case("wide").n > M.MAX_ADD + 3 * M.THREADS
    assert K.case("one").n_add == 1
    for name in ("ring", "k65", "lattice", "iter1"):       # bit-equal candidates inside the first n_add, and across its end
        c, got = K.case(name), K.mirror(name)
        inside = across = 0
        for u, seeds in enumerate(c.units):
            s, p = got["score"][u], np.delete(got["p"][u], seeds)
            inside += int((bits(s[:-1]) == bits(s[1:])).sum())
            across += int((bits(p) == bits(s[-1:])).sum() > (bits(s) == bits(s[-1:])).sum())
        assert inside > 0 and across > 0, (name, inside, across)
    assert [K.case(f"iter{k}").max_iter for k in (1, 2, 30)] == [1, 2, 30] and all(K.case(f"iter{k}").tol == 0 for k in (1, 2, 30))
    assert (K.mirror("stop1")["iters"] == 1).all()
    c = K.case("strict")
    errs = M.walk(c.rowptr, c.col, c.units[0], c.restart, c.tol, c.max_iter)[2]
    assert errs[3] == c.tol and len(errs) == 5 and errs[4] < c.tol
    c, got = K.case("same"), K.mirror("same")
    assert all(np.array_equal(c.units[0], c.units[i]) for i in (2, 5)) and np.array_equal(bits(got["p"][0]), bits(got["p"][5]))
    assert len(K.case("many").units) > M.MAX_BLOCKS
    c = K.case("not_converged")
    assert (K.mirror("not_converged")["iters"] == c.max_iter).all()
    assert all(M.walk(c.rowptr, c.col, u, c.restart, c.tol, c.max_iter)[2][-1] >= c.tol for u in c.units)
    p, seeds, n_add = K.null_case("flat")
    got = M.null_stats(p[0], seeds[0], n_add, "z")
    assert (got["sd"][:50] == 0).all() and (got["z"][:50][~np.isin(np.arange(50), seeds[0])] == 0).all()
    assert (got["ge"][20:30] == p.shape[1] - 1).all() and np.isnan(got["z"][seeds[0]]).all()
    assert np.array_equal(bits(got["z"][120:130]), bits(got["z"][130:140])) and (p[0, 0, 120:130] != p[0, 0, 130:140]).all()
    assert [K.null_case(k)[0].shape[1] for k in ("r3", "r65")] == [3, 65]


def _toy():
    net = P.read_network(NET)
    sets = _sets_cli.load_seed_sets(SEEDS)
    return net, [net.node_set(sets[k]) for k in sorted(sets)]


def _outputs(rule):
    """every asserted output under `rule`: the cases' tables, the null's cases, the toy network's recovery"""
    out = []
    for name in SMALL:
        c = K.case(name)
        t = M.table(c.rowptr, c.col, c.units[:6], c.n_add, c.restart, c.tol, c.max_iter, rule)
        out += [t["node"], t["iters"], bits(t["score"]), bits(t["p"])]
    for name in K.NULL_CASES:
        p, seeds, n_add = K.null_case(name)
        for by in ("p", "z"):
            for s in range(len(seeds)):
                t = M.null_stats(p[s], seeds[s], n_add, by, rule)
                out += [bits(t["mean"]), bits(t["sd"]), bits(t["z"]), t["ge"], t["node"]]
    net, members = _toy()
    draws = diamond.holdout_draws(members, 0.34, 4, 3)
    out += list(M.recovery(net.rowptr, net.col, draws, 5, 0.75, 1e-6, 1000, rule))
    # the kept seeds' scores under the hold-out: what a wrong p0 changes even where the ranking survives it
    out += [bits(M.walk(net.rowptr, net.col, kept, 0.75, 1e-6, 1000, rule,
                        p0_size=len(kept) + len(held) if rule == "p0_unnormalised" else None)[0]) for reps in draws for kept, held in reps]
    return out


def test_every_ablation_changes_an_asserted_output():
    right = _outputs(None)
    for rule in M.ABLATIONS:
        wrong = _outputs(rule)
        assert len(wrong) == len(right)
        assert any(not np.array_equal(a, b) for a, b in zip(right, wrong)), rule


def test_recovery_on_the_toy_network_equals_a_plain_loop():
    net, members = _toy()
    n_add, repeats = 5, 4
    draws = diamond.holdout_draws(members, 0.34, repeats, 3)
    rec, held = M.recovery(net.rowptr, net.col, draws, n_add, 0.75, 1e-6, 1000)
    flat = [kept for reps in draws for kept, _ in reps]
    node = M.table(net.rowptr, net.col, flat, n_add, 0.75, 1e-6, 1000)["node"].reshape(len(draws), repeats, n_add)
    want = np.zeros_like(rec)
    for i, reps in enumerate(draws):
        for j, (_, gone) in enumerate(reps):
            want[i] += np.cumsum(np.isin(node[i, j], gone) & (node[i, j] >= 0))
    assert np.array_equal(rec, want) and rec.max() > 0 and held.tolist() == [sum(len(h) for _, h in reps) for reps in draws]
    assert (np.diff(rec, axis=1) >= 0).all() and (rec[:, -1] <= held).all()
