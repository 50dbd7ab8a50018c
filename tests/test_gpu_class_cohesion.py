"""GPU: csrc/class_cohesion.hip (gss_pair_sums_lists, gss_pair_sums_random) through classes.pair_sums / random_pair_sums / class_cohesion,
against the numpy mirror (class_cohesion_mirror.py).

Permutations are integers: equal to the mirror's np.lexsort((i, key)) exactly.
Accuracy: a sum T of K = m (m - 1) / 2 non-negative terms, added in any order, is within gamma(K - 1) T of the exact sum, gamma(k) = k u /
(1 - k u), u = 2^-53; the mirror's math.fsum is the reference.  A dropped or doubled term moves T by about 1 / K relative, orders above.
Bits: the kernels' order of additions is stated in include/gssgcn.h and restated term by term in the mirror (ordered_prefixes); the device's
sums equal it bit for bit, and hence each other under every regrouping of a call."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import class_cohesion_mirror as M  # noqa: E402
from conftest import record_measured  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd import classes as K  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES_N = (2, 3, 64, 65, 257, 1331, 4096)
_MATRICES = {}


def matrix(n):
    """a symmetric non-negative matrix of n rows -> (host, device); made once per n and never written"""
    if n not in _MATRICES:
        rng = np.random.RandomState(1000 + n)
        h = rng.rand(n, n)
        h = h + h.T
        np.fill_diagonal(h, 0.0)
        _MATRICES[n] = (h, torch.from_numpy(h).cuda())
    return _MATRICES[n]


def host(t):
    return t.cpu().numpy()


# ---- permutations --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES_N)
def test_permutations_equal_the_mirror(n):
    _, d = matrix(n)
    for seed, P, s0, width in ((0, 1, 0, n), (0, 7, 12345, n), (2 ** 63 + 5, 7, 0, n), (0, 300, 12345, min(n, 40)), (2 ** 63 + 5, 300, 0, min(n, 40))):
        _, perm = K.random_pair_sums(d, [width], P, seed=seed, first=s0, perms=True)
        perm = host(perm)
        assert perm.shape == (P, width)
        for s in range(P):
            assert np.array_equal(perm[s], M.permutation(seed, s0 + s, n)[:width]), (n, seed, P, s0, s)


# ---- accuracy and the stated order ---------------------------------------------------------------------------------------------------

def size_sets(n):
    sets = [[2], [n], sorted({m for m in (2, 3, 63, 64, 65, n) if 2 <= m <= n}), list(range(2, min(n, 40) + 1))]
    return [s for k, s in enumerate(sets) if s not in sets[:k]]


@pytest.mark.parametrize("n", SIZES_N)
def test_random_sums_against_fsum_and_the_stated_order(n):
    h, d = matrix(n)
    P, s0, seed = (2, 5, 3) if n == 4096 else (3, 5, 3)
    worst = 0.0
    for sizes in size_sets(n):
        if n == 4096 and sizes == [n]:
            continue      # m = 4096 is in the mixed set below; the mirror is slow there
        sums, perm = K.random_pair_sums(d, sizes, P, seed=seed, first=s0, perms=True)
        sums, perm = host(sums), host(perm)
        for s in range(P):
            exact = M.fsum_prefixes(h, perm[s], sizes)
            for m, got, want in zip(sizes, sums[s], exact):
                pairs = m * (m - 1) // 2
                bound = M.gamma(pairs - 1) * want
                share = abs(got - want) / bound if bound else float(got != want)
                print(f"n={n} sizes={len(sizes)} s={s} m={m} |got - fsum| / bound = {share:.3g}")
                worst = max(worst, share)
                assert abs(got - want) <= bound, (n, s, m, got, want, bound)
            assert np.array_equal(sums[s], M.ordered_prefixes(h, perm[s], sizes)), (n, s, sizes)
    record_measured(f"class_cohesion.random_sums[n={n}]", worst_share_of_bound=worst)


def test_list_sums_against_fsum_and_the_stated_order():
    h, d = matrix(1331)
    rng = np.random.RandomState(4)
    lists = [rng.permutation(1331)[:m] for m in (2, 3, 28, 63, 64, 65, 66, 111, 266, 1331)] + [rng.randint(0, 1331, 1500)]     # the last: repeats, two chunks
    got = host(K.pair_sums(d, lists))
    worst = 0.0
    for a, g in zip(lists, got):
        want, pairs = M.fsum_pairs(h, a), len(a) * (len(a) - 1) // 2
        bound = M.gamma(pairs - 1) * want
        worst = max(worst, abs(g - want) / bound if bound else float(g != want))
        assert abs(g - want) <= bound, (len(a), g, want, bound)
        assert g == M.ordered_pairs(h, a), len(a)
    record_measured("class_cohesion.list_sums", worst_share_of_bound=worst)


# ---- bit-equality --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (65, 1331))
def test_sums_do_not_depend_on_how_a_call_is_cut(n):
    h, d = matrix(n)
    sizes = sorted({2, 3, 17, 64, 65, min(n, 266)})
    P, s0 = 300, 40
    whole, perm = K.random_pair_sums(d, sizes, P, seed=9, first=s0, perms=True)
    again = K.random_pair_sums(d, sizes, P, seed=9, first=s0)
    assert torch.equal(whole, again)                                                         # run to run
    for k, m in enumerate(sizes):                                                            # a size alone
        alone = K.random_pair_sums(d, [m], P, seed=9, first=s0)
        assert torch.equal(alone[:, 0], whole[:, k]), m
    parts = [K.random_pair_sums(d, sizes, c, seed=9, first=s0 + f) for f, c in ((0, 1), (1, 99), (100, 200))]
    assert torch.equal(torch.cat(parts), whole)                                              # samples in chunks through `first`
    perm = host(perm)
    picks = [(s, k) for s in (0, 1, 150, 299) for k in range(len(sizes))]
    lists = [perm[s][:sizes[k]] for s, k in picks]
    by_list = K.pair_sums(d, lists)                                                          # the lists' entry point on the same ordered sets
    assert torch.equal(by_list, torch.stack([whole[s, k] for s, k in picks]))
    view = torch.zeros(n, n + 5, dtype=torch.float64, device="cuda")[:, :n]                  # a leading dimension above n
    view.copy_(d)
    assert view.stride(0) == n + 5
    assert torch.equal(K.random_pair_sums(view, sizes, 7, seed=9, first=s0), whole[:7])
    assert torch.equal(K.pair_sums(view, lists), by_list)


def test_a_list_alone_and_among_300_and_short_lists():
    h, d = matrix(257)
    rng = np.random.RandomState(6)
    lists = [rng.permutation(257)[:rng.randint(0, 120)] for _ in range(300)]
    lists[0], lists[1], lists[299] = [], [5], [7]
    every = K.pair_sums(d, lists)
    assert torch.equal(every, K.pair_sums(d, lists))
    for c in (2, 3, 150, 298):
        assert torch.equal(K.pair_sums(d, [lists[c]]), every[c:c + 1]), c
    got = host(every)
    for c, a in enumerate(lists):
        if len(a) < 2:
            assert got[c] == 0.0 and not np.signbit(got[c]), c
    assert host(K.pair_sums(d, [[], [3], []])).tolist() == [0.0, 0.0, 0.0]
    assert K.pair_sums(d, []).shape == (0,)
    assert host(K.pair_sums(h, [lists[150]]))[0] == got[150]                                 # a host matrix is uploaded


# ---- planted structure ---------------------------------------------------------------------------------------------------------------

def test_planted_clusters_are_found():
    clusters = [list(range(0, 10)), list(range(10, 24)), list(range(24, 44))]
    n, P, seed = 44, 999, 1
    cluster_of = np.repeat(np.arange(3), [len(c) for c in clusters])
    h = np.where(cluster_of[:, None] == cluster_of[None, :], 0.1, 1.0)
    np.fill_diagonal(h, 0.0)
    scattered = [0, 4, 8, 11, 15, 19, 22, 25, 29, 33, 37, 41]
    # on the CPU first: no sampled set of a class's size lies inside one cluster, so every random sum holds a 1.0 where the class has 0.1
    for s in range(P):
        perm = M.permutation(seed, s, n)
        for c in clusters:
            assert len(set(cluster_of[perm[:len(c)]])) > 1, (s, len(c))
    rec = K.class_cohesion(torch.from_numpy(h).cuda(), clusters + [scattered], P, seed=seed)
    for r, c in zip(rec, clusters):
        assert r["n_drugs"] == len(c) and r["p"] == 1 / 1000 and r["z"] < 0
        assert abs(r["mean_distance"] - 0.1) <= 0.1 * M.gamma(r["n_pairs"]) * 2
    assert rec[3]["p"] > 0.05 and rec[3]["n_drugs"] == 12


def test_class_cohesion_equals_its_parts():
    h, d = matrix(257)
    classes = {"a": list(range(0, 30)), "b": list(range(20, 27)), "c": [256, 3, 77], "d": list(range(100, 130))}
    rec, sizes, null = K.class_cohesion(d, classes, 50, seed=4, return_null=True)
    assert sizes == [3, 7, 30] and null.shape == (50, 3) and [r["class"] for r in rec] == list(classes)
    assert np.array_equal(null, host(K.random_pair_sums(d, sizes, 50, seed=4)))
    observed = host(K.pair_sums(d, list(classes.values())))
    want = K.cohesion_stats(observed, [30, 7, 3, 30], sizes, null)
    for r, w in zip(rec, want):
        assert all(r[k] == w[k] or (r[k] != r[k] and w[k] != w[k]) for k in w)


# ---- refusals: every one on the host or in the list check, before a kernel reads through a bad argument ----------------------------

def test_refusals_by_name():
    h, d = matrix(65)
    with pytest.raises(_lib.GssError, match=r"pair_sums_random: n=1 is outside \[2, 4096\]"):
        K.random_pair_sums(np.zeros((1, 1)), [2], 1)
    lib = _lib.load()
    small = torch.zeros(4, dtype=torch.float64, device="cuda")
    sizes = torch.tensor([2], dtype=torch.int32, device="cuda")
    out = torch.full((1,), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.gss_pair_sums_random(4097, small.data_ptr(), 4097, 0, 0, 1, 1, sizes.data_ptr(), out.data_ptr(), 0, _lib.current_stream())
    assert rc == -22 and "pair_sums_random: n=4097 is outside [2, 4096]" in lib.gss_last_error().decode()
    for bad, words in (([3, 3], r"sizes\[1\] = 3 is not above sizes\[0\] = 3"), ([1], r"sizes\[0\] = 1 is outside \[2, n=65\]"),
                       ([66], r"sizes\[0\] = 66 is outside \[2, n=65\]"), ([5, 4], r"sizes\[1\] = 4 is not above")):
        with pytest.raises(_lib.GssError, match=words):
            K.random_pair_sums(d, bad, 3)
    with pytest.raises(_lib.GssError, match=r"P=0 samples must be >= 1"):
        K.random_pair_sums(d, [2], 0)
    with pytest.raises(_lib.GssError, match=r"s0=-1"):
        K.random_pair_sums(d, [2], 1, first=-1)
    with pytest.raises(_lib.GssError, match=r"outside \[0, 2\^31\]"):
        K.random_pair_sums(d, [2], 2, first=2 ** 31 - 1)
    with pytest.raises(_lib.GssError, match=r"pair_sums_lists: idx\[4\] = 65 is outside \[0, n=65\)"):
        K.pair_sums(d, [[1, 2, 3], [0, 65, 4]])
    with pytest.raises(_lib.GssError, match=r"pair_sums_lists: idx\[0\] = -1 is outside"):
        K.pair_sums(d, [[-1, 2]])
    assert host(out)[0] == -7.0
    torch.cuda.synchronize()
    bad = h.copy()
    bad[9, 40] = bad[40, 9] = np.nan
    labels = [f"DB{i:05d}" for i in range(65)]
    for call in (lambda: K.pair_sums(bad, [[1, 2]], labels=labels), lambda: K.random_pair_sums(bad, [2], 1, labels=labels),
                 lambda: K.class_cohesion(bad, [[1, 2]], 5, labels=labels)):
        with pytest.raises(ValueError, match="a distance of 'DB00009' is NaN"):
            call()
    with pytest.raises(ValueError, match="a distance of 'row 9' is NaN"):
        K.pair_sums(bad, [[1, 2]])
    with pytest.raises(ValueError, match="must list at least 2 drugs, each once"):
        K.class_cohesion(d, [[1, 1]], 5)
