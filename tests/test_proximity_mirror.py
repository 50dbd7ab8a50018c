"""CPU: the conditions tests/test_gpu_proximity_ops.py rests on, established on tests/proximity_mirror.py alone with the inputs of
tests/proximity_cases.py: a case that loses its property, or a wrong rule that no case would show, fails here and not on the GPU.

The cases have their properties (each stated and asserted below): distances with two components, isolated nodes and n on both sides
of 512; 254 hops kept and 255 refused; `exhaust` with full and shrunk samples; ties over the ballot chunks, a unique centre, two
centres at positions 63 | 64; zero spread on the complete graph.  The draw-by-draw random_table agrees with the older vectorised
random_sets, pair_values with measures, and stats_sequential with numpy's mean / std within the GPU test's tolerance.

Every wrong rule of proximity_mirror.ABLATIONS changes an output the GPU test asserts, in the case ABLATION_CASE names.  For outputs
compared bit for bit "changes" is `not array_equal`; for toleranced ones (TOL_REL = 1e-12 relative) the change is measured in tolerances
and must be >= 1000:

    ablation          case          output it changes                                    margin
    first_centre      cycle_tied    centres, n_centres                                   bits (1 unit of 2)
    inner_self        sizes         inner                                                bits (7 units of 9)
    inner_single      sizes         inner of the one-member set                          bits (1 unit)
    stats_first64     sizes         inner, centres                                       bits (4 units: the sizes above 64)
    colmin_first64    grid          separation d                                         bits (5 of 11 pairs: those with ns > 64)
    kernel_max_size   grid          kernel d (toleranced)                                smallest |change| / tolerance 2.2e9
    redraws_19        exhaust       random-set nodes / sizes  (n_random = 64 suffices)   bits (samples 46, 57 of set 0, side 0)
    redraws_21        exhaust       random-set nodes / sizes  (n_random = 64 suffices)   bits (samples 6, 19, 35 of set 0, side 0)
    add_taken         exhaust       random-set nodes / sizes                             bits (the 49 shrunk samples of set 0)
    unsorted          exhaust       random-set nodes                                     bits (all 64 samples of set 0)
    pair_sample0      grid          m of every measure                                   bits (all 11 pairs)
    sample_sd         grid          s (toleranced)                                       smallest |change| / tolerance 1.2e11
    drop_p0           batch7        out rows past the first batch                        bits (rows 3 .. 6 never written)

The smallest ratio over the toleranced rows is 2.2e9 (kernel_max_size: ln(260 / 257) = 0.0116 on a value near 5)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proximity_cases as K  # noqa: E402
import proximity_mirror as M  # noqa: E402

TOL_REL = 1e-12              # tests/test_gpu_proximity_ops.py: s, pval and the kernel measure within this of the mirror (abs 1e-11 on z)
SENSITIVITY = 1000           # a wrong rule moves a toleranced output by at least this many tolerances


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def flat(table):
    return [x for rows in table for x in rows]


# ---- graphs and distances ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["split_511", "split_512", "split_513"])
def test_split_graphs_have_two_components_isolated_nodes_and_a_finite_diameter(name):
    g, D = K.graph(name), K.distances(name)
    a, b = g.parts
    assert g.n == int(name[-3:]) and len(g.isolated) >= 10 and len(a) > 64 and len(b) > 64
    assert (D[np.ix_(a, b)] == 255).all() and (D[np.ix_(a, a)] < 255).all() and (D[np.ix_(b, b)] < 255).all()
    iso = D[g.isolated]
    assert (iso == 255).sum() == len(g.isolated) * (g.n - 1) and (np.diag(D) == 0).all()
    assert (np.diff(g.rowptr)[g.isolated] == 0).all()
    assert 3 <= K.diameter(name) < 255 and D.max() == 255
    assert np.array_equal(D, D.T)


def test_distance_edge_graphs():
    assert K.graph("single").n == 1 and len(K.graph("single").col) == 0 and K.distances("single").tolist() == [[0]]
    assert K.diameter("single") == 0
    star = K.graph("star_600")
    assert np.diff(star.rowptr)[K.STAR_HUB] == 599 > 512 and K.diameter("star_600") == 2
    D = K.distances("path_255")
    assert K.diameter("path_255") == 254 and D[0, 254] == D[254, 0] == 254 and D.max() == 254
    g = K.graph("path_256")
    assert g.n == 256 and len(g.col) == 510                      # 255 hops end to end: one more than a byte holds beside "unreachable"
    for name in ("web_300", "web_132", "web_4100"):
        assert K.distances(name).max() < 255, name               # connected


# ---- random sets ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.RANDOM_CASES)
@pytest.mark.parametrize("side", [0, 1])
def test_random_table_is_the_vectorised_mirror_draw_by_draw(name, side):
    c = K.random_case(name)
    table = K.random_table(name, side)
    for s, members in enumerate(c.sets):
        assert np.array_equal(table[s][0], members) and len(table[s]) == c.n_random + 1
        want = M.random_sets(members, c.node_bin, c.bin_list, c.seed, side, s, c.n_random)
        for k, w in enumerate(want):
            assert np.array_equal(table[s][k + 1], w), (s, k)
        for x in table[s]:
            assert len(x) <= c.max_size and (np.diff(x) > 0).all()
            assert np.array_equal(np.bincount(c.node_bin[x], minlength=4) <= np.bincount(c.node_bin[members], minlength=4), np.ones(4, bool))


def test_exhaust_has_full_and_shrunk_samples():
    c = K.random_case("exhaust")
    assert len(c.sets[0]) == 32 == len(c.bin_list[0]) and len(c.bin_list[1]) == 100 and len(c.sets[2]) == 0
    assert len(c.sets) * (c.n_random + 1) > 256                   # a second block of random_sets_kernel
    for side, lo, full in ((0, 29, 15), (1, 30, 16)):
        sizes = np.array([len(x) for x in K.random_table("exhaust", side)[0][1:]])
        print(f"side {side}: sizes {np.bincount(sizes)[lo:]} from {lo}")
        assert sizes.min() == lo and sizes.max() == 32 and (sizes == 32).sum() == full and len(sizes) == 64
    a, b = K.random_table("exhaust", 0), K.random_table("exhaust", 1)
    assert any(not np.array_equal(x, y) for x, y in zip(flat(a)[1:], flat(b)[1:]))           # the sides draw differently


def test_mixed_case_has_its_sets():
    c = K.random_case("mixed")
    assert [len(b) for b in c.bin_list] == [1, 30, 40, 61] and c.sets[0].tolist() == [17]
    assert len(c.sets[1]) > 0 and len(c.sets[2]) == 0 and len(c.sets[3]) > 0
    assert sorted(set(c.node_bin[c.sets[3]].tolist())) == [1, 2, 3]
    for side in (0, 1):
        t = K.random_table("mixed", side)
        assert all(x.tolist() == [17] for x in t[0]) and all(len(x) == 0 for x in t[2])
        assert all(17 in x for x in t[4])
    assert all(len(rows) == 1 for rows in K.random_table("n_random_0", 0))
    a, b = K.random_table("mixed", 0), K.random_table("mixed", 1)
    assert any(not np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))


# ---- set stats --------------------------------------------------------------------------------------------------------------------------

def test_set_cases_have_their_properties():
    table, max_size = K.set_table("sizes")
    assert tuple(len(x) for x in flat(table)) == K.SET_SIZES and max_size > 200
    st = flat(K.set_mirror("sizes"))
    assert st[0] == (0.0, st[0][1], 0) and len(st[0][1]) == 0
    assert st[1][0] == 0.0 and st[1][2] == 1 and st[2][0] >= 1.0 and st[2][2] == 2            # two members: both tied
    for x, (inner, c, nc) in zip(flat(table), st):
        assert nc == len(c) and set(c.tolist()) <= set(x.tolist()) and (np.diff(c) > 0).all()
        assert inner == 0.0 or 1.0 <= inner < 255
    late = [int(np.searchsorted(x, c[0])) for x, (_, c, _) in zip(flat(table), st) if len(x) > 64]
    print("position of the first centre in the sets above 64 members:", late)
    assert max(late) >= 64                                                                    # a centre a 64-member kernel would miss
    (inner, c, nc), = flat(K.set_mirror("cycle_tied"))[:1]
    assert nc == 150 and np.array_equal(c, np.arange(150)) and inner == 1.0
    a, b = flat(K.set_mirror("complete_tied"))[:2]
    assert a[2] == 129 and a[0] == 1.0 and b[2] == 65 and b[0] == 1.0
    hub, leaves = flat(K.set_mirror("star"))[:2]
    x = flat(K.set_table("star")[0])[0]
    assert hub[1].tolist() == [K.STAR_HUB] and int(np.searchsorted(x, K.STAR_HUB)) == 70 and hub[0] == 1.0
    assert leaves[2] == 70 and leaves[0] == 2.0


def test_tie_63_64_has_exactly_those_two_centres():
    x = flat(K.set_table("tie_63_64")[0])[0]
    inner, c, nc = flat(K.set_mirror("tie_63_64"))[0]
    assert nc == 2 and c.tolist() == [K.DS_A, K.DS_B] and len(x) == 102
    assert x[63] == K.DS_A and x[64] == K.DS_B
    tot = K.distances("double_star")[np.ix_(x, x)].astype(np.int64).sum(axis=1)
    assert tot[63] == tot[64] == 151 and np.sort(tot)[2] == 251


# ---- score ------------------------------------------------------------------------------------------------------------------------------

def test_score_cases_have_their_shapes():
    g = K.score_case("grid")
    assert tuple(len(r[0]) for r in g.ftab) == K.FROM_SIZES and tuple(len(r[0]) for r in g.ttab) == K.TO_SIZES
    assert set(i for i, _ in g.pairs) == set(range(5)) == set(j for _, j in g.pairs)
    assert (len(g.pairs) * g.n_samples) % 4 == 2                                              # a tail block with two idle waves
    assert any(len(r[2]) != len(r[0]) for r in g.ttab) and len(g.ttab[3][2]) == 64 and len(g.ftab[3][2]) == 64
    assert g.to_max_size > 257 and g.from_max_size > 130
    a = K.score_case("grid_all")
    assert a.pairs is None and (len(K.pair_list(a)) * a.n_samples) % 4 != 0
    u = K.score_case("pairs_unordered").pairs
    assert len(set(u)) < len(u) and u != sorted(u)
    b = K.score_case("lds_4096")
    assert b.to_max_size == 4096 == len(b.ttab[0][0]) and tuple(len(x) for x in b.ttab[0]) == K.BIG_TO and K.graph(b.graph).n == 4100
    e = K.score_case("exhaust")
    fs = np.array([len(x) for x in e.ftab[0]])
    ts = np.array([len(x) for x in e.ttab[0]])
    assert (fs[1:] < fs[0]).any() and (fs[1:] == fs[0]).any() and (ts[1:] < ts[0]).any() and (fs != ts).any()
    assert K.score_case("batch7").pairs == K.GRID_PAIRS[:7]


@pytest.mark.parametrize("name", K.SCORE_CASES)
def test_no_toleranced_comparison_hangs_on_cancellation(name):
    """the kernel measure's values carry a rounding error of a few 1e-15 (values of 2 to 7, sums of up to 4096 terms in another order);
    its spread is >= 1e-2 in every case, so s, z and pval inherit at most about 1e-13 -- a tenth of the GPU test's tolerance.  The
    integer measures' values are exact on both sides: their spread is exactly 0 or far above rounding"""
    c, out = K.score_case(name), K.score_mirror(name)
    live = out[~np.isnan(out[:, 0, 0])]
    if "kernel" in c.which:
        print(f"{name}: kernel spread {live[:, 2, 2].min():.3g} .. {live[:, 2, 2].max():.3g}, d {live[:, 2, 0].min():.3g} .. {live[:, 2, 0].max():.3g}")
        assert live[:, 2, 2].min() >= 1e-2 and 1.0 <= live[:, 2, 0].min() and live[:, 2, 0].max() <= 8.0
    s = live[:, [0, 1, 3, 4], 2]
    assert ((s == 0) | (s >= 1e-3)).all()


def test_empties_are_nan_in_exactly_their_pairs():
    c = K.score_case("empties")
    out = K.score_mirror("empties")
    nan_pair = np.array([i == 1 or j == 0 for i, j in K.pair_list(c)])
    assert nan_pair.sum() == 5 and len(nan_pair) == 9
    assert np.isnan(out[nan_pair]).all() and out[nan_pair].shape == (5, 5, 5) and np.isfinite(out[~nan_pair]).all()


def test_sd0_case_has_zero_spread():
    c = K.score_case("sd0")
    v = K.score_values("sd0")
    T, S = np.concatenate(flat(c.ftab)), np.concatenate(flat(c.ttab))
    assert T.max() < 20 <= S.min() and "kernel" not in c.which
    assert (v[:, [0, 1, 3], :] == 1.0).all() and (v[:, [2, 4], :] == 0.0).all()
    out = K.score_mirror("sd0")
    assert (out[:, :, 2] == 0).all() and (out[:, :, 3] == 0).all() and (out[:, :, 4] == 0.5).all()
    assert any(not np.array_equal(x, rows[0]) for rows in c.ftab for x in rows[1:])           # the random sets do differ from the set


@pytest.mark.parametrize("name", ["grid", "exhaust"])
def test_pair_values_are_the_older_measures_and_stats_sequential_is_numpy(name):
    c = K.score_case(name)
    d = K.dist(c.graph)
    v = K.score_values(name)
    out = K.score_mirror(name)
    worst = 0.0
    for q, (i, j) in enumerate(K.pair_list(c)):
        for r in (0, 1, c.n_samples - 1):
            want = M.measures(d, c.ftab[i][r], c.ttab[j][r])
            assert np.array_equal(bits(np.array([want[m] for m in M.MEASURES])), bits(v[q, :, r])), (q, r)
        for k, m in enumerate(M.MEASURES):
            ref = np.array(M.stats(v[q, k, 0], v[q, k, 1:]))
            got = out[q, k, 1:]
            if ref[1] > 1e-9:                                     # numpy sums pairwise: near-zero spreads are rounding on both sides
                worst = max(worst, np.max(np.abs(got[[0, 1, 3]] - ref[[0, 1, 3]]) / np.abs(ref[[0, 1, 3]])))
                assert abs(got[2] - ref[2]) <= 1e-11
    print(f"{name}: max relative |sequential - numpy| over m, s, pval {worst:.3g}")
    assert worst <= TOL_REL


# ---- every wrong rule shows ---------------------------------------------------------------------------------------------------------------

def _set_flat(name, ablate=None):
    st = flat(K.set_mirror(name, ablate))
    return np.array([s[0] for s in st]), [s[1] for s in st], np.array([s[2] for s in st])


@pytest.mark.parametrize("ablate", sorted(M.ABLATIONS))
def test_each_wrong_rule_changes_an_asserted_output(ablate):
    kind, name = K.ABLATION_CASE[ablate]
    if kind == "set":
        ri, rc, rn = _set_flat(name)
        wi, wc, wn = _set_flat(name, ablate)
        changed = (bits(ri) != bits(wi)) | (rn != wn) | np.array([not np.array_equal(a, b) for a, b in zip(rc, wc)])
        print(f"{ablate} on {name}: {int(changed.sum())} of {len(changed)} units change")
        assert changed.any()
        if ablate == "inner_single":
            assert np.flatnonzero(changed).tolist() == [K.SET_SIZES.index(1)]
        if ablate == "stats_first64":
            assert np.flatnonzero(changed).tolist() == [i for i, k in enumerate(K.SET_SIZES) if k > 64]
    elif kind == "random":
        c = K.random_case(name)
        right, wrong = K.random_table(name, 0)[0], K.random_table(name, 0, ablate)[0]
        diff = [k for k in range(c.n_random + 1) if not np.array_equal(right[k], wrong[k])]
        print(f"{ablate} on {name}: samples of set 0 that change {diff} at n_random = {c.n_random}")
        assert diff and 0 not in diff
    elif ablate == "drop_p0":
        right, wrong = K.score_mirror(name, batch=3, fill=-77.0), K.score_mirror(name, ablate, batch=3, fill=-77.0)
        assert np.array_equal(bits(right), bits(K.score_mirror(name)))
        assert (wrong[3:] == -77.0).all() and not np.array_equal(bits(right[:3]), bits(wrong[:3]))
    else:
        right, wrong = K.score_mirror(name), K.score_mirror(name, ablate)
        exact = {"colmin_first64": (4, 0), "pair_sample0": (slice(None), 1)}
        if ablate in exact:
            k, f = exact[ablate]
            moved = np.array([not np.array_equal(bits(right[q, k, f]), bits(wrong[q, k, f])) for q in range(len(right))])
            print(f"{ablate} on {name}: {int(moved.sum())} of {len(moved)} pairs change")
            assert moved.all() if ablate == "pair_sample0" else moved.any()
        else:
            k, f = {"kernel_max_size": (2, 0), "sample_sd": (slice(None), 2)}[ablate]
            a, b = right[:, k, f], wrong[:, k, f]
            ratio = np.abs(a - b) / (TOL_REL * np.abs(a))
            print(f"{ablate} on {name}: smallest |change| / tolerance {ratio.min():.3g}")
            assert ratio.min() >= SENSITIVITY


def test_ablation_table_names_every_wrong_rule_and_a_case():
    assert set(K.ABLATION_CASE) == set(M.ABLATIONS)
    for kind, name in K.ABLATION_CASE.values():
        assert name in {"set": K.SET_CASES, "random": K.RANDOM_CASES, "score": K.SCORE_CASES}[kind]
