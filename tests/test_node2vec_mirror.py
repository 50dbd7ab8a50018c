"""CPU: the conditions tests/test_gpu_node2vec_ops.py rests on, established on tests/node2vec_mirror.py alone with the inputs of
tests/node2vec_cases.py: a seed that loses one fails here, not on the GPU.

Walks.  exact_transitions (the law from its definition) agrees with the probabilities the reference walker's own alias tables gave
(the committed fixture, fp32 storage) below 1e-6; the mirror's walks at (p, q) = (1, 64), (1e-6, 1), (1, 16) on a 12-node digraph pass a
chi-square test against that law in every state (measured minimum p-values 2.3e-3, 5.8e-2, 3.4e-2 over 42, 41, 42 states against a
bound of 1e-3 / states = 2.4e-5) -- the first comparison of the mirror's direct-draw branch with anything; the fallback cases take that
branch 103, 1,762 and 8,895 times where the three (p, q) of tests/test_gpu_node2vec.py take it 0 times; the vectorised direct draw
picks what the entry-by-entry one picks; the hub row's prefix sums hold ties and the binary search probes them.

SGNS.  Every case has the property it is named for (from the mirror's stats); in every case the fp64 mirror's |f| stays >= 1e-3 clear
of the skip threshold 6 and the fp32 mirror takes the same decisions, so no comparison hangs on a coin toss; each wrong rule of
node2vec_mirror.ABLATIONS moves the fp64 result of its case by far more than the GPU comparison's bound allows:

    ablation        case            max |wrong - right|   / d32(case)     (d32 = max |fp32 mirror - fp64 mirror|)
    keep_lt         keep_boundary   2.4e-2                4.6e4
    bisect_right    table_ties      2.2e-1                4.0e5
    tail_tokens     long_80         1.6e-1                2.3e5
    window_hi       window_1        8.3e-2                2.1e5
    last_negative   negative_1      9.3e-2                3.7e5
    neg_eq_center   dims_64         3.9e-2                6.8e4
    alpha_epoch     epochs_3_e1     5.9e-2                8.5e4
    f_skip          f_skip          3.7e-1                2.3e5

against a required 100 x 8 = 800 (8 is the margin of the GPU comparison, in units of d32).  d32 itself is 2.6e-7 to 2.4e-6 on the
unit-scale cases and 1.7e-9 on `partition`, whose result does not depend on the order of its sentences (run here in reverse)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import node2vec_cases as K  # noqa: E402
import node2vec_mirror as M  # noqa: E402

MARGIN = 8                   # tests/test_gpu_node2vec_ops.py: device within MARGIN x d32 of the fp64 mirror
SENSITIVITY = 100            # every wrong rule at least this many bounds away
FEW_NEGATIVES = ("negative_1", "degenerate_sentences", "partition")      # too few draws for 100 negatives to equal the center


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.mark.parametrize("case", [0, 1])
def test_exact_transitions_agree_with_the_reference_walkers_tables(case):
    z = np.load(os.path.join(HERE, "golden", "node2vec_msi_small.npz"))
    fix = {k: z[k] for k in z.files}
    _, adj, names = M.msi_small_graph()
    assert list(fix["names"]) == names
    ref1, ref2 = M.fixture_transitions(fix, case)
    got1, got2 = M.exact_transitions(adj, float(fix["p"][case]), float(fix["q"][case]))
    assert set(ref1) == set(got1) and set(ref2) == set(got2)
    worst = 0.0
    for ref, got in ((ref1, got1), (ref2, got2)):
        for state, probs in ref.items():
            assert set(probs) == set(got[state]), state
            worst = max(worst, max(abs(pr - got[state][x]) for x, pr in probs.items()))
    print(f"case {case}: {len(ref1)} + {len(ref2)} states, max |exact - fixture| {worst:.3g}")
    assert worst < 1e-6


@pytest.mark.parametrize("name", K.TINY_CASES)
def test_mirror_walks_at_extreme_pq_follow_the_exact_law(name):
    c = K.walk_case(name)
    adj = c.adj()
    w, ln, stats = K.mirror_walks(name)
    pv, impossible = M.transition_chi2(w, ln, laws=M.exact_transitions(adj, c.p, c.q), n=adj.shape[0])
    print(f"{name}: {len(pv)} states, min p {pv.min():.3g} (bound {1e-3 / len(pv):.3g}), {stats['direct_draws']} direct draws of {stats['steps']} steps")
    assert impossible == 0
    assert len(pv) >= 35, len(pv)
    assert pv.min() > 1e-3 / len(pv), (pv.min(), len(pv))      # Bonferroni; with 40 states a share-below-0.01 rule hangs on one state
    assert stats["direct_draws"] >= 50


def test_direct_draws_happen_in_the_fallback_cases_and_never_at_the_suites_pq():
    for name in K.FALLBACK_CASES + ["hub_ties_q64"]:
        stats = K.mirror_walks(name)[2]
        print(name, stats)
        assert stats["direct_draws"] >= 50, (name, stats)
    c = K.walk_case(K.FALLBACK_CASES[0])
    for p, q in K.SUITE_PQ:                                    # the gap this closes: the older tests never leave the rejection loop
        stats = {}
        M.walks(c.adj(), c.nw, c.L, p, q, c.seed, stats=stats)
        assert stats["direct_draws"] == 0 and stats["steps"] > 10000, (p, q, stats)


@pytest.mark.parametrize("name", ["fallback_q16", "fallback_q64", "hub_ties_q64"])
def test_vectorised_direct_draw_picks_what_the_entry_by_entry_one_picks(name):
    c = K.walk_case(name)
    w, ln, _ = K.mirror_walks(name)
    w2, ln2 = M.walks(c.adj(), c.nw, c.L, c.p, c.q, c.seed, scalar_direct=True)
    assert np.array_equal(w, w2) and np.array_equal(ln, ln2)


def test_hub_row_has_tied_prefix_sums_and_the_search_meets_them():
    a = M.csr(K.hub_graph())
    b, e = a.indptr[K.HUB], a.indptr[K.HUB + 1]
    cum = M.row_prefix(a)[b:e]
    assert e - b >= 5000 and a.data[b:e].max() / a.data[b:e].min() > 1e17
    assert (np.diff(cum) == 0).sum() >= 100 and (np.diff(cum) >= 0).all()
    for name in ("hub_ties_pq", "hub_ties_q64"):
        w, ln, stats = K.mirror_walks(name)
        assert stats["prefix_ties"] >= 1, (name, stats)
        assert (w[:, 1:] == K.HUB).sum() >= 100                # the hub's row is left often, from many previous nodes
    assert K.mirror_walks("hub_ties_pq")[2]["direct_draws"] == 0


def test_walk_edge_cases_have_their_shapes():
    for name, count in (("walks_255", 255), ("walks_256", 256), ("walks_257", 257)):
        w, ln, _ = K.mirror_walks(name)
        assert len(w) == count and (ln < w.shape[1]).any() and (ln == w.shape[1]).any()
    w, ln, _ = K.mirror_walks("len_1")
    assert w.shape[1] == 1 and (ln == 1).all() and (w >= 0).all()
    w, ln, stats = K.mirror_walks("len_2")
    assert set(ln.tolist()) == {1, 2} and stats["direct_draws"] == 0
    w, ln, _ = K.mirror_walks("single_self_loop")
    assert (w == 0).all() and (ln == 5).all()
    w, ln, _ = K.mirror_walks("single_no_edge")
    assert (w[:, 0] == 0).all() and (w[:, 1:] == -1).all() and (ln == 1).all()
    assert M.csr(K.walk_case("single_no_edge").adj()).nnz == 0


@pytest.mark.parametrize("name", K.SERIAL_CASES)
def test_sgns_case_has_its_property_and_stable_branches(name):
    c = K.sgns_case(name)
    s0, s1, st = K.sgns_mirror(name, np.float64)
    _, _, st32 = K.sgns_mirror(name, np.float32)
    f, f32 = np.array(st["f_abs"]), np.array(st32["f_abs"])
    gap = np.abs(f - 6).min()
    kept_len = np.array(list(st["kept_len"].values()))
    kept, dropped = np.array(st["kept_pos"]), np.array(st["dropped_pos"])
    moved = max(np.abs(s0 - c.syn0).max(), np.abs(s1 - c.syn1).max())
    print(f"{name}: {st['pairs']} pairs, {len(f)} decisions ({int((f >= 6).sum())} skipped), min ||f| - 6| {gap:.3g}, "
          f"{st['neg_eq_center']} negatives = center, d32 {K.d32(name):.3g}, moved {moved:.3g}")
    assert gap >= 1e-3 and len(f) == len(f32) and np.array_equal(f < 6, f32 < 6)
    assert moved >= c.moved_min and K.d32(name) > 0 and K.d32(name) < 1e-5
    assert st["pairs"] >= 100 and len(f) == st["pairs"] * (1 + c.negative) - st["neg_eq_center"]
    if name not in FEW_NEGATIVES:
        assert st["neg_eq_center"] >= 100
    if name.startswith("long_"):
        L = c.walks.shape[1]
        cuts = [64] if L == 80 else [64, 128]
        for cut in cuts:                                        # the ballot compaction's later passes keep and drop tokens
            for pos in (kept, dropped):
                assert (pos < cut).sum() >= 10 and (pos >= cut).sum() >= (3 if cut == 128 else 10), (name, cut)   # 128, 129: 24 tokens
        assert 0.2 < len(dropped) / (len(kept) + len(dropped)) < 0.45 and c.lengths.max() == L
    else:
        assert c.walks.shape[1] <= 64
    if name == "window_1":
        assert c.window == 1
    if name == "window_wider_than_sentence":
        assert c.window > 2 * c.walks.shape[1]
    if name == "negative_63":
        assert c.negative == 63 and len(f) <= 2e5
    if name == "f_skip":
        assert (f >= 6).sum() >= 100
    if name == "keep_boundary":
        tok = c.walks.reshape(-1)
        assert (tok == c.v).sum() == 1 and tok[c.tv] == c.v and (tok == c.u).sum() == 1 and tok[c.tu] == c.u
        assert c.sample_int[c.v] == K.keep_draw(c.seed, 0, c.tv) and c.sample_int[c.u] == K.keep_draw(c.seed, 0, c.tu) - 1
        L = c.walks.shape[1]
        assert len(dropped) == 1 and dropped[0] == c.tu % L    # u's token is the only one dropped: v's, on the boundary, is kept
        assert st["kept_len"][0, c.tv // L] == c.lengths[c.tv // L] and st["kept_len"][0, c.tu // L] == c.lengths[c.tu // L] - 1
        assert not np.array_equal(bits(s0[c.v]), bits(c.syn0[c.v].astype(np.float64)))
        assert np.array_equal(bits(s0[c.u]), bits(c.syn0[c.u].astype(np.float64)))
    if name == "table_ties":
        assert np.array_equal(c.cum_table, np.arange(1, c.n + 1))
    if name.startswith("epochs_3") or name == "min_alpha_clamp":
        assert c.epochs == 3 and set(ep for ep, _ in st["kept_len"]) == {c.first_epoch}
    if name == "min_alpha_clamp":
        assert np.float32(c.min_alpha) > np.float32(c.alpha) and c.first_epoch == 1
    if name == "degenerate_sentences":
        assert set(c.lengths.tolist()) == {1, 2}
        assert (kept_len == 0).sum() >= 10 and (kept_len == 1).sum() >= 10 and (kept_len == 2).sum() >= 10
    if name == "partition":
        assert len(c.walks) == K.PARTITION_S and len(np.unique(c.walks)) == c.walks.size == c.n and not c.syn0.any()
        assert (kept_len == 2).all() and st["pairs"] == c.n
        assert np.array_equal(bits(s1), bits(c.syn1.astype(np.float64)))         # no syn1neg row changes: every l1 read is zero
        assert (np.abs(s0).max(axis=1) > 0).all()                                # and every syn0 row got its one update


def test_epochs_3_chain_is_the_three_epoch_run():
    """the cases epochs_3_e0 .. e2 run one epoch each from the state before: together they are the mirror's plain three-epoch run"""
    c = K.sgns_case("epochs_3_e0")
    want = M.sgns(c.walks, c.lengths, c.n, c.d, window=c.window, epochs=3, negative=c.negative, seed=c.seed, syn0=c.syn0, syn1=c.syn1,
                  cum_table=c.cum_table, sample_int=c.sample_int)
    got = K.sgns_mirror("epochs_3_e2", np.float32)
    assert np.array_equal(bits(want[0]), bits(got[0])) and np.array_equal(bits(want[1]), bits(got[1]))
    for e in (1, 2):
        before = K.sgns_mirror("epochs_3_e%d" % (e - 1), np.float32)
        assert np.array_equal(bits(K.sgns_case("epochs_3_e%d" % e).syn0), bits(before[0]))


@pytest.mark.parametrize("ablate", M.ABLATIONS)
def test_each_wrong_rule_is_far_outside_the_gpu_bound(ablate):
    name = K.ABLATION_CASE[ablate]
    r0, r1, _ = K.sgns_mirror(name, np.float64)
    w0, w1, _ = K.sgns_mirror(name, np.float64, ablate)
    effect = max(np.abs(w0 - r0).max(), np.abs(w1 - r1).max())
    unit = K.d32(name)
    print(f"{ablate} on {name}: max |wrong - right| {effect:.3g} = {effect / unit:.3g} x d32 ({unit:.3g})")
    assert effect >= SENSITIVITY * MARGIN * unit


def test_ablation_table_names_every_wrong_rule_and_a_case():
    assert set(K.ABLATION_CASE) == set(M.ABLATIONS) and set(K.ABLATION_CASE.values()) <= set(K.SGNS_CASES)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_partition_result_does_not_depend_on_the_order_of_sentences(dtype):
    a0, a1, _ = K.sgns_mirror("partition", dtype)
    b0, b1, _ = K.sgns_mirror("partition", dtype, None, True)
    assert np.array_equal(bits(a0), bits(b0)) and np.array_equal(bits(a1), bits(b1))


def test_counts_case_has_its_shape():
    w, ln, n = K.counts_case()
    valid = np.arange(w.shape[1])[None, :] < ln[:, None]
    counts = np.bincount(w[valid], minlength=n)
    assert w.size % 256 != 0 and w.size > 256 and (w[~valid] == -1).any() and (w[~valid] >= 0).any()
    assert ((w[valid] >= 0) & (w[valid] < n)).all() and (counts == 0).sum() == 1
    assert (w[~valid][w[~valid] >= 0] == int(np.flatnonzero(counts == 0)[0])).all()   # the garbage would show as a count of the absent node
