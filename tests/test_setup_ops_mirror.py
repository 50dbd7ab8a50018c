"""CPU: what tests/test_gpu_setup_ops.py rests on, shown without a GPU.
  * the mirrors are right: percentile against np.percentile, the kNN contract against np.argpartition on tie-free data, the
    normalisation against oracle/gss_oracle.preprocess_graph;
  * the inputs have the properties they were made for: similarities exact in fp32, every percentile at its intended position, levels of
    both signs, tie groups, ties across the k-th place, forced row lengths, an asymmetric matrix;
  * the inputs can tell a wrong rule from the right one: the device's route through tiles, radix passes and the min pass
    (setup_ops_mirror.select) gives the mirror's bits, and with the off-diagonal weight fixed at 1 or at 2, the tile mask dropped,
    `rank + 1 >= eq_count` turned into `>`, the min pass skipped or its floor taken as `>=`, it gives other bits on these very inputs."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import setup_ops_cases as K  # noqa: E402
import setup_ops_mirror as M  # noqa: E402
from oracle import gss_oracle as O  # noqa: E402

RTOL_FP64 = 1e-13            # row sums and D^-1/2 (test_normalize_adj_matches_reference_fixture)
RTOL_AHAT = 1.2e-7           # A_hat in fp32 against the reference's cast


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- percentile -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.EXACT_CASES)
def test_exact_cases_are_exact_and_every_percentile_sits_where_it_was_meant_to(name):
    e, s = K.pct_case(name), K.pct_sim(name)
    n = e.shape[0]
    assert M.exact_in_fp32(s) and not np.signbit(s[s == 0]).any()
    if name.startswith("lat_"):
        assert set(np.unique(e)) <= {-1.0, -0.5, 0.0, 0.5, 1.0} and np.array_equal(s * 4, np.round(s * 4)) and np.abs(s).max() <= e.shape[1]
    val, cum = M.levels(s)
    plan = K.pct_plan(name)
    assert [p[2] for p in plan[-3:]] == ["q0", "q100", "largest_group"]
    for q, lo, what in plan:
        assert 0.0 <= q <= 100.0
        got_lo, hi, frac = M.position(n, q)
        assert got_lo == lo, (what, q, got_lo, lo)
        kind, _, b = what.partition("@")
        if not b:
            continue
        b = int(b)
        a_val, b_val, v = val[b], val[b + 1], K.pct_sorted(name)
        if kind == "in_B":
            assert v[lo] == b_val
            continue
        assert v[lo] == a_val and v[hi] == b_val and hi == lo + 1                    # the straddle: the min pass decides hi
        want = {"last_of_A": 0.0, "midpoint": 0.5, "inside_straddle": 0.75}[kind]
        assert abs(frac - want) < 1e-6 and (kind == "last_of_A" or frac > 0.0), (what, frac)


def test_lattice_cases_have_levels_of_both_signs_tie_groups_and_a_sign_boundary():
    for name in K.LATTICE_CASES:
        n = K.pct_case(name).shape[0]
        val, cum = M.levels(K.pct_sim(name))
        if n < 63:
            continue
        cnt = np.diff(np.concatenate([[0], cum]))
        assert len(val) >= 60 and (val < 0).sum() >= 20 and (val > 0).sum() >= 20, (name, len(val))
        assert cnt.max() >= 40, (name, cnt.max())                                    # tie groups far beyond the symmetric pair (d = 1024: 42)
        b = K.pct_boundaries(name)
        assert len(b) >= 5 and val[b[0]] < 0 <= val[b[0] + 1], name
    assert max(np.diff(np.concatenate([[0], M.levels(K.pct_sim(nm))[1]])).max() for nm in K.LATTICE_CASES) >= 1500


def test_special_row_all_equal_and_adjacent_cases_have_their_shapes():
    s = K.pct_sim("special_65")
    val, cum = M.levels(s)
    cnt = np.diff(np.concatenate([[0], cum]))
    assert sorted(cnt.tolist()) == [1, 128, 4096]                                    # v.v, the off-diagonal tile twice, u.u
    assert len(np.unique([s[0, 0], s[0, 64], s[64, 64]])) == 3
    assert len(K.pct_boundaries("special_65")) == 2
    assert len(M.levels(K.pct_sim("all_equal"))[0]) == 1 and K.pct_case("all_equal").shape[0] == 65
    s = K.pct_sim("adjacent")
    keys = M.ordered_key(s.astype(np.float32)).ravel()
    assert len(np.unique(keys)) == 820
    assert len(np.unique(keys >> np.uint32(21))) == 1                                # one first digit
    assert len(np.unique(keys >> np.uint32(10))) == 88                               # 88 second-digit prefixes
    assert len(np.unique(keys & np.uint32(0x3FF))) == 365                            # 365 third digits
    trace, crossed = {}, 0
    for q, lo, what in K.pct_plan("adjacent"):
        M.select(K.pct_case("adjacent"), q, trace=trace)
        crossed += trace["ran_min"] and (trace["key_hi"] >> 10) != (trace["key_lo"] >> 10)
    assert crossed >= 3                                                              # min passes that cross a bin edge of pass 2


@pytest.mark.parametrize("name", K.EXACT_CASES)
def test_percentile_mirror_agrees_with_numpy_to_one_fp32_ulp(name):
    s, v = K.pct_sim(name), K.pct_sorted(name)
    n = s.shape[0]
    worst = 0.0
    for q, got in zip(K.pct_qs(name), K.pct_mirror(name)):
        ref = np.percentile(s.ravel(), q)
        lo, hi, _ = M.position(n, q)
        ulp = np.spacing(np.float32(max(abs(v[lo]), abs(v[hi]))))                    # of the larger of the two values interpolated
        worst = max(worst, abs(float(got) - ref))
        assert abs(float(got) - ref) <= ulp, (name, q, got, ref)
    print(f"{name}: mirror against np.percentile, worst {worst:.3e}")


@pytest.mark.parametrize("name", K.EXACT_CASES)
def test_device_route_gives_the_mirrors_bits(name):
    e = K.pct_case(name)
    got = np.array([M.select(e, q) for q in K.pct_qs(name)], np.float32)
    assert np.array_equal(f32bits(got), f32bits(K.pct_mirror(name)))


def _changed(name, mutate, kinds=None):
    """the percentiles of the case's plan at which the mutated route gives other bits (or finds no bin) -> list of `what`"""
    e, out = K.pct_case(name), []
    for (q, _lo, what), want in zip(K.pct_plan(name), K.pct_mirror(name)):
        if kinds and what.partition("@")[0] not in kinds:
            continue
        got = M.select(e, q, mutate)
        if got is None or f32bits(got) != f32bits(want):
            out.append(what)
    return out


def test_wrong_tile_weights_and_a_dropped_mask_change_the_answer():
    for name in ("lat_65_16", "lat_129_48", "lat_200_1024", "special_65"):          # off-diagonal tiles: both weights are in play
        few = 3 if name == "special_65" else 8
        assert len(_changed(name, "wgt1")) >= few and "q100" in _changed(name, "wgt1"), name   # N^2 is never reached: no bin for the rank
        assert len(_changed(name, "wgt2")) >= few, name
    for name in ("lat_63_16", "lat_64_64", "lat_3_16"):                              # one tile: weight 2 doubles every count
        assert len(_changed(name, "wgt2")) >= 2, name
        assert not _changed(name, "wgt1"), name
    for name in ("lat_63_16", "lat_65_48", "lat_129_64", "lat_200_16", "lat_3_1024", "special_65"):   # n off the tile: clamped rows counted
        assert len(_changed(name, "no_mask")) >= 2, name
    assert not _changed("lat_64_16", "no_mask")
    side = _changed("special_65", "wgt1")                                             # the 128 entries counted as 64 move both boundaries
    assert any(w.endswith("@0") for w in side) and any(w.endswith("@1") for w in side)


@pytest.mark.parametrize("mutate", ["rank_gt", "no_min", "floor_ge"])
def test_a_lost_min_pass_changes_every_straddle_with_a_fraction(mutate):
    for name in K.EXACT_CASES:
        if not K.pct_boundaries(name):
            assert not _changed(name, mutate), name
            continue
        changed = _changed(name, mutate)
        inside = [w for _q, _lo, w in K.pct_plan(name) if w.partition("@")[0] in ("midpoint", "inside_straddle")]
        assert sorted(changed) == sorted(inside), (name, mutate)                      # frac 0 and both-in-B stay: they must not move


def test_a_key_without_the_sign_flip_orders_the_negative_levels_backwards():
    s32 = K.pct_sim("lat_65_16").astype(np.float32).ravel()
    order = np.argsort(s32, kind="stable")
    assert (np.diff(M.ordered_key(s32)[order].astype(np.int64)) >= 0).all()
    assert (np.diff(M.ordered_key_no_flip(s32)[order].astype(np.int64)) < 0).any()
    for v in (np.float32(-2.5), np.float32(0.0), np.float32(7.25), np.float32(-1e-40)):
        assert f32bits(M.key_to_float(M.ordered_key(v)[()])) == f32bits(v)


def test_non_finite_similarities_fall_into_eight_bins_of_the_first_histogram_and_nowhere_else():
    top = lambda v: int(M.ordered_key(np.array([v], np.float32))[0] >> np.uint32(21))  # noqa: E731
    fmax = np.finfo(np.float32).max
    assert top(np.inf) == 0x7FC and top(-np.inf) == 3 and top(fmax) == 0x7FB and top(-fmax) == 4
    nans = np.array([0x7F800001, 0x7FC00000, 0x7FFFFFFF, 0xFF800001, 0xFFC00000, 0xFFFFFFFF], np.uint32).view(np.float32)
    tops = [int(k >> np.uint32(21)) for k in M.ordered_key(nans)]
    assert all(t >= 0x7FC for t in tops[:3]) and all(t <= 3 for t in tops[3:])
    for name in K.EXACT_CASES:
        keys, wts = M.tile_keys(K.pct_sim(name).astype(np.float32))
        hist = M.pass0_histogram(keys, wts)
        assert hist.sum() == K.pct_case(name).shape[0] ** 2 and M.non_finite_count(hist) == 0
    for name in K.NON_FINITE_CASES:
        e, s = K.pct_case(name), K.pct_sim(name)
        assert e.shape == (65, 16) and not np.isfinite(s.astype(np.float32)).all()
        if name == "overflow":
            assert np.isfinite(e).all() and np.isinf(s.astype(np.float32)).sum() >= 3
        with np.errstate(invalid="ignore", over="ignore"):
            keys, wts = M.tile_keys(s.astype(np.float32))
        assert M.non_finite_count(M.pass0_histogram(keys, wts)) == int((~np.isfinite(s.astype(np.float32))).sum())
        with pytest.raises(M.NonFinite):
            M.percentile(e, 50.0, s)
        if name == "nan":
            assert np.isnan(np.percentile(s.ravel(), 50.0))


@pytest.mark.parametrize("name", K.UNIT_CASES)
def test_unit_row_cases_are_not_exact_and_the_rank_condition_holds_for_numpys_own_answer(name):
    s, v = K.pct_sim(name), K.pct_sorted(name)
    assert not M.exact_in_fp32(s)
    for q in K.UNIT_QS:
        rank_condition(v, s.shape[0], q, np.float32(np.percentile(v, q)))


def rank_condition(v, n, q, got, tol=2e-6):
    """v: the sorted fp64 similarities.  The number of them at or below the returned value may differ from lo + 1 by at most the number
    within tol of it, plus one when the answer is interpolated -> (the difference, the allowance)"""
    lo, _hi, frac = M.position(n, q)
    got = float(got)
    k = int(np.searchsorted(v, got + tol, side="right") - np.searchsorted(v, got - tol, side="left"))
    below = int(np.searchsorted(v, got, side="right"))
    allow = k + (1 if frac > 0 else 0)
    assert abs(below - (lo + 1)) <= allow, (q, below, lo + 1, allow)
    return abs(below - (lo + 1)), allow


# ---- kNN top-k ------------------------------------------------------------------------------------------------------------------------

def test_knn_cases_integer_similarities_are_exact_and_ties_cross_the_kth_place():
    for name in K.INT_CASES + ["equal_130"]:
        x, k = K.knn_case(name)
        assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 2 and 1 <= k <= min(len(x), 64)
        s = K.knn_sim(name)
        assert np.array_equal(s, np.round(s)) and np.array_equal(s, s.T)
    assert len(K.TIE_CASES) >= 5
    for name in K.TIE_CASES:
        x, k = K.knn_case(name)
        share = M.tie_across_kth(K.knn_sim(name), k).mean()
        print(f"{name}: {share:.2f} of the rows tie across place {k}")
        assert share >= 0.25, (name, share)
    assert M.tie_across_kth(K.knn_sim("int_65_8_64"), 64).sum() >= 5                 # one column left out: fewer rows tie, some do
    assert M.tie_across_kth(K.knn_sim("equal_130"), 5).all()
    for name in K.GAUSS_CASES:
        x, k = K.knn_case(name)
        assert not M.tie_across_kth(K.knn_sim(name), k).any()
    assert {K.knn_case(c)[0].shape[0] for c in K.WINDOW_CASES} == {130}


def test_knn_contract_accepts_argpartition_and_both_tie_rules_and_refuses_what_it_should():
    for name in K.GAUSS_CASES:                                                       # tie-free: the contract pins the set argpartition returns
        (x, k), s = K.knn_case(name), K.knn_sim(name)
        n = len(x)
        idx = np.argpartition(s, -k, 1)[:, -k:].astype(np.int32)
        M.check_topk(s, np.take_along_axis(s, idx, 1), idx, n)
        folded = [M.fold_topk(s[i], k) for i in range(n)]
        assert np.array_equal(np.sort(np.array([f[1] for f in folded]), 1), np.sort(idx, 1))
    differ = 0
    for name in ("int_130_8_5", "int_65_8_64", "equal_130", "int_64_8_5"):          # ties: `>` and `>=` keep other columns, both within the contract
        (x, k), s = K.knn_case(name), K.knn_sim(name)
        n = len(x)
        for strict in (True, False):
            f = [M.fold_topk(s[i], k, strict) for i in range(n)]
            M.check_topk(s, np.array([a for a, _ in f]), np.array([b for _, b in f]), n)
        a = np.array([M.fold_topk(s[i], k, True)[1] for i in range(n)])
        b = np.array([M.fold_topk(s[i], k, False)[1] for i in range(n)])
        differ += int((np.sort(a, 1) != np.sort(b, 1)).any(1).sum())
    assert differ >= 50
    (x, k), s = K.knn_case("int_130_24_5"), K.knn_sim("int_130_24_5")
    f = [M.fold_topk(s[i], k) for i in range(130)]
    val, idx = np.array([a for a, _ in f]), np.array([b for _, b in f])
    M.check_topk(s, val, idx, 130)
    M.check_topk(s[65:130], val[65:130], idx[65:130], 130)                           # a window's rows against their own similarities
    row = int(np.flatnonzero(~M.tie_across_kth(s, k))[0])
    worse = int(np.argmin(s[row]))
    for clause, spoil in (("repeat", lambda v, i: (v, np.r_[i[:-1], i[0]])),
                          ("out of", lambda v, i: (v, np.r_[i[:-1], 130])),
                          ("not the similarity", lambda v, i: (np.r_[v[:-1], v[-1] + 1.0], i)),
                          ("k largest", lambda v, i: (np.r_[s[row, worse], v[1:]], np.r_[worse, i[1:]]))):
        v2, i2 = val.copy(), idx.copy()
        v2[row], i2[row] = spoil(val[row], idx[row])
        with pytest.raises((AssertionError, IndexError), match=clause):
            M.check_topk(s, v2, i2, 130)
    with pytest.raises(AssertionError):                                              # a window read at the wrong rows (row_lo dropped)
        M.check_topk(s[65:130], val[0:65], idx[0:65], 130)


# ---- normalisation --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.NORM_CASES)
def test_normalisation_mirror_agrees_with_the_oracle_and_the_rows_have_their_lengths(name):
    c = K.norm_case(name)
    lengths = np.diff(c.rowptr)
    assert c.n == int(name[1:]) and (lengths >= 1).all() and (c.val > 0).all()
    a = K.csr_of(c)
    assert np.array_equal(a.diagonal(), np.ones(c.n)) and (K.norm_case(name).adj.diagonal() == 0).all()
    for r, want in K.FORCED.get(name, {}).items():
        assert lengths[r] == want, (name, r)
    for r in range(c.n):
        assert (np.diff(c.col[c.rowptr[r]:c.rowptr[r + 1]]) > 0).all()
    ref, ref_rowsum = O.preprocess_graph(c.adj)
    rowsum, dinv = M.rowsum_dinv(c.rowptr, c.val)
    np.testing.assert_allclose(rowsum, ref_rowsum, rtol=RTOL_FP64)
    assert np.array_equal(ref.indptr, c.rowptr) and np.array_equal(ref.indices, c.col)
    np.testing.assert_allclose(M.scale(c.rowptr, c.col, c.val, dinv, as_fp32=False), ref.data, rtol=RTOL_FP64)
    np.testing.assert_allclose(M.scale(c.rowptr, c.col, c.val, dinv), ref.data.astype(np.float32), rtol=RTOL_AHAT, atol=0)


def test_forced_row_lengths_cover_both_sides_of_the_64_lane_stride():
    seen = set()
    for name in K.NORM_CASES:
        seen |= set(np.diff(K.norm_case(name).rowptr).tolist())
    assert {1, 63, 64, 65, 129, 300} <= seen
    assert [K.norm_case(nm).n for nm in K.NORM_CASES[:5]] == [1, 3, 4, 5, 257]


def test_shards_of_the_asymmetric_matrix_and_a_swapped_scale_order():
    c, t = K.norm_case(K.ASYMMETRIC), K.transpose_case(K.ASYMMETRIC)
    a = K.csr_of(c)
    assert (a != a.T).nnz > 100 and abs(a - a.T).max() > 0.1
    _, dinv = M.rowsum_dinv(c.rowptr, c.val)
    whole = M.scale(c.rowptr, c.col, c.val, dinv)
    whole_t = sp.csr_matrix(sp.csr_matrix((whole, c.col, c.rowptr), shape=(c.n, c.n)).T)
    whole_t.sort_indices()
    assert np.array_equal(whole_t.indptr, t.rowptr) and np.array_equal(whole_t.indices, t.col)
    cuts = K.shard_cuts(c.n)
    assert {r0 for r0, _ in cuts} == {0, 1, c.n // 2, c.n - 1} and {1, 4, 5} <= {rows for _, rows in cuts}
    assert (0, c.n) in cuts and (c.n - 1, 1) in cuts
    swapped = 0
    for row0, rows in cuts:
        rp, col, val, e0 = K.cut(c, row0, rows)
        assert np.array_equal(f32bits(M.scale_shard(row0, rp, col, val, dinv, 0)), f32bits(whole[e0:e0 + len(val)]))
        rp, col, val, e0 = K.cut(t, row0, rows)
        got = M.scale_shard(row0, rp, col, val, dinv, 1)
        assert np.array_equal(f32bits(got), f32bits(whole_t.data[e0:e0 + len(val)]))
        assert np.array_equal(f32bits(M.scale_shard(row0, rp, col, val, dinv, 0)), f32bits(got))
    # The two factors of the transposed branch in the other order: 561 of the 2,027 fp64 products of this matrix differ in their last bit,
    # and none of them survives the cast to fp32 (a product would have to lie within 2^-53 of an fp32 rounding boundary).  So the ORDER of
    # the factors is not observable in the op's output; which dinv an entry reads is, and that is what the shard tests hold.
    rows = M.row_of_entry(t.rowptr)
    one, other = (t.val * dinv[rows]) * dinv[t.col], (t.val * dinv[t.col]) * dinv[rows]
    assert (one != other).sum() >= 100 and np.array_equal(f32bits(one.astype(np.float32)), f32bits(other.astype(np.float32)))
    half = rows >= c.n // 2                                                          # row0 dropped, on the shard [n // 2, n)
    wrong = (t.val[half] * dinv[rows[half] - c.n // 2]) * dinv[t.col[half]]
    assert (f32bits(wrong.astype(np.float32)) != f32bits(whole_t.data[half])).mean() > 0.9


def test_rowsum_check_cases():
    for name in K.CHECK_CASES:
        v = K.check_case(name)
        kind, n = name.split("_")
        count, first = M.rowsum_check(v)
        if kind == "good":
            assert (count, first) == (0, -1) and (int(n) < 63 or (np.isinf(v).any() and (v == 5e-324).any()))
        elif kind == "every":
            assert (count, first) == (int(n), 0)
        elif kind == "late":
            assert (count, first) == (3, 997)
        else:
            at = sorted({p for p in K.BAD_AT + (int(n) - 1,) if p < int(n)})
            assert (count, first) == (len(at), 0)
    v = K.check_case("planted_1000")
    assert v[0] == 0 and v[63] == 0 and np.signbit(v[63]) and v[64] < 0 and np.isnan(v[255])      # every kind of bad value, in four waves
