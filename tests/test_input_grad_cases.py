"""CPU: the cases, the port of launch_gemm's EPI_SPLIT decision and the two references of tests/input_grad_cases.py, which
tests/test_gpu_input_grad.py holds gss_dense_bwd_input to.  The class table is pinned: whoever changes launch_gemm (and its port) sees
here which case lost its class, and that all 14 instantiations are still launched by some GPU case.  The int regime's reference is held
to numpy's int64 matmul, a numpy float32 evaluation of the unit regime sits inside the derived bound, and the seeded mutations -- a K
chunk dropped, a column tile fed from the other weight half -- are rejected by both checks."""
import numpy as np
import pytest

import input_grad_cases as C

# (nt, mt) -> {d: the n of CASES} under the default gemm_variant 2.  Without a row list the class is the whole-line kernel of that
# (nt, mt) where nt >= 2 and the MFMA-layout ("plain") kernel where nt = 1; with a row list always the plain one.
TABLE = {
    (1, 1): {16: (1, 15, 16, 17, 63, 64, 65, 129), 48: (65, 129)},
    (1, 2): {272: (1, 15, 16, 17, 63, 64, 65, 129, 127, 128)},
    (2, 1): {32: (1, 15, 16, 17, 63, 64, 65, 129, 447, 511, 513, 1025), 96: (65, 129), 64: (8128,), 192: (2688,), 128: (129, 4032)},
    (2, 2): {288: (1, 15, 16, 17, 63, 64, 65, 129, 127, 128, 895, 1023, 1025, 2049), 320: (1600,), 256: (129, 1984), 384: (1344,),
             512: (960,), 1024: (448,)},
    (4, 1): {64: (8129, 8191, 8192), 192: (2689, 2751, 2752), 128: (4033, 4095, 4096, 8128)},
    (4, 2): {320: (1601, 1663, 1664, 1665), 256: (1985, 2047, 2048, 4032), 384: (1345, 1407, 1408, 2688),
             512: (961, 1023, 1024, 1984), 1024: (449, 511, 512, 960)},
    (8, 1): {128: (8129, 8191, 8192)},
    (8, 2): {256: (4033, 4095, 4096), 384: (2689, 2751, 2752), 512: (1985, 2047, 2048), 1024: (961, 1023, 1024)},
}


def test_the_class_table_is_pinned_and_covers_all_14_instantiations():
    got = {}
    for d, n in C.CASES:
        nt, mt, lines = C.tile_class(n, d, False)
        assert lines == (nt >= 2)
        assert C.tile_class(n, d, True) == (nt, mt, False)
        assert C.tile_class(n, d, False, 5) == (nt, mt, lines) and C.tile_class(n, d, True, 5) == (nt, mt, False)
        assert C.tile_class(n, d, False, 3) == (nt, 2, lines) and C.tile_class(n, d, True, 3) == (nt, 2, False)
        got.setdefault((nt, mt), {}).setdefault(d, []).append(n)
    assert {k: {d: tuple(ns) for d, ns in v.items()} for k, v in got.items()} == TABLE
    assert len(set(C.CASES)) == len(C.CASES)
    reached = C.reached()
    assert set(reached) == set(C.ALL_CLASSES) and len(C.ALL_CLASSES) == 14
    for cls in C.ALL_CLASSES:
        by_default = [x for x in reached[cls] if x[3] == 2]
        print(cls, len(reached[cls]), "launches,", len(by_default), "under the default gemm_variant; e.g.", (by_default or reached[cls])[0])
        assert by_default, f"no GPU case launches gemm_nt_lds_kernel<{cls[0]}, {cls[1]}, EPI_SPLIT, 4, {'true' if cls[2] else 'false'}> by default"
    # the row threshold of mt, held from both sides
    assert [C.tile_class(n, 32, False) for n in C.BIG_N] == [(2, 1, True), (2, 2, True)]


def test_thresholds_of_the_port_are_the_issue_s():
    """the smallest n of the larger nt per width, as replayed from launch_gemm: one row fewer gives the class below"""
    for d, nt, n in ((64, 4, 8129), (192, 4, 2689), (320, 4, 1601), (128, 4, 4033), (128, 8, 8129), (256, 4, 1985), (256, 8, 4033),
                     (384, 4, 1345), (384, 8, 2689), (512, 4, 961), (512, 8, 1985), (1024, 4, 449), (1024, 8, 961)):
        assert C.tile_class(n, d, False)[0] == nt and C.tile_class(n - 1, d, False)[0] == nt // 2, (d, nt, n)
        assert (d, n) in C.CASES and (d, n - 1) in C.CASES, (d, n)
        if nt >= 4 and d >= 64:
            assert (d, n + 62) in C.CASES and (d, n + 63) in C.CASES, (d, n)
    for d in (16, 48, 272):
        assert {C.tile_class(n, d, False)[0] for n in (1, 10 ** 6)} == {1}
    for d in (32, 96, 288):
        assert {C.tile_class(n, d, False)[0] for n in (1, 10 ** 6)} == {2}
    assert [C.tile_class(1, d, False)[1] for d in (240, 256, 272)] == [1, 2, 2]


def test_the_cases_stand_on_both_sides_of_a_tile_edge_and_show_every_branch_of_xcd_ids():
    for d in (32, 288):
        assert {C.node_tiles(n, d) for dd, n in C.CASES if dd == d} >= set(C.XCD_TILES), d
    by_class = {}
    for d, n in C.CASES:
        nt, mt, _ = C.tile_class(n, d, False)
        by_class.setdefault((nt, mt), []).append(n)
    for (nt, mt), ns in by_class.items():
        tile = 64 * mt
        rem = {n % tile for n in ns}
        assert 0 in rem and 1 in rem and tile - 1 in rem, (nt, mt, sorted(rem))      # a full last tile, one of one row, one a row short
        assert any(n % 2 for n in ns)                                                # an even / odd pair of the whole-line epilogue cut in two


def test_row_lists_are_unique_valid_and_hold_the_first_and_the_last_row():
    for d, n in C.CASES:
        if d not in (16, 128):
            continue
        rows = C.case("int", d, n)["rows"]
        assert rows.dtype == np.int32 and len(rows) == n == len(np.unique(rows)) and rows.min() >= 0 and rows.max() == 3 * n - 1
        assert n == 1 or (rows[0] == 0 and rows[-1] == 3 * n - 1)
        assert n < 64 or (np.diff(rows) < 0).any()                 # not sorted: a scatter


@pytest.mark.parametrize("d,n", [(16, 17), (48, 129), (272, 128), (32, 513), (128, 129)])
def test_int_reference_is_numpy_s_int64_product(d, n):
    c = C.case("int", d, n)
    assert np.abs(c["dp"]).max() <= 3 and np.abs(c["w1t"]).max() <= 3 and (c["dp"] == np.round(c["dp"])).all()
    gax, gam = C.exact(c["dp"], c["w1t"], c["w2t"])
    assert np.array_equal(gax, (c["dp"].astype(np.int64) @ c["w1t"].astype(np.int64).T).astype(np.float32))
    assert np.array_equal(gam, (c["dp"].astype(np.int64) @ c["w2t"].astype(np.int64).T).astype(np.float32))
    assert 9 * 1024 < 2 ** 24


def test_big_cases_are_one_small_product_indexed():
    for n in C.BIG_N:
        c = C.big_case(n)
        assert c["dp"].shape == (n, 32) and c["gax"].shape == (n, 32)
        for r in (0, C.TILED_ROWS - 1, C.TILED_ROWS, n - 1):
            assert np.array_equal(c["gax"][r], (c["dp"][r].astype(np.int64) @ c["w1t"].astype(np.int64).T).astype(np.float32))
            assert np.array_equal(c["gam"][r], (c["dp"][r].astype(np.int64) @ c["w2t"].astype(np.int64).T).astype(np.float32))
        assert len(np.unique(c["dp"][:C.TILED_ROWS], axis=0)) > C.TILED_ROWS - 8


@pytest.mark.parametrize("d,n", C.CASES)
def test_float32_evaluation_sits_inside_the_derived_bound(d, n):
    """numpy's float32 matmul (blocked, FMA or not) of the unit regime, against the fp64 reference"""
    c = C.case("unit", d, n)
    (gax, gam), (lim_ax, lim_am) = C.reference(c["dp"], c["w1t"], c["w2t"])
    worst = 0.0
    for ref, lim, wt in ((gax, lim_ax, c["w1t"]), (gam, lim_am, c["w2t"])):
        got = c["dp"] @ wt.T
        assert got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= lim).all(), (d, n, float((err / lim).max()))
        worst = max(worst, float((err / lim).max()))
    print(f"d={d} n={n}: float32 error / bound {worst:.3f}")
    if n >= 17:
        s = C.scales(n)
        assert (s == np.float32(2.0 ** -20)).any() and (s == np.float32(2.0 ** 10)).any()
        assert np.array_equal(c["dp"][3] * np.float32(2.0 ** 20) * np.float32(2.0 ** -20), c["dp"][3])        # the scaling is exact


@pytest.mark.parametrize("d,n", [(16, 17), (32, 65), (128, 129), (192, 64), (272, 17)])
def test_the_seeded_mutations_are_rejected(d, n):
    nt = C.tile_class(n, d, False)[0]
    tiles = d // (16 * nt)
    for regime in ("int", "unit"):
        c = C.case(regime, d, n)
        if regime == "int":
            ref = C.exact(c["dp"], c["w1t"], c["w2t"])

            def ok(got):
                return all(np.array_equal(g.astype(np.float32), r) for g, r in zip(got, ref))
        else:
            ref, lim = C.reference(c["dp"], c["w1t"], c["w2t"])

            def ok(got):
                return all((np.abs(g - r) <= b).all() for g, r, b in zip(got, ref, lim))

        def product(dp, w1t, w2t):
            return dp.astype(np.float64) @ w1t.astype(np.float64).T, dp.astype(np.float64) @ w2t.astype(np.float64).T

        assert ok(product(c["dp"], c["w1t"], c["w2t"]))
        for chunk in (0, d // 16 - 1):
            assert not ok(product(C.drop_k_chunk(c["dp"], chunk), c["w1t"], c["w2t"])), (regime, "dropped chunk", chunk)
            doubled = c["dp"].copy()
            doubled[:, 16 * chunk:16 * (chunk + 1)] *= 2
            assert not ok(product(doubled, c["w1t"], c["w2t"])), (regime, "doubled chunk", chunk)
        for tile in (0, tiles - 1):
            assert not ok(product(c["dp"], *C.swap_halves(c["w1t"], c["w2t"], nt, tile))), (regime, "swapped half", tile)
        # a row read from the clamp row (staging clamps to n - 1), a row of a scaled-down band included
        for r in ((0, 3) if n > 4 else (0,)):
            if n > 1:
                clamped = c["dp"].copy()
                clamped[r] = c["dp"][n - 1]
                assert not ok(product(clamped, c["w1t"], c["w2t"])), (regime, "clamp row", r)
