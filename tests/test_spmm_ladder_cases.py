"""CPU: what tests/spmm_ladder_cases.py claims about its own inputs, asserted from its restatement of the placement rule of
csrc/segments.h -- so that a red exact comparison in tests/test_gpu_spmm_ladder.py is the kernel's, not a wrong claim of the cases.
(The descriptors the C++ really builds are checked by tests/native/segments_check.cpp.)

Two properties cannot exist at every width, by the rule itself, and are asserted to be impossible there instead of present:
  * an empty segment inside a block of a whole-CSR schedule needs (p - 1) ceil(len / p) >= len with len > 16 p, i.e. p >= 32: with one
    lane group per wave (d >= 256 unsliced) the largest block has 16 groups.  Checked for every length up to a full row;
  * a wave that mixes block sizes needs two aligned blocks smaller than the wave, of different sizes: four groups per wave at least."""
import numpy as np
import pytest
import scipy.sparse as sp

import sparse_hop_mirror as M
import spmm_ladder_cases as L

GPW_LOG2 = (0, 1, 2, 3, 4)


def test_the_graphs_are_what_the_docstring_says():
    g = L.graph("ladder")
    assert g.n_cols == L.N_COLS == 8320 and g.n_rows == 2 * len(L.LADDER_LENGTHS) + len(L.EXTRA_LENGTHS) + L.N_FILLER + 5 < g.n_cols
    for k in L.LADDER_LENGTHS:
        assert len(L.rows_of_length(g, k)) >= 2, k
        if k > 9:
            assert len(L.rows_of_length(g, k)) == 2 and g.keep[L.rows_of_length(g, k)].tolist() == [True, False], k
    for k in L.EXTRA_LENGTHS:
        assert len(L.rows_of_length(g, k)) == 1
    assert g.lens[0] == 0 and g.lens[-1] == 0 and all(g.lens[r] == 0 for r in g.empty_run) and np.diff(g.empty_run).tolist() == [1, 1]
    assert 100_000 < g.a.nnz < 130_000
    long_rows = np.flatnonzero(g.lens > 9)
    assert (np.diff(np.sort(long_rows)) > 1).any() and not np.array_equal(g.lens[long_rows], np.sort(g.lens[long_rows]))   # permuted
    for kind in L.KINDS:
        a = L.graph(kind).a
        assert a.has_sorted_indices and a.dtype == np.float32 and a.indices.dtype == np.int32
        for r in range(a.shape[0]):
            cols = a.indices[a.indptr[r]:a.indptr[r + 1]]
            assert (np.diff(cols) > 0).all()                      # sorted and distinct
        assert set(np.unique(a.data).tolist()) == {1.0, 2.0, 3.0}
    p = L.graph("packed")
    assert (p.lens == 32).all() and p.n_rows % 256 == 0


@pytest.mark.parametrize("gl", GPW_LOG2)
def test_the_ladder_reaches_every_block_class(gl):
    g = L.graph("ladder")
    s = L.schedule(g.lens, gl)
    assert sorted(set(s.plog.tolist())) == list(range(s.ngb_log2 + 1))
    assert s.whole.any() and (s.plog[s.whole] == s.ngb_log2).all() and (s.per[s.whole] > L.SEG_EDGES).all()
    assert (s.per[~s.whole] <= L.SEG_EDGES).all()
    assert ((s.plog == s.ngb_log2) & ~s.whole).any()              # the largest block with ordinary segments too
    holed = (s.n_empty > 0) & (s.p > 1)
    if gl >= 1:
        assert holed.any() and 513 in s.lens[holed]
        assert set(s.lens[holed].tolist()) >= {4: {513, 1025, 2049, 4097}, 3: {513, 1025, 2049, 4097, 8193}, 2: {513, 1025, 2049}, 1: {513}}[gl]
    else:
        every = L.schedule(np.arange(0, L.N_COLS + 1), 0)
        assert not ((every.n_empty > 0) & (every.p > 1)).any()    # impossible at one group per wave (module docstring)
        assert not holed.any()
    if gl >= 2:
        assert L.mixed_waves(s)
    else:
        assert not L.mixed_waves(s) and s.gpw < 4
    assert L.mixed_workgroups(s)
    assert all(s.multi[w] for w in L.mixed_workgroups(s))
    assert s.padding > 0
    assert L.schedule(L.graph("packed").lens, gl).padding == 0
    assert (L.schedule(L.graph("packed").lens, gl).plog == 0).all()
    # the sparse batch: a member row of every class, an empty member, a member column in the first and the last segment of such rows
    ids = L.batch("ladder")
    assert 35 <= len(ids) <= 60 and len(set(ids.tolist())) == len(ids)
    members = ids[ids < g.n_rows]
    assert set(s.plog[members].tolist()) == set(range(s.ngb_log2 + 1)) and s.whole[members].any() and (g.lens[members] == 0).any()
    hit_classes = set()
    for k in L.CLASS_LENGTHS:
        r0, r1 = L.rows_of_length(g, k)[:2]
        cols0 = g.a.indices[g.a.indptr[r0]:g.a.indptr[r0 + 1]]
        assert cols0[0] in ids and cols0[-1] in ids and np.isin(g.a.indices[g.a.indptr[r1]:g.a.indptr[r1 + 1]], ids).any()
        hit_classes.add(int(s.plog[r0]))
    assert hit_classes == set(range(s.ngb_log2 + 1))
    # the row filter keeps one row of every class and drops the other copy of the same length
    assert set(s.plog[g.keep].tolist()) == set(s.plog[~g.keep].tolist()) == set(range(s.ngb_log2 + 1))
    assert s.whole[g.keep].any() and s.whole[~g.keep].any()


@pytest.mark.parametrize("gl", GPW_LOG2)
def test_the_column_halves_cover_the_in_wave_and_two_wave_classes_again(gl):
    """splitting by column changes every row's class in both halves: both must still reach plog 1 .. 4"""
    for which in ("first", "second"):
        h = L.part("ladder", which)
        s = L.schedule(np.diff(h.indptr), gl)
        assert set(s.plog.tolist()) >= {1, 2, 3, 4}, which
    first, second = L.halves("ladder")
    assert abs(first - sp.csr_matrix(L.graph("ladder").a) + second).nnz == 0
    assert first.indices.max() < L.N_COLS // 3 <= second.indices.min()


@pytest.mark.parametrize("gl", GPW_LOG2)
def test_under_spmm_giant_64_the_three_passes_cover_the_classes(gl):
    g = L.graph("ladder")
    gi = L.giant_items(g.lens, L.GIANT)
    per_row = dict(zip(g.lens[gi.rows].tolist(), gi.finish.tolist()))
    assert 64 not in per_row and (per_row[65], per_row[80], per_row[81]) == (5, 5, 6)       # both sides of the threshold and of a chunk edge
    assert gi.short.max() == 64 and gi.chunks.max() == 16 and set(gi.chunks.tolist()) >= {1, 15, 16}
    assert len(gi.rows) > 40                                       # almost every ladder row is giant
    fin = L.schedule(gi.finish, gl)
    assert len(set(fin.plog.tolist())) >= 5 and fin.plog.max() == min(fin.ngb_log2, 5) and L.mixed_workgroups(fin)
    assert set(L.schedule(gi.short, gl).plog.tolist()) == {0, 1}
    assert gi.finish.max() == 520 and gi.finish.min() == 5


def test_widths_map_to_the_five_lane_group_classes():
    assert [L.gpw_log2_of(d) for d in L.WIDTHS] == [4, 3, 2, 2, 1, 0, 0, 0]
    assert [L.gpw_log2_of(d, s) for d, s in ((128, 2), (128, 4), (128, 8), (512, 2), (512, 4), (512, 8), (1024, 2), (1024, 4), (1024, 8))] == \
        [2, 3, 4, 0, 1, 2, 0, 0, 1]


@pytest.mark.parametrize("d", L.WIDTHS)
def test_the_exactness_premise(d):
    """every reference is an integer (dp: a multiple of 0.5) far below 2^24 -- and so is every partial sum a kernel can form, by the
    worst case over the operands' ranges; the references come from scipy over int64, not from project code"""
    for kind in L.KINDS:
        g = L.graph(kind)
        for name in L._GATHERED + L._BY_ROW:
            x = L.operand(kind, d, name)
            assert x.dtype == np.float32 and np.array_equal(x, np.rint(x)) and np.abs(x).max() <= 4
        p = L.operand(kind, d, "p")
        planted = np.zeros(g.n_rows, bool)
        planted[list(L.plant_rows(g))] = True
        assert (p[~planted] >= 1).all() and np.array_equal(p[~planted], np.rint(p[~planted]))
        assert all(np.array_equal(p[r, :4].view(np.int32), L.P_PLANT.view(np.int32)) for r in L.plant_rows(g))
        assert g.lens.max() * 3 * 4 * 4 + 8 < 2 ** 24
        worst = 0
        for name, ref in L.all_references(kind, d).items():
            if name.endswith(" dp"):
                exact = ref[~planted]
                assert np.array_equal(2 * exact, np.rint(2 * exact)), name
                worst = max(worst, np.abs(ref).max() * 2)
            else:
                assert ref.dtype == np.int64, name
                worst = max(worst, np.abs(ref).max())
        assert worst < 2 ** 24
        # the sparse references: a zero-sum live row and a member with a zero gradient are among the cases
        cs, r1 = L.bwd1s_case(kind, d), L.bwd1s_ref(kind, d)
        assert (cs.live & ~r1.nz).any() and r1.nz[cs.pos_row >= 0].all() and not r1.nz.all()
        assert (cs.g_am_b == 0).all(1).any()


def test_the_planted_elements_bound_is_the_mirrors():
    """dp on the four planted elements of the planted rows is the one non-exact check: the mirror's own (k + 4) 2^-24 S over this file's
    S (the mode's expression over absolute values).  Where p = -20 the sum is scaled by e^-20 and the bound is below 2^-9 even on the
    row of 4097 entries; gx of the same rows, and every other element of dp, stay exact"""
    for kind in L.KINDS:
        g = L.graph(kind)
        rows = list(L.plant_rows(g))
        for ref in (L.bwd2_ref(kind, 48, True, False), L.bwd2_ref(kind, 48, True, True), L.bwd2_ref(kind, 48, False, False),
                    L.bwd2s_ref(kind, 48, False), L.bwd2s_ref(kind, 48, True)):
            lim = M.bound(ref.k, ref.s_dp)
            assert np.isfinite(lim).all() and (lim >= 0).all() and lim[rows, 3].max() < 2.0 ** -9
            assert (np.abs(ref.dp) <= ref.s_dp + 1e-9).all()
        if kind == "ladder":
            assert sorted(g.lens[rows].tolist()) == sorted(L.PLANT_LENGTHS)
