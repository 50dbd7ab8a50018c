"""CPU: tests/sparse_hop_mirror.py -- the fp64 contract the row-sparse SpMM modes are held to in test_gpu_sparse_ops.py -- is itself
checked here: (1) against scipy products of the scattered dense operands, which it must equal to fp64 rounding; (2) an fp32 evaluation of
the same loops stays inside the derived bound (k + 4) 2^-24 S at every case and seed the GPU tests use, so the bound's term count fits
the epilogues as they are; (3) the inputs really hold the situations the GPU tests are about (zero-sum rows with member neighbours,
zero pieces in live rows, members on word edges); (4) the bitmap helpers."""
import numpy as np
import pytest

import sparse_hop_cases as K
import sparse_hop_mirror as M

FP64 = 1e-13    # |mirror - scipy| <= FP64 * S: both are fp64 sums of the same terms in different orders (k <= 2100 terms, u = 1.1e-16)


def scatter(rows_compact, ids, n):
    out = np.zeros((n, rows_compact.shape[1]), np.float64)
    keep = ids < n
    out[ids[keep]] = rows_compact[keep]
    return out


def close64(got, ref, s):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - ref) <= FP64 * s + 1e-300))


@pytest.mark.parametrize("kind,d,b", K.BWD1_CASES)
def test_bwd1_sparse_mirror_equals_scipy_and_fp32_stays_inside_the_bound(kind, d, b):
    cs = K.bwd1_case(kind, d, b)
    g = cs.g
    A = g.a.astype(np.float64)
    ref = M.bwd1_sparse(g.a, cs.g_am_b, cs.g_ax_b, cs.pos, cs.pos_row, cs.x_in, cs.ax)
    dm = A @ scatter(cs.g_am_b, cs.ids, g.n_cols)
    u = dm * cs.x_in + scatter(cs.g_ax_b, cs.ids, g.n_rows)
    assert close64(ref.u, u, ref.s_u) and close64(ref.t, dm * cs.ax, ref.s_t)
    member = cs.pos_row >= 0
    assert np.array_equal(ref.nz, member | (dm != 0).any(1)) and ref.written.all()
    assert np.array_equal(ref.k, np.asarray((A != 0).astype(np.int64) @ (cs.pos >= 0).astype(np.int64)).reshape(-1))
    # the filters are pure: a consistent posbits and a live-row set that covers the members and their neighbours change nothing
    live = K.live_rows_of(cs, extra=(1, g.n_rows - 2))
    filt = M.bwd1_sparse(g.a, cs.g_am_b, cs.g_ax_b, cs.pos, cs.pos_row, cs.x_in, cs.ax, posbits=M.pack_bits(cs.ids, g.n_cols),
                         live_rows=M.pack_bits(np.flatnonzero(live), g.n_rows), skip_zero_rows=True)
    assert np.array_equal(filt.u, ref.u) and np.array_equal(filt.t, ref.t) and np.array_equal(filt.nz, ref.nz)
    assert np.array_equal(filt.written, ref.nz) and not (ref.nz & ~live).any()
    # the situations the GPU test is about are in the inputs
    if b > 1:
        assert ref.k[cs.zrow] >= 1 and not ref.nz[cs.zrow] and not member[cs.zrow]              # member neighbours, zero sum, not a member
        live_rows = ref.nz & (ref.k > 0) & (ref.s_t != 0).any(1)
        assert live_rows.sum() >= 10 and not ref.s_t[live_rows][:, 4:8].any()                   # live rows whose piece 1 is zero
        assert (member & (ref.k > 0) & ~(ref.s_t != 0).any(1)).any() or b < 300                 # a member row with member neighbours and a zero sum
        for i in K.EDGE_IDS + (g.n_cols - 1, g.n_rows - 1, g.hubs[0], g.empty[0]):
            assert cs.pos[i] >= 0
    # an fp32 evaluation of the same loops against the bound
    f32 = M.bwd1_sparse(g.a, cs.g_am_b, cs.g_ax_b, cs.pos, cs.pos_row, cs.x_in, cs.ax, dtype=np.float32)
    assert f32.u.dtype == np.float32
    assert np.all(np.abs(f32.u.astype(np.float64) - ref.u) <= M.bound(ref.k, ref.s_u))
    assert np.all(np.abs(f32.t.astype(np.float64) - ref.t) <= M.bound(ref.k, ref.s_t))
    # ... and the bound is sharp enough to see one entry: dropping a row's last contributing entry moves it by far more
    r = int(np.flatnonzero((ref.k == 1) & (ref.s_t != 0).any(1))[0]) if ((ref.k == 1) & (ref.s_t != 0).any(1)).any() else -1
    if r >= 0:
        assert np.any(np.abs(0.0 - ref.t[r]) > 1e3 * M.bound(ref.k, ref.s_t)[r])


@pytest.mark.parametrize("kind,d,b,limit", [c + (0,) for c in K.BWD2_CASES] + K.LIMIT_CASES)
def test_bwd2_sparse_res_mirror_equals_scipy_and_fp32_stays_inside_the_bound(kind, d, b, limit):
    cs = K.bwd2_case(kind, d, b, limit)
    g = cs.g
    A = g.a.astype(np.float64)
    own = limit or g.n_rows
    ref = M.bwd2_sparse_res(g.a, cs.u, cs.t, cs.p, cs.c, cs.res_b, cs.pos_row, pos_row_limit=limit)
    gx = A @ cs.u.astype(np.float64)
    gx[:own] += cs.t
    eg = np.where(cs.p > 0, 1.0, np.exp(np.minimum(cs.p, 0).astype(np.float64)))
    dp = cs.c * gx * eg
    dp[:own] += scatter(cs.res_b, cs.ids, g.n_rows)[:own]
    assert close64(ref.gx, gx, ref.s_gx) and close64(ref.dp, dp, ref.s_dp)
    assert np.array_equal(ref.k, g.lens)
    # nzbits = exactly the non-zero rows of u (t is zero elsewhere): a pure filter
    assert not cs.t[~cs.inside[:own]].any() and np.array_equal(cs.inside, (cs.u != 0).any(1))
    filt = M.bwd2_sparse_res(g.a, cs.u, cs.t, cs.p, cs.c, cs.res_b, cs.pos_row, nzbits=M.pack_bits(np.flatnonzero(cs.inside), g.n_cols),
                             pos_row_limit=limit)
    assert np.array_equal(filt.dp, ref.dp) and np.array_equal(filt.gx, ref.gx) and (filt.k <= ref.k).all()
    for fr in (ref, filt):
        f32 = M.bwd2_sparse_res(g.a, cs.u, cs.t, cs.p, cs.c, cs.res_b, cs.pos_row, pos_row_limit=limit, dtype=np.float32,
                                nzbits=None if fr is ref else M.pack_bits(np.flatnonzero(cs.inside), g.n_cols))
        assert np.all(np.abs(f32.gx.astype(np.float64) - fr.gx) <= M.bound(fr.k, fr.s_gx))
        assert np.all(np.abs(f32.dp.astype(np.float64) - fr.dp) <= M.bound(fr.k, fr.s_dp))
    # two passes: the entries split by column, the first half's sums handed over as y_in
    c0 = g.n_cols // 3
    first, second = K.split_by_column(g.a, c0)
    y1 = M.spmm_filtered(first, cs.u).y
    two = M.bwd2_sparse_res(second, cs.u, cs.t, cs.p, cs.c, cs.res_b, cs.pos_row, y_in=y1, pos_row_limit=limit)
    assert close64(two.dp, dp, ref.s_dp) and close64(two.gx, gx, ref.s_gx)


@pytest.mark.parametrize("kind,d,b", K.FWD_CASES)
def test_filtered_forward_mirror_equals_scipy_and_fp32_stays_inside_the_bound(kind, d, b):
    cs = K.fwd_case(kind, d, b)
    g = cs.g
    A = g.a.astype(np.float64)
    live = np.zeros(g.n_rows, bool)
    live[cs.rows] = True
    bits = M.mark_rows_and_neighbours(g.a, cs.rows, np.zeros(M.words_for(g.n_cols), np.uint32))
    marked = M.unpack_bits(bits, g.n_cols)
    want = np.zeros(g.n_cols, bool)
    want[cs.rows] = True
    want[np.flatnonzero(np.asarray(A[cs.rows].astype(bool).sum(0)).reshape(-1))] = True
    assert np.array_equal(marked, want)
    y_ref = A @ cs.x.astype(np.float64)
    for kw, written, x in ((dict(row_pos=cs.row_pos), live, cs.x), (dict(row_bits=bits), marked[:g.n_rows], cs.x),
                           (dict(row_pos=cs.row_pos, row_bits=bits), live, cs.x),
                           (dict(gather_bits=M.pack_bits(np.flatnonzero(cs.inside), g.n_cols)), np.ones(g.n_rows, bool), cs.xz)):
        ref = M.spmm_filtered(g.a, x, h=None if "row_pos" in kw or "gather_bits" in kw else cs.h, **kw)
        assert np.array_equal(ref.written, written)
        yy = A @ x.astype(np.float64)
        assert close64(ref.y[written], yy[written], ref.s_y[written]) and not ref.y[~written].any()
        if ref.m is not None:
            assert close64(ref.m[written], (yy * cs.h)[written], ref.s_m[written])
        f32 = M.spmm_filtered(g.a, x, h=None if ref.m is None else cs.h, dtype=np.float32, **kw)
        assert np.all(np.abs(f32.y.astype(np.float64) - ref.y) <= M.bound(ref.k, ref.s_y))
        if ref.m is not None:
            assert np.all(np.abs(f32.m.astype(np.float64) - ref.m) <= M.bound(ref.k, ref.s_m))
    # gather_bits over an operand that is zero outside the set: the unfiltered product of the same operand
    assert close64(M.spmm_filtered(g.a, cs.xz, gather_bits=M.pack_bits(np.flatnonzero(cs.inside), g.n_cols)).y,
                   A @ cs.xz.astype(np.float64), M.spmm_filtered(g.a, cs.xz).s_y)
    assert y_ref.shape == (g.n_rows, d)


def test_bitmap_helpers():
    rng = np.random.RandomState(5)
    n = 1000
    ids = rng.permutation(n)[:77]
    w = M.pack_bits(ids, n)
    got = M.unpack_bits(w, n)
    assert got.sum() == 77 and got[ids].all() and len(w) == 32 and all(M.get_bit(w, int(i)) for i in ids)
    start = rng.randint(0, 2 ** 32, 32, dtype=np.uint64).astype(np.uint32)
    for first, last in ((0, 0), (5, 6), (5, 37), (31, 33), (32, 64), (70, 999), (0, 1000)):
        f = M.bits_fill(start, first, last)
        a, b = M.unpack_bits(start, 1024), M.unpack_bits(f, 1024)
        inside = (np.arange(1024) >= first) & (np.arange(1024) < last)
        assert b[inside].all() and np.array_equal(a[~inside], b[~inside])
    touched = np.unique(ids >> 5)
    clean = start.copy()
    clean[touched] = 0
    withneg = np.concatenate([ids, [-1, -7]])
    s = M.batch_bits(withneg, clean, 1)
    assert np.array_equal(M.unpack_bits(s, 1024), M.unpack_bits(clean, 1024) | np.isin(np.arange(1024), ids))
    assert np.array_equal(M.batch_bits(withneg, s, 0), clean)
