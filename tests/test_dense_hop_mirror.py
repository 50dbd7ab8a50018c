"""CPU: the dense backward mirrors of tests/sparse_hop_mirror.py (bwd1_dense, bwd2_dense) -- the fp64 contract SPMM_BWD1 and SPMM_BWD2
are held to in test_gpu_dense_hops.py -- checked for every case and seed the GPU tests use: (a) against scipy fp64 products plus the
epilogue; (b) an fp32 evaluation of the same loops stays inside the derived bound (k + 4) 2^-24 S, so the reference alone stays inside
the bound; (c) two passes over the entries split by column, the first pass's sums handed over as y_in, are the one-pass result;
(d) the bound sees a single entry: zeroing the entry of a degree-1 row moves the result by more than 1e3 bounds; (e) the planted
situations are really in the inputs."""
import numpy as np
import pytest
import scipy.sparse as sp

import dense_hop_cases as D
import sparse_hop_cases as K
import sparse_hop_mirror as M

FP64 = 1e-13    # |mirror - scipy| <= FP64 * S: both are fp64 sums of the same terms in different orders (k <= 2100 terms, u = 1.1e-16)


def close64(got, ref, s):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - ref) <= FP64 * s + 1e-300))


def inside(f32, ref, k, s):
    return bool(np.all(np.abs(f32.astype(np.float64) - ref) <= M.bound(k, s)))


def degree_one_row(g, x):
    """a row with one stored entry whose column's operand row is not zero"""
    for r in np.flatnonzero(g.lens == 1):
        if x[g.a.indices[g.a.indptr[r]]].all():
            return int(r)
    raise AssertionError("no degree-1 row")


def without_entries(a_row):
    return sp.csr_matrix((np.zeros_like(a_row.data), a_row.indices, a_row.indptr), shape=a_row.shape)


def test_case_lists_cover_every_width_mode_and_graph():
    for d in D.WIDTHS:
        assert {m for m, _, dd in D.ONE_PASS if dd == d} == {"bwd1", "bwd2"}
        assert {k for _, k, dd in D.ONE_PASS if dd == d} == (set(D.KINDS) if d < 1024 else {"hub", "rect"})
    for mode in ("bwd1", "bwd2"):
        assert {k for m, k, _ in D.ONE_PASS if m == mode} == set(D.KINDS)
        assert {k for m, k, _ in D.TWO_PASS_CASES if m == mode} == {"hub", "rect", "giant"}
        assert {d for m, _, d in D.TWO_PASS_CASES if m == mode} == set(D.WIDTHS)
    assert {c for _, _, c in D.BWD2_CASES} == {1.0, 0.3} and {c for _, _, c, _ in D.LIMIT_CASES} == {1.0, 0.3}
    assert {lim for _, _, _, lim in D.LIMIT_CASES} == {600, 577} and {k for k, _, _, _ in D.LIMIT_CASES} == {"rect", "rect_tail"}
    g = D.graph("rect_tail")
    for limit in (577, 600):   # a long row (a giant one under spmm_giant = 64) on each side of the limit
        assert g.hubs[0] < limit <= D.TAIL_ROW < g.n_rows and g.lens[g.hubs[0]] > 200 and g.lens[D.TAIL_ROW] >= 200
    assert (D.graph("rect").a[:D.TAIL_ROW] != g.a[:D.TAIL_ROW]).nnz == 0 and D.graph("rect").lens[D.TAIL_ROW] < 64


@pytest.mark.parametrize("kind,d", D.all_bwd1())
def test_bwd1_dense_mirror(kind, d):
    cs = D.bwd1_case(kind, d)
    g = cs.g
    A = g.a.astype(np.float64)
    ref = M.bwd1_dense(g.a, cs.g_am, cs.g_ax, cs.x_in, cs.ax)
    # (a) scipy
    dm = A @ cs.g_am.astype(np.float64)
    assert close64(ref.u, cs.g_ax + dm * cs.x_in, ref.s_u) and close64(ref.t, dm * cs.ax, ref.s_t)
    assert np.array_equal(ref.k, g.lens) and ref.nz.all() and ref.written.all()
    # (b) fp32 in entry order
    f32 = M.bwd1_dense(g.a, cs.g_am, cs.g_ax, cs.x_in, cs.ax, dtype=np.float32)
    assert f32.u.dtype == np.float32 and f32.t.dtype == np.float32
    assert inside(f32.u, ref.u, ref.k, ref.s_u) and inside(f32.t, ref.t, ref.k, ref.s_t)
    # (c) two passes
    first, second = K.split_by_column(g.a, g.n_cols // 3)
    y1 = M.spmm_filtered(first, cs.g_am).y
    two = M.bwd1_dense(second, cs.g_am, cs.g_ax, cs.x_in, cs.ax, y_in=y1)
    assert close64(two.u, ref.u, ref.s_u) and close64(two.t, ref.t, ref.s_t)
    assert np.array_equal(two.k, np.diff(second.indptr) + 1)
    f32 = M.bwd1_dense(second, cs.g_am, cs.g_ax, cs.x_in, cs.ax, y_in=y1.astype(np.float32), dtype=np.float32)
    assert inside(f32.u, two.u, two.k, two.s_u) and inside(f32.t, two.t, two.k, two.s_t)
    # (d) sharpness
    r = degree_one_row(g, cs.g_am)
    row = g.a[r:r + 1]
    sl = slice(r, r + 1)
    full = M.bwd1_dense(row, cs.g_am, cs.g_ax[sl], cs.x_in[sl], cs.ax[sl])
    gone = M.bwd1_dense(without_entries(row), cs.g_am, cs.g_ax[sl], cs.x_in[sl], cs.ax[sl])
    assert full.k[0] == 1 and np.array_equal(full.t, ref.t[sl])
    assert np.all(np.abs(full.t - gone.t) > 1e3 * M.bound(full.k, full.s_t))
    assert np.median(np.abs(full.u - gone.u) / M.bound(full.k, full.s_u)) > 1e3
    # (e) the planted situations
    for e in g.empty:
        assert g.lens[e] == 0 and np.array_equal(ref.u[e], cs.g_ax[e].astype(np.float64)) and not ref.t[e].any() and not ref.s_t[e].any()
    assert not cs.g_am[D.ZERO_BLOCK].any() and cs.g_am[:D.ZERO_BLOCK.start].all() and cs.g_am[D.ZERO_BLOCK.stop:].all()
    assert all(g.lens[h] >= 600 for h in g.hubs) and (ref.s_t[g.hubs[0]] != 0).all()
    assert cs.x_in.all() and cs.ax.all() and cs.g_ax.all()      # dense: no operand row is zero by accident


@pytest.mark.parametrize("kind,d,c,limit", D.all_bwd2())
def test_bwd2_dense_mirror(kind, d, c, limit):
    cs = D.bwd2_case(kind, d, limit)
    g = cs.g
    A = g.a.astype(np.float64)
    own = limit or g.n_rows
    assert cs.t.shape == (own, d) and cs.res.shape == (own, d)
    au = A @ cs.u.astype(np.float64)
    eg = np.where(cs.p > 0, 1.0, np.exp(np.minimum(cs.p, 0).astype(np.float64)))
    first, second = K.split_by_column(g.a, g.n_cols // 3)
    y1 = M.spmm_filtered(first, cs.u).y
    r1 = degree_one_row(g, cs.u)
    for res in (cs.res, None):
        ref = M.bwd2_dense(g.a, cs.u, cs.t, cs.p, c, res=res, own_row_limit=limit)
        # (a) scipy
        gx = au.copy()
        gx[:own] += cs.t
        dp = c * gx * eg
        if res is not None:
            dp[:own] += res
        assert close64(ref.gx, gx, ref.s_gx) and close64(ref.dp, dp, ref.s_dp)
        assert np.array_equal(ref.k, g.lens)
        # (b) fp32 in entry order
        f32 = M.bwd2_dense(g.a, cs.u, cs.t, cs.p, c, res=res, own_row_limit=limit, dtype=np.float32)
        assert f32.dp.dtype == np.float32 and f32.gx.dtype == np.float32
        assert inside(f32.gx, ref.gx, ref.k, ref.s_gx) and inside(f32.dp, ref.dp, ref.k, ref.s_dp)
        # (c) two passes
        two = M.bwd2_dense(second, cs.u, cs.t, cs.p, c, res=res, y_in=y1, own_row_limit=limit)
        assert close64(two.gx, ref.gx, ref.s_gx) and close64(two.dp, ref.dp, ref.s_dp)
        assert np.array_equal(two.k, np.diff(second.indptr) + 1)
        f32 = M.bwd2_dense(second, cs.u, cs.t, cs.p, c, res=res, y_in=y1.astype(np.float32), own_row_limit=limit, dtype=np.float32)
        assert inside(f32.gx, two.gx, two.k, two.s_gx) and inside(f32.dp, two.dp, two.k, two.s_dp)
    # (d) sharpness, first with t = 0 and no residual: every element moves by its whole magnitude
    row = g.a[r1:r1 + 1]
    sl = slice(r1, r1 + 1)
    t0 = np.zeros((1, d), np.float32)
    full = M.bwd2_dense(row, cs.u, t0, cs.p[sl], c)
    gone = M.bwd2_dense(without_entries(row), cs.u, t0, cs.p[sl], c)
    assert full.k[0] == 1
    assert np.all(np.abs(full.gx - gone.gx) > 1e3 * M.bound(full.k, full.s_gx))
    assert np.all(np.abs(full.dp - gone.dp) > 1e3 * M.bound(full.k, full.s_dp))
    # ... and with t and the residual in: the typical element still moves by far more than a thousand bounds
    if r1 < own:
        full = M.bwd2_dense(row, cs.u, cs.t[sl], cs.p[sl], c, res=cs.res[sl])
        gone = M.bwd2_dense(without_entries(row), cs.u, cs.t[sl], cs.p[sl], c, res=cs.res[sl])
        assert np.median(np.abs(full.gx - gone.gx) / M.bound(full.k, full.s_gx)) > 1e3
    # (e) the planted situations
    ref = M.bwd2_dense(g.a, cs.u, cs.t, cs.p, c, res=cs.res, own_row_limit=limit)
    for e in g.empty:
        assert g.lens[e] == 0
        if e < own:
            assert np.array_equal(ref.gx[e], cs.t[e].astype(np.float64))
        else:
            assert not ref.gx[e].any() and not ref.dp[e].any()
    assert not cs.u[D.ZERO_BLOCK].any() and cs.u[:D.ZERO_BLOCK.start].all() and cs.u[D.ZERO_BLOCK.stop:].all()
    for r in D.p_rows(g):
        assert np.array_equal(cs.p[r, :4].view(np.int32), D.P_PLANT.view(np.int32))
        assert np.signbit(cs.p[r, 1]) and not np.signbit(cs.p[r, 0]) and cs.p[r, 2] == np.finfo(np.float32).tiny
        assert np.array_equal(M.elu_grad(cs.p[r, :3].astype(np.float64)), [1.0, 1.0, 1.0])
        assert M.elu_grad(cs.p[r, 3:4].astype(np.float64))[0] == np.exp(-20.0)
    assert (cs.p[D.POS_ROW] > 0).all() and (cs.p[D.NEG_ROW] < 0).all() and (cs.p[861] < 0).all()
    if limit:
        assert 0 < limit < g.n_rows and g.empty[-1] >= limit and 860 >= limit and g.lens[g.hubs[0]] >= 1200 and g.hubs[0] < limit
        behind = slice(limit, g.n_rows)
        assert close64(ref.gx[behind], au[behind], ref.s_gx[behind]) and close64(ref.dp[behind], (c * au * eg)[behind], ref.s_dp[behind])
