"""CPU: tests/rownorm_mirror.py and tests/rownorm_cases.py, which tests/test_gpu_rownorm.py holds gss_rownorm_elu_bwd(_ex) to.  The
fp64 formulas against torch's autograd of F.normalize and F.elu; the geometry port pinned; a float32 evaluation in the kernel's order
inside the derived bound at every case; a dot that misses one float4 of one row rejected by that bound."""
import numpy as np
import pytest

import rownorm_cases as K
import rownorm_mirror as M

# d -> (lpr_log2, VPL, lanes of the last float4 slot that hold data): every (lane group, VPL) class and the partly filled groups
GEOMETRY = {16: (2, 1, 4), 32: (3, 1, 8), 48: (4, 1, 12), 64: (4, 1, 16), 128: (5, 1, 32), 192: (6, 1, 48), 256: (6, 1, 64),
            320: (6, 2, 16), 512: (6, 2, 64), 576: (6, 4, 16), 1024: (6, 4, 64)}


def test_geometry_port_is_pinned():
    assert tuple(GEOMETRY) == K.WIDTHS
    for d, (lg, vpl, last) in GEOMETRY.items():
        d4, got_lg, got_vpl = M.row_geometry(d)
        assert (got_lg, got_vpl) == (lg, vpl) and d4 == d // 4
        full_slots, rem = divmod(d4, 64) if vpl > 1 else (0, d4)
        assert (rem or 64) == last and full_slots + (1 if rem else 0) <= vpl
        assert M.depth(d) == 4 * vpl + lg
    assert {(lg, vpl) for lg, vpl, _ in GEOMETRY.values()} == {(2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (6, 2), (6, 4)}
    assert sorted({M.rows_per_block(d) for d in K.WIDTHS}) == [4, 8, 16, 32, 64]
    # every tail of every rows_per_block: one row, a block less one / whole / and one (64), and for the smaller blocks 3, 4, 5 and 333
    for rpb in (4, 8, 16, 32, 64):
        rem = {b % rpb for b in K.BATCHES}
        assert 1 in rem and len(rem) >= 3, (rpb, rem)
    assert {63, 64, 65} <= set(K.BATCHES) and {3, 4, 5} <= set(K.BATCHES)


def test_batches_hold_the_planted_rows():
    for d in (16, 576):
        t = K.table(d)
        assert np.array_equal(t["p"][K.P_ROW, :4].view(np.int32), K.P_PLANT.view(np.int32))
        assert (t["p"][K.POS_ROW] > 0).all() and (t["p"][K.NEG_ROW] < 0).all()
        for b in K.BATCHES:
            idx = K.batch(d, b)["idx"]
            assert len(np.unique(idx)) == b and idx[-1] == K.N - 1
            if b >= 2:
                assert idx[0] == K.ZERO_ROW
            if b >= 5:
                assert set(K.MUST) <= set(idx.tolist())
        for n in K.FWD_N:
            lst = K.fwd_list(d, n)
            assert len(np.unique(lst)) == len(lst) and lst.min() == 0 and lst.max() == n - 1


@pytest.mark.parametrize("d", (16, 48, 320))
def test_fp64_formulas_are_autograd_s(d):
    torch = pytest.importorskip("torch")
    t, bt = K.table(d), K.batch(d, 65)
    live = bt["idx"] != K.ZERO_ROW
    idx = bt["idx"][live]
    x = torch.from_numpy(t["x"].astype(np.float64)[idx]).requires_grad_()
    e = torch.nn.functional.normalize(x, dim=1)
    e.backward(torch.from_numpy(bt["de"][live].astype(np.float64)))
    got = M.backward(bt["de"][live], idx, t["e"], t["inv_den"], t["p"], 0.3)
    # (e and inv_den are float32 roundings: 2^-24 relative each)
    assert np.abs(got.dx - x.grad.numpy()).max() <= 1e-6 * np.abs(got.dx).max()
    p = torch.from_numpy(t["p"].astype(np.float64)[idx]).requires_grad_()
    (0.3 * torch.nn.functional.elu(p)).backward(x.grad)
    assert np.abs(got.dp - p.grad.numpy()).max() <= 1e-6 * np.abs(got.dp).max()
    # the zero row: e = 0, inv_den = 1e12 -> dx = 1e12 de
    z = M.backward(bt["de"][~live], bt["idx"][~live], t["e"], t["inv_den"], t["p"], 1.0)
    assert np.allclose(z.dx, 1e12 * bt["de"][~live].astype(np.float64), rtol=1e-7)


@pytest.mark.parametrize("d", K.WIDTHS)
def test_float32_in_the_kernel_s_order_sits_inside_the_bound_and_a_dropped_float4_does_not(d):
    t = K.table(d)
    worst = {"dx": 0.0, "dp": 0.0}
    miss = np.inf
    for b in K.BATCHES:
        bt = K.batch(d, b)
        for c in K.CS:
            ref = M.backward(bt["de"], bt["idx"], t["e"], t["inv_den"], t["p"], c)
            dx, dp = M.backward_fp32(bt["de"], bt["idx"], t["e"], t["inv_den"], t["p"], c)
            for key, got, want, lim in (("dx", dx, ref.dx, M.bound_dx(d, ref.s_dx)), ("dp", dp, ref.dp, M.bound_dp(d, ref.s_dp))):
                err = np.abs(got.astype(np.float64) - want)
                assert (err <= lim).all(), (d, b, c, key)
                with np.errstate(all="ignore"):
                    worst[key] = max(worst[key], float(np.where(err == 0, 0.0, err / lim).max()))
            # one float4 of one row missing from the dot: the last one (a partly filled group's) and the first, in a live row
            r = int(np.flatnonzero(bt["idx"] != K.ZERO_ROW)[-1])
            if not bt["de"][r].any():
                continue
            for f4 in (0, d // 4 - 1):
                dx, dp = M.backward_fp32(bt["de"], bt["idx"], t["e"], t["inv_den"], t["p"], c, drop=(r, f4))
                assert (np.abs(dx.astype(np.float64) - ref.dx) > M.bound_dx(d, ref.s_dx)).any(), (d, b, c, f4)
                assert (np.abs(dp.astype(np.float64) - ref.dp) > M.bound_dp(d, ref.s_dp)).any(), (d, b, c, f4)
                miss = min(miss, float((np.abs(dx.astype(np.float64) - ref.dx)[r] / M.bound_dx(d, ref.s_dx)[r]).max()))
    print(f"d={d}: float32 error / bound dx {worst['dx']:.3f}, dp {worst['dp']:.3f}; a dropped float4 is at least {miss:.0f} bounds away")
    assert 0 < worst["dx"] < 1 and 0 < worst["dp"] < 1


def test_pos_set_mirror():
    idx = K.batch(64, 65)["idx"]
    pos = M.pos_set(idx, K.N, K.POS_FREE)
    assert (pos[idx] == np.arange(65)).all() and (pos != K.POS_FREE).sum() == 65
