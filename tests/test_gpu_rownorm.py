"""-m gpu: the row normalisation without a row list (gss_rownorm_fwd) and its backward fused with ELU' on the batch rows
(gss_rownorm_elu_bwd, and gss_rownorm_elu_bwd_ex with the batch-position map's side write, as a plan calls it) of csrc/elementwise.hip,
at one width per (lane group, VPL) class of row_geometry and at the widths that fill their lane group only partly (48, 192, 320, 576),
with batch sizes on every tail of rows_per_block.  Cases: tests/rownorm_cases.py; contract and derived bound: tests/rownorm_mirror.py
(checked on the CPU by tests/test_rownorm_mirror.py).

Backward: per element |dx - ref| <= (m + 3) 2^-24 S_dx and |dp - ref| <= (m + 7) 2^-24 S_dp, m = 4 VPL + log2(LPR) -- derived in the
mirror, no measured tolerance.  dx_b and dp_b are b rows in front of pre-filled rows that must stay so; pos_set starts as -7 and must
hold pos_set[idx[r]] = r and -7 elsewhere; pos_set = NULL and the 11-argument entry give the same bits.  Forward: E and inv_den within
tolerances.DENSE_STEP_BOUND (the bounds gss_rownorm_fwd_rows is held to), the bits of gss_rownorm_fwd_rows on listed rows, the zero row
exactly, nothing behind row n.  No test provokes a fault: idx and the row lists hold unique valid rows, refusals are refused on the host.

Largest error / bound ratios observed on the MI355X over all batch sizes and both c (GSS_RECORD_PARITY; 1.0 would be the bound itself),
dx / dp by width: 16 0.21 / 0.27, 32 0.16 / 0.23, 48 0.16 / 0.22, 64 0.17 / 0.24, 128 0.14 / 0.22, 192 0.13 / 0.20, 256 0.13 / 0.22,
320 0.10 / 0.17, 512 0.094 / 0.19, 576 0.065 / 0.13, 1024 0.073 / 0.14."""
import numpy as np
import pytest

import dense_step_mirror as DM
import rownorm_cases as K
import rownorm_mirror as M
import tolerances as T
from conftest import record_measured
from guarded import PREFILL, Out, bits, close, cu, ptr, written

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import gcn_drug_repurposing_amd as pkg
    from gcn_drug_repurposing_amd import _lib

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib = pkg.load(), _lib
    ns.st = lambda: _lib.current_stream()
    return ns


def last_error(G):
    return G.lib.gss_last_error().decode()


def prefilled(x):
    return bits(x) == np.int32(PREFILL)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def run_bwd(G, D, d, b, c, entry):
    """entry: "ex" (with pos_set), "ex-null" (pos_set = NULL) or "11-argument" -> dx_b, dp_b [b + GUARD_ROWS][d], pos_set [N] or None"""
    dx, dp = Out(b + K.GUARD_ROWS, d), Out(b + K.GUARD_ROWS, d)
    pos = Out(K.N, fill=K.POS_FREE, dtype=torch.int32) if entry == "ex" else None
    args = [d, ptr(D["de"]), ptr(D["idx"]), b, ptr(D["e"]), ptr(D["inv_den"]), ptr(D["p"]), c, dx.ptr, dp.ptr]
    if entry == "11-argument":
        G._lib.check(G.lib.gss_rownorm_elu_bwd(*args, G.st()))
    else:
        G._lib.check(G.lib.gss_rownorm_elu_bwd_ex(*args, None if pos is None else pos.ptr, G.st()))
    return dx.host("dx_b"), dp.host("dp_b"), None if pos is None else pos.host("pos_set")


@pytest.mark.parametrize("d", K.WIDTHS)
def test_backward_at_every_tail_of_the_block(G, d):
    t = K.table(d)
    table = {k: cu(t[k]) for k in ("e", "inv_den", "p")}
    worst = {"dx": 0.0, "dp": 0.0}
    try:
        for b in K.BATCHES:
            bt = K.batch(d, b)
            D = dict(table, de=cu(bt["de"]), idx=cu(bt["idx"]))
            for c in K.CS:
                what = f"d={d} b={b} c={c}"
                ref = M.backward(bt["de"], bt["idx"], t["e"], t["inv_den"], t["p"], c)
                dx, dp, pos = run_bwd(G, D, d, b, c, "ex")
                for key, got, want, lim in (("dx", dx, ref.dx, M.bound_dx(d, ref.s_dx)), ("dp", dp, ref.dp, M.bound_dp(d, ref.s_dp))):
                    assert not prefilled(got[:b]).any(), f"{what} {key}: a piece of a batch row keeps the pre-fill"
                    assert prefilled(got[b:]).all(), f"{what} {key}: a row behind b was written"
                    err = np.abs(got[:b].astype(np.float64) - want)
                    with np.errstate(all="ignore"):
                        ratio = np.nan_to_num(np.where(err == 0, 0.0, err / lim), nan=np.inf)
                    worst[key] = max(worst[key], float(ratio.max()))
                    assert (err <= lim).all(), (f"{what} {key}: {int((err > lim).sum())} elements beyond the derived bound, worst {ratio.max():.3f} x in "
                                                f"batch row {int(ratio.max(1).argmax())} (node row {bt['idx'][int(ratio.max(1).argmax())]})")
                assert np.array_equal(pos, M.pos_set(bt["idx"], K.N, K.POS_FREE)), f"{what}: pos_set is not idx's inverse on the members and -7 elsewhere"
                for entry in ("ex-null", "11-argument", "ex"):
                    dx2, dp2, _ = run_bwd(G, D, d, b, c, entry)
                    assert same(dx, dx2) and same(dp, dp2), f"{what}: {entry} differs from gss_rownorm_elu_bwd_ex with pos_set"
                # p > 0 takes the branch elu' = 1: the smallest normal among the planted values, and the all-positive row (+0, -0 and
                # -20 go through expf and are held by the bound like every other element)
                where = np.flatnonzero(bt["idx"] == K.P_ROW)
                if len(where) and c == 1.0:
                    r = int(where[0])
                    assert same(dp[r, 2], dx[r, 2]), f"{what}: elu'(the smallest normal) is not 1"
                where = np.flatnonzero(bt["idx"] == K.POS_ROW)
                if len(where) and c == 1.0:
                    assert same(dp[int(where[0])], dx[int(where[0])]), f"{what}: the all-positive row"
    finally:
        print(f"rownorm_bwd[{d}]: error / bound dx {worst['dx']:.3f}, dp {worst['dp']:.3f}")
        record_measured(f"rownorm_bwd[{d}]", **worst)


@pytest.mark.parametrize("d", K.WIDTHS)
def test_forward_without_a_list(G, d):
    t = K.table(d)
    x_d = cu(t["x"])
    ref_e, ref_inv = DM.normalize(t["x"])
    for n in K.FWD_N:
        what = f"d={d} n={n}"
        e, inv = Out(n + K.GUARD_ROWS, d), Out(n + K.GUARD_ROWS)
        G._lib.check(G.lib.gss_rownorm_fwd(n, d, ptr(x_d), e.ptr, inv.ptr, G.st()))
        e, inv = e.host("E"), inv.host("inv_den")
        written(e[:n], f"{what} E"), written(inv[:n], f"{what} inv_den")
        assert prefilled(e[n:]).all() and prefilled(inv[n:]).all(), f"{what}: written behind row n"
        close(e[:n], ref_e[:n], T.DENSE_STEP_BOUND["e"], np.abs(ref_e).max(), f"{what} E")
        live = np.setdiff1d(np.arange(n), [K.ZERO_ROW])
        if len(live):
            err = (np.abs(inv[live].astype(np.float64) - ref_inv[live]) / ref_inv[live]).max()
            print(f"{what} inv_den: err {err:.3e} (bound {T.DENSE_STEP_BOUND['inv_den']:.1e})")
            assert err <= T.DENSE_STEP_BOUND["inv_den"], f"{what} inv_den: {err:.3e}"
        assert not e[K.ZERO_ROW].any() and inv[K.ZERO_ROW] == np.float32(1e12), f"{what}: the zero row"
        # the listed rows of gss_rownorm_fwd_rows: the same bits, and nothing else written
        lst = K.fwd_list(d, n)
        e2, inv2 = Out(n + K.GUARD_ROWS, d), Out(n + K.GUARD_ROWS)
        G._lib.check(G.lib.gss_rownorm_fwd_rows(len(lst), d, ptr(x_d), e2.ptr, inv2.ptr, ptr(cu(lst)), G.st()))
        e2, inv2 = e2.host("E (list)"), inv2.host("inv_den (list)")
        rows = lst.astype(np.int64)
        other = np.ones(n + K.GUARD_ROWS, bool)
        other[rows] = False
        assert same(e2[rows], e[rows]) and same(inv2[rows], inv[rows]), f"{what}: gss_rownorm_fwd differs from gss_rownorm_fwd_rows on listed rows"
        assert prefilled(e2[other]).all() and prefilled(inv2[other]).all(), f"{what}: gss_rownorm_fwd_rows wrote an unlisted row"


def test_no_rows_is_no_launch_and_refusals_launch_nothing(G):
    d, b = 48, 5
    t, bt = K.table(d), K.batch(d, b)
    D = {k: cu(v) for k, v in dict(t, **bt).items() if k != "x"}
    dx, dp, pos = Out(b, d), Out(b, d), Out(K.N, fill=K.POS_FREE, dtype=torch.int32)
    good = [d, ptr(D["de"]), ptr(D["idx"]), b, ptr(D["e"]), ptr(D["inv_den"]), ptr(D["p"]), 0.3, dx.ptr, dp.ptr, pos.ptr, G.st()]

    def swap(i, v):
        return good[:i] + [v] + good[i + 1:]

    assert G.lib.gss_rownorm_elu_bwd_ex(*swap(3, 0)) == 0
    assert G.lib.gss_rownorm_elu_bwd_ex(*swap(0, 20)) != 0 and "d=20" in last_error(G), last_error(G)
    for i in (1, 2, 4, 5, 6, 8, 9):
        assert G.lib.gss_rownorm_elu_bwd_ex(*swap(i, None)) != 0 and "rownorm_elu_bwd: null operand" in last_error(G), (i, last_error(G))
    assert G.lib.gss_rownorm_elu_bwd_ex(*swap(3, -1)) != 0 and "rownorm_elu_bwd" in last_error(G), last_error(G)
    e, inv = Out(5, d), Out(5)
    x_d = cu(t["x"])
    assert G.lib.gss_rownorm_fwd(0, d, ptr(x_d), e.ptr, inv.ptr, G.st()) == 0
    assert G.lib.gss_rownorm_fwd(5, 20, ptr(x_d), e.ptr, inv.ptr, G.st()) != 0 and "d=20" in last_error(G), last_error(G)
    assert G.lib.gss_rownorm_fwd(5, d, None, e.ptr, inv.ptr, G.st()) != 0 and "rownorm_fwd: null operand" in last_error(G), last_error(G)
    torch.cuda.synchronize()
    assert dx.untouched() and dp.untouched() and e.untouched() and inv.untouched(), "a refused or empty call wrote an output"
    assert (pos.host("pos_set") == K.POS_FREE).all(), "a refused or empty call wrote pos_set"
