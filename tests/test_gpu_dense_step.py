"""-m gpu: the dense half of a plan's step, launcher by launcher, against its fp64 contract (tests/dense_step_mirror.py).  A plan reaches
csrc/dense.hip through dense_fwd with a row list, dense_fwd_first + acc_in_p, dense_fwd_norm, rownorm_fwd over a row list, wgrad_partial at
a slice offset, wgrad_partial_pair, wgrad_reduce over several problems, wgrad_reduce_adam, adam_step4 and transpose2; the entry points
gss_dense_fwd_rows ... gss_transpose2 call exactly those.

Inputs come from tests/dense_step_cases.py.  Bounds (tests/tolerances.py): P, x_next, gW, gb 3e-6 of the largest entry, as test_dense_fwd
and test_dense_bwd_weight; Adam 2.5e-7 x max(1, |ref|), as test_adam_matches_torch_semantics; E, inv_den and E_B 8 x the error of the
mirror's own formulas in numpy float32, or 3e-6 where that is larger.  Where the code states a contract of equal bits -- the listed rows
of a pass over a row list against the pass over all rows, two launches against one, the weight-stationary kernel against the staged
tiles, E_B against E, two problems in one launch against two launches -- the comparison is exact.  The integer regime of the weight
gradient is exact in fp32 in any order: a slice dropped, read twice or read from the wrong offset is an exact mismatch.

Every output sits between canary elements and starts as a NaN of a recognisable payload: it must be fully written where the contract
says so and keep the pre-fill where it says it is not written (rows beyond n, unlisted rows, rows whose list entry is negative, E_B slots
no member maps to, slices outside [slice0, slice0 + ns)).  No test provokes a fault: every launch that runs gets valid arguments, the
refusals are refused on the host before any launch."""
import ctypes as C

import numpy as np
import pytest

import dense_step_cases as K
import dense_step_mirror as M
import tolerances as T
from guarded import PREFILL, Out, bits, close, cu, knobs, ptr, written

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL = -22
POS_FREE = -7                        # a batch-position map entry nobody wrote
PLAIN = T.DENSE_STEP_PLAIN
NAMES = ("W1", "b1", "W2", "b2")
# Adam's default betas AS THE LIBRARY RECEIVES THEM: the ABI carries them as float, and the kernels form 1 - beta from that float, as torch
# does from the double it is given.  The reference gets the same two numbers.  (With the doubles 0.9 / 0.999 in the reference instead, 1 - beta2
# differs by 1.3e-5 relative -- 0.001 against 1 - 0.999f = 0.00099998713 -- and so does v: measured on an MI355X v 1.3e-5, m 3.0e-7 of the
# largest entry, the parameters 6e-8, inside their bound either way.)
BETA1, BETA2, ADAM_EPS = float(np.float32(0.9)), float(np.float32(0.999)), 1e-8


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
    ns.dev = {}
    return ns


def last_error(G):
    return G.lib.gss_last_error().decode()


def filled(a):
    """a guarded buffer that starts as the host array `a` (float32 or int32)"""
    o = Out(*a.shape, dtype=torch.float32 if a.dtype == np.float32 else torch.int32)
    o.t.copy_(cu(a).reshape(-1))
    return o


def prefilled(x):
    return bits(x) == np.int32(PREFILL)


# ================================================================ the forward projection
def operands(G, regime, n, d, length=None):
    """the case and its device copies (a few cases stay cached: the long ones are shared between tests)"""
    key = (regime, n, d, length)
    c = K.forward(*key)
    if key not in G.dev:
        if len(G.dev) >= 6:
            G.dev.clear()
        G.dev[key] = {k: cu(c[k]) for k in ("ax", "am", "w1", "b1", "w2", "b2", "p_prev", "pos", "list") if k in c}
    return c, G.dev[key]


def call_fwd(G, c, D, prev, lst=None, acc=None):
    """gss_dense_fwd_rows -> rc, P, x_next as guarded [N][d] buffers; acc: the buffer gss_dense_fwd_first wrote (acc_in_p)"""
    p, x = acc if acc is not None else Out(c["n"], c["d"]), Out(c["n"], c["d"])
    rc = G.lib.gss_dense_fwd_rows(c["n"] if lst is None else lst.numel(), c["d"], ptr(D["ax"]), ptr(D["am"]), ptr(D["w1"]), ptr(D["b1"]), ptr(D["w2"]),
                                  ptr(D["b2"]), ptr(D["p_prev"]) if prev else None, K.DECAY, p.ptr, x.ptr, ptr(lst), int(acc is not None), G.st())
    return rc, p, x


def call_norm(G, c, D, prev, lst=None, rows_out=None, pos=None, acc=None, d=None):
    """gss_dense_fwd_norm -> rc, P, E [N][d], inv_den [N]"""
    p, e, inv = acc if acc is not None else Out(c["n"], c["d"]), Out(c["n"], c["d"]), Out(c["n"])
    rc = G.lib.gss_dense_fwd_norm(c["n"] if lst is None else lst.numel(), d or c["d"], ptr(D["ax"]), ptr(D["am"]), ptr(D["w1"]), ptr(D["b1"]),
                                  ptr(D["w2"]), ptr(D["b2"]), ptr(D["p_prev"]) if prev else None, K.DECAY, p.ptr, e.ptr, inv.ptr, ptr(lst),
                                  None if rows_out is None else rows_out.ptr, ptr(pos), int(acc is not None), G.st())
    return rc, p, e, inv


def rows_of(c, lst):
    """(node rows a launch covers, mask of the others)"""
    rows = np.arange(c["n"]) if lst is None else c["list"][c["list"] >= 0].astype(np.int64)
    other = np.ones(c["n"], bool)
    other[rows] = False
    return rows, other


def check_plain(c, ref, rows, other, p, x, what):
    """P and x_next of the covered rows against the mirror, the zero rows exactly, every other row untouched"""
    written(p[rows], f"{what} P"), written(x[rows], f"{what} x_next")
    close(p[rows], ref["p"][rows], PLAIN, np.abs(ref["p"]).max(), f"{what} P")
    close(x[rows], ref["x"][rows], PLAIN, np.abs(ref["x"]).max(), f"{what} x_next")
    z = np.intersect1d(c["zero"], rows)
    assert not p[z].any() and not x[z].any(), f"{what}: a zero row is not zero bit for bit"
    assert prefilled(p[other]).all() and prefilled(x[other]).all(), f"{what}: a row outside the launch was written"


def check_norm(c, ref, rows, other, p, e, inv, what):
    written(p[rows], f"{what} P"), written(e[rows], f"{what} E"), written(inv[rows], f"{what} inv_den")
    close(p[rows], ref["p"][rows], PLAIN, np.abs(ref["p"]).max(), f"{what} P")
    close(e[rows], ref["e"][rows], T.DENSE_STEP_BOUND["e"], np.abs(ref["e"]).max(), f"{what} E")
    z = np.intersect1d(c["zero"], rows)
    live = np.setdiff1d(rows, z)
    if len(live):
        err = (np.abs(inv[live].astype(np.float64) - ref["inv_den"][live]) / ref["inv_den"][live]).max()
        print(f"{what} inv_den: err {err:.3e} (bound {T.DENSE_STEP_BOUND['inv_den']:.1e})")
        assert err <= T.DENSE_STEP_BOUND["inv_den"], f"{what} inv_den: {err:.3e} per row"
    assert not p[z].any() and not e[z].any() and (inv[z] == np.float32(1e12)).all(), f"{what}: a zero row gives P = 0, E = 0, inv_den = 1e12 exactly"
    assert prefilled(p[other]).all() and prefilled(e[other]).all() and prefilled(inv[other]).all(), f"{what}: a row outside the launch was written"


def same_rows(got, full, rows, what):
    assert np.array_equal(bits(got[rows]), bits(full[rows])), f"{what}: listed rows differ from the pass over all rows"


def run_plain_list(G, regime, n, d, length, prevs=(False, True)):
    c, D = operands(G, regime, n, d, length)
    rows, other = rows_of(c, True)
    every, none = rows_of(c, None)
    for prev in prevs:
        what = f"{regime} d={d} list={length} prev={prev}"
        ref = K.forward_reference(regime, n, d, length, prev)
        rc, fp, fx = call_fwd(G, c, D, prev)
        G._lib.check(rc, what)
        fp, fx = fp.host("P"), fx.host("x_next")
        check_plain(c, ref, every, none, fp, fx, what + " (all rows)")
        rc, p, x = call_fwd(G, c, D, prev, D["list"])
        G._lib.check(rc, what)
        p, x = p.host("P"), x.host("x_next")
        check_plain(c, ref, rows, other, p, x, what)
        same_rows(p, fp, rows, what + " P"), same_rows(x, fx, rows, what + " x_next")


@pytest.mark.parametrize("length", K.ROWS_LENS)
@pytest.mark.parametrize("d", K.ROWS_SPLIT_D + K.ROWS_WAVE_D)
def test_fwd_short_row_lists(G, d, length):
    """gemm_rows_split_kernel (d = 64, 128, 256) and the one-wave tiles (d = 16, 32, 48, 192) over 1 .. 100 listed rows of 300"""
    for regime in ("unit", "zero"):
        run_plain_list(G, regime, K.ROWS_N, d, length)


@pytest.mark.parametrize("n,d,length", K.LONG_ROWS)
def test_fwd_long_row_lists(G, n, d, length):
    """the smallest lists that leave the short-list branch: the staged tiles in the MFMA layout, rows through the list"""
    run_plain_list(G, "unit", n, d, length)


@pytest.mark.parametrize("n", K.SPLIT_N)
@pytest.mark.parametrize("d", K.SPLIT_D)
def test_two_launches_give_the_bits_of_one(G, d, n):
    """dense_fwd_first (PART 1) + acc_in_p (PART 2) against one launch, without and with the fused norm"""
    assert G.lib.gss_dense_fwd_split_available(n, d) == 1
    for regime in ("unit", "zero"):
        c, D = operands(G, regime, n, d)
        every, none = rows_of(c, None)
        for prev in (False, True):
            what = f"{regime} d={d} n={n} prev={prev}"
            ref = K.forward_reference(regime, n, d, None, prev)
            rc, p1, x1 = call_fwd(G, c, D, prev)
            G._lib.check(rc, what)
            p1, x1 = p1.host("P"), x1.host("x_next")
            check_plain(c, ref, every, none, p1, x1, what)
            rc, q1, e1, i1 = call_norm(G, c, D, prev)
            G._lib.check(rc, what)
            q1, e1, i1 = q1.host("P"), e1.host("E"), i1.host("inv_den")
            check_norm(c, ref, every, none, q1, e1, i1, what + " norm")
            for norm in (False, True):
                acc = Out(n, d)
                G._lib.check(G.lib.gss_dense_fwd_first(n, d, ptr(D["ax"]), ptr(D["w1"]), acc.ptr, G.st()), what)
                raw = written(acc.host("acc"), f"{what}: the raw accumulators").copy()
                ref_acc = c["ax"].astype(np.float64) @ c["w1"].astype(np.float64).T
                close(raw, ref_acc, PLAIN, max(np.abs(ref_acc).max(), 1e-30), f"{what} AX W1^T")
                if norm:
                    rc, p2, e2, i2 = call_norm(G, c, D, prev, acc=acc)
                    G._lib.check(rc, what)
                    assert np.array_equal(bits(p2.host("P")), bits(q1)) and np.array_equal(bits(e2.host("E")), bits(e1)), f"{what}: two launches, norm"
                    assert np.array_equal(bits(i2.host("inv_den")), bits(i1)), f"{what}: two launches, inv_den"
                else:
                    rc, p2, x2 = call_fwd(G, c, D, prev, acc=acc)
                    G._lib.check(rc, what)
                    assert np.array_equal(bits(p2.host("P")), bits(p1)) and np.array_equal(bits(x2.host("x_next")), bits(x1)), f"{what}: two launches"


def test_two_launches_are_refused_where_there_is_no_such_form(G):
    """d = 32, a row list, d = 128 under gemm_ws = 1: GSS_EINVAL by name, nothing launched, nothing written"""
    def refused(c, D, d, n, lst=None, first=True):
        acc = Out(c["n"], d)
        if first:
            assert G.lib.gss_dense_fwd_first(n, d, ptr(D["ax"]), ptr(D["w1"]), acc.ptr, G.st()) == EINVAL
            assert "no two-launch form" in last_error(G), last_error(G)
        rc, p, x = call_fwd(G, c, D, True, lst, acc=acc)
        assert rc == EINVAL and "no two-launch form" in last_error(G), last_error(G)
        rc, p, e, inv = call_norm(G, c, D, True, lst, acc=acc)
        assert rc == EINVAL and "no two-launch form" in last_error(G), last_error(G)
        torch.cuda.synchronize()
        for o in (acc, x, e, inv):
            assert o.untouched(), "a refused call wrote an output"

    c, D = operands(G, "unit", 17, 32)
    assert G.lib.gss_dense_fwd_split_available(17, 32) == 0
    refused(c, D, 32, 17)
    c, D = operands(G, "unit", K.ROWS_N, 64, 17)
    assert G.lib.gss_dense_fwd_split_available(17, 64) == 1          # ... of 17 rows without a list
    refused(c, D, 64, 17, D["list"], first=False)
    c, D = operands(G, "unit", 300, 128)
    with knobs(G, gemm_ws=1):
        assert G.lib.gss_dense_fwd_split_available(300, 128) == 0
        refused(c, D, 128, 300)
    assert G.lib.gss_dense_fwd_split_available(300, 128) == 1


# ================================================================ the fused norm
def check_rows_out(c, rows_out, e, by, what):
    """E_B: the slots a member maps to hold E's row bit for bit, every other slot keeps the pre-fill"""
    eb = rows_out.host(f"{what} rows_out")
    want, ok = (M.rows_out_by_list(e, c["list"]) if by == "list" else M.rows_out_by_pos(e, c["pos"], c["b"]))
    assert np.array_equal(bits(eb[ok]), bits(want[ok])), f"{what}: rows_out is not E's rows"
    assert prefilled(eb[~ok]).all(), f"{what}: a rows_out slot nobody maps to was written"
    assert ok.any()


def run_norm_all(G, regime, n, d, what0="", prevs=(False, True)):
    c, D = operands(G, regime, n, d)
    every, none = rows_of(c, None)
    for prev in prevs:
        what = f"{what0}{regime} d={d} n={n} prev={prev}"
        ref = K.forward_reference(regime, n, d, None, prev)
        rc, p, e, inv = call_norm(G, c, D, prev)
        G._lib.check(rc, what)
        p, e, inv = p.host("P"), e.host("E"), inv.host("inv_den")
        check_norm(c, ref, every, none, p, e, inv, what)
        rows_out = Out(c["b"], d)
        rc, p2, e2, inv2 = call_norm(G, c, D, prev, rows_out=rows_out, pos=D["pos"])
        G._lib.check(rc, what)
        p2, e2, inv2 = p2.host("P"), e2.host("E"), inv2.host("inv_den")
        check_norm(c, ref, every, none, p2, e2, inv2, what + " +map")
        check_rows_out(c, rows_out, e2, "pos", what)
        assert np.array_equal(bits(p2), bits(p)) and np.array_equal(bits(e2), bits(e)) and np.array_equal(bits(inv2), bits(inv)), f"{what}: rows_out changed the pass"
    return p, e, inv


def run_norm_list(G, regime, n, d, length, what0="", prevs=(False, True)):
    c, D = operands(G, regime, n, d, length)
    rows, other = rows_of(c, True)
    every, none = rows_of(c, None)
    for prev in prevs:
        what = f"{what0}{regime} d={d} list={length} prev={prev}"
        ref = K.forward_reference(regime, n, d, length, prev)
        rc, fp, fe, fi = call_norm(G, c, D, prev)
        G._lib.check(rc, what)
        fp, fe, fi = fp.host("P"), fe.host("E"), fi.host("inv_den")
        check_norm(c, ref, every, none, fp, fe, fi, what + " (all rows)")
        rows_out = Out(length, d)
        rc, p, e, inv = call_norm(G, c, D, prev, D["list"], rows_out=rows_out)
        G._lib.check(rc, what)
        p, e, inv = p.host("P"), e.host("E"), inv.host("inv_den")
        check_norm(c, ref, rows, other, p, e, inv, what)
        same_rows(p, fp, rows, what + " P"), same_rows(e, fe, rows, what + " E"), same_rows(inv, fi, rows, what + " inv_den")
        check_rows_out(c, rows_out, e, "list", what)


@pytest.mark.parametrize("n", K.NORM_N)
@pytest.mark.parametrize("d", K.NORM_D)
def test_norm_all_rows(G, d, n):
    """EPI_FWD_NORM over all rows: without rows_out, and with E_B through the batch-position map"""
    for regime in ("unit", "zero"):
        run_norm_all(G, regime, n, d)


@pytest.mark.parametrize("length", K.NORM_LENS)
@pytest.mark.parametrize("d", K.NORM_D)
def test_norm_short_row_lists(G, d, length):
    """EPI_FWD_NORM over a row list with rows_out: rows_out[t] = E[list[t]], a skipped entry's slot keeps the pre-fill"""
    for regime in ("unit", "zero"):
        run_norm_list(G, regime, K.ROWS_N, d, length)


@pytest.mark.parametrize("n,d,length", K.NORM_LONG)
def test_norm_long_row_lists(G, n, d, length):
    """16,321 listed rows leave the short-list branch.  d = 256 is the regression test of a defect: launch_gemm used to give such a list the
    one-block tile with grid.y = 1, which wrote 16 of a row's 256 features and normalised the row over those 16; a list under the fused
    norm at d = 256 now takes the whole-row kernel whatever its length"""
    run_norm_list(G, "unit", n, d, length)


@pytest.mark.parametrize("variant", [3, 5])
def test_norm_under_the_forced_tile_shapes(G, variant):
    """gemm_variant 3 (128-node tiles of four waves: at d = 256 the four-wave 256-feature form) and 5 (of eight waves); 2 is every other test"""
    with knobs(G, gemm_variant=variant):
        for d in K.NORM_D:
            for regime in ("unit", "zero"):
                for n in (17, 300):
                    run_norm_all(G, regime, n, d, f"gemm_variant={variant} ", prevs=(True,))
                run_norm_list(G, regime, K.ROWS_N, d, 100, f"gemm_variant={variant} ", prevs=(True,))


def test_norm_weight_stationary(G):
    """gemm_ws = 1 at d = 128: proj_ws_kernel<EPI_FWD_NORM> with and without the position map -- the bits of the staged tiles (its stated
    contract); rows_out over a row list keeps the staged tiles and still gives the right result"""
    d = 128
    for n in (17, 300):
        for regime in ("unit", "zero"):
            with knobs(G, gemm_ws=0):
                staged = run_norm_all(G, regime, n, d, "gemm_ws=0 ", prevs=(True,))
            with knobs(G, gemm_ws=1):
                ws = run_norm_all(G, regime, n, d, "gemm_ws=1 ", prevs=(True,))
                run_norm_all(G, regime, n, d, "gemm_ws=1 ", prevs=(False,))
            for a, b, k in zip(staged, ws, ("P", "E", "inv_den")):
                assert np.array_equal(bits(a), bits(b)), f"{regime} n={n}: {k} of the weight-stationary kernel differs from the staged tiles"
    with knobs(G, gemm_ws=1):
        for regime in ("unit", "zero"):
            run_norm_list(G, regime, K.ROWS_N, d, 100, "gemm_ws=1 ")


def test_norm_refusals(G):
    """d = 48 has no fused norm; rows_out goes with exactly one of a row list and a position map.  By return code and message only"""
    c, D = operands(G, "unit", K.ROWS_N, 48, 17)
    rc, p, e, inv = call_norm(G, c, D, True)
    assert rc == EINVAL and "dense_fwd_norm: needs d in" in last_error(G), last_error(G)
    outs = [p, e, inv]
    c, D = operands(G, "unit", K.ROWS_N, 64, 17)
    for lst, pos in ((D["list"], D["pos"]), (None, None)):
        rows_out = Out(c["b"], 64)
        rc, p, e, inv = call_norm(G, c, D, True, lst, rows_out=rows_out, pos=pos)
        assert rc == EINVAL and "rows_out goes with" in last_error(G), last_error(G)
        outs += [p, e, inv, rows_out]
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused call wrote an output"


@pytest.mark.parametrize("n,d,length", K.rownorm_cases())
def test_rownorm_over_a_row_list(G, n, d, length):
    """gss_rownorm_fwd_rows at the widths without a fused norm"""
    c = K.rownorm(n, d, length)
    x_d, lst_d = cu(c["x"]), cu(c["list"])
    ref_e, ref_inv = M.normalize(c["x"])
    cc = dict(n=n, list=c["list"])
    out = {}
    for lst in (None, lst_d):
        e, inv = Out(n, d), Out(n)
        G._lib.check(G.lib.gss_rownorm_fwd_rows(n if lst is None else length, d, ptr(x_d), e.ptr, inv.ptr, ptr(lst), G.st()))
        e, inv = e.host("E"), inv.host("inv_den")
        rows, other = rows_of(cc, lst)
        what = f"d={d} list={None if lst is None else length}"
        written(e[rows], what), written(inv[rows], what)
        close(e[rows], ref_e[rows], T.DENSE_STEP_BOUND["e"], np.abs(ref_e).max(), f"{what} E")
        z = np.intersect1d(c["zero"], rows)
        live = np.setdiff1d(rows, z)
        if len(live):
            err = (np.abs(inv[live].astype(np.float64) - ref_inv[live]) / ref_inv[live]).max()
            print(f"{what} inv_den: err {err:.3e} (bound {T.DENSE_STEP_BOUND['inv_den']:.1e})")
            assert err <= T.DENSE_STEP_BOUND["inv_den"]
        assert not e[z].any() and (inv[z] == np.float32(1e12)).all(), f"{what}: the zero row"
        assert prefilled(e[other]).all() and prefilled(inv[other]).all(), f"{what}: an unlisted row was written"
        out[lst is None] = (e, inv, rows)
    e, inv, rows = out[False]
    same_rows(e, out[True][0], rows, "E"), same_rows(inv, out[True][1], rows, "inv_den")


# ================================================================ the weight gradient
class Slabs:
    """the partial buffer of `total` slices: [total][d][2 d] weight slabs followed by [total][d] bias slabs, guarded and pre-filled"""

    def __init__(self, total, d):
        self.total, self.d = total, d
        self.out = Out(total * (2 * d * d + d))

    @property
    def ptr(self):
        return self.out.ptr

    def host(self):
        h = self.out.host("the partial buffer")
        nw = self.total * 2 * self.d * self.d
        return h[:nw].reshape(self.total, self.d, 2 * self.d), h[nw:].reshape(self.total, self.d)


def on_device(c):
    return {k: None if c[k] is None else cu(c[k]) for k in ("dp", "ax", "am", "rows")}


def slices(G, n, d, n_max=None):
    ns = G.lib.gss_wgrad_slices(n, d)
    assert 1 <= ns and (n == 0 or ns <= G.lib.gss_wgrad_slices_max(n if n_max is None else n_max, d))
    return ns


def partial(G, c, D, slabs, slice0, n=None):
    ns = C.c_int32(-1)
    rc = G.lib.gss_wgrad_partial(c["n"] if n is None else n, c["d"], ptr(D["dp"]), ptr(D["ax"]), ptr(D["am"]), ptr(D["rows"]), slabs.ptr, slabs.total,
                                 slice0, C.byref(ns), G.st())
    return rc, ns.value


def pair(G, d, c0, D0, s0, c1, D1, s1, slabs, n1=None):
    a, b = C.c_int32(-1), C.c_int32(-1)
    rc = G.lib.gss_wgrad_partial_pair(d, c0["n"], ptr(D0["dp"]), ptr(D0["ax"]), ptr(D0["am"]), ptr(D0["rows"]), s0, c1["n"] if n1 is None else n1,
                                      ptr(D1["dp"]), ptr(D1["ax"]), ptr(D1["am"]), ptr(D1["rows"]), s1, slabs.ptr, slabs.total, C.byref(a), C.byref(b), G.st())
    return rc, a.value, b.value


def grads_out(d):
    return dict(W1=Out(d, d), b1=Out(d), W2=Out(d, d), b2=Out(d))


def reduce(G, d, slabs, nslices, outs=None, accumulate=0, gb2=True):
    outs = outs or grads_out(d)
    rc = G.lib.gss_wgrad_reduce(d, slabs.ptr, slabs.total, nslices, outs["W1"].ptr, outs["W2"].ptr, outs["b1"].ptr, outs["b2"].ptr if gb2 else None,
                                accumulate, G.st())
    return rc, outs


def check_grads(g, want, exact, what):
    """g: host arrays by name; want: (gW1, gW2, gb).  b1 and b2 receive the same gradient"""
    assert np.array_equal(bits(g["b1"]), bits(g["b2"])), f"{what}: gb2 is not gb"
    for k, ref in (("W1", want[0]), ("W2", want[1]), ("b1", want[2])):
        written(g[k], f"{what} g{k}")
        if exact:
            assert np.array_equal(g[k], ref), f"{what}: g{k} is not the exact integer sum ({int((g[k] != ref).sum())} entries differ)"
        else:
            close(g[k], ref, PLAIN, np.abs(ref).max(), f"{what} g{k}")


def host_grads(outs):
    return {k: v.host("g" + k) for k, v in outs.items()}


@pytest.mark.parametrize("n,d,gathered", [(300, 64, False), (100, 128, True), (300, 256, False), (100, 48, True), (300, 16, False)])
def test_partial_writes_its_slices_and_nothing_else(G, n, d, gathered):
    c = K.wgrad("int", 300, n, d, gathered)
    D = on_device(c)
    ns = slices(G, n, d)
    slabs = Slabs(ns + 2, d)
    rc, got = partial(G, c, D, slabs, 1)
    G._lib.check(rc)
    assert got == ns
    w, b = slabs.host()
    for k in (0, ns + 1):
        assert prefilled(w[k]).all() and prefilled(b[k]).all(), f"slice {k} outside [1, {1 + ns}) was written"
    written(w[1:-1], "the weight slabs"), written(b[1:-1], "the bias slabs")
    gw1, gw2, gb = K.exact([K.problem(c)])
    # integers: the slabs' sum in any order is the exact gradient, [gW1 | gW2] side by side
    assert np.array_equal(w[1:-1].sum(0)[:, :d], gw1) and np.array_equal(w[1:-1].sum(0)[:, d:], gw2) and np.array_equal(b[1:-1].sum(0), gb)
    # the reduce reads slices [0, nslices) of the buffer: the same problem at slice 0 of a buffer of its own
    own = Slabs(ns, d)
    G._lib.check(partial(G, c, D, own, 0)[0])
    rc, outs = reduce(G, d, own, ns)
    G._lib.check(rc)
    check_grads(host_grads(outs), (gw1, gw2, gb), True, f"n={n} d={d}")


def reduce_tail(G, d, k):
    n = 32 * k
    c = K.wgrad("int", n, n, d, False)
    D = on_device(c)
    slabs = Slabs(k, d)
    rc, ns = partial(G, c, D, slabs, 0)
    G._lib.check(rc)
    assert ns == k == slices(G, n, d), "32 rows per slice"
    rc, outs = reduce(G, d, slabs, k)
    G._lib.check(rc)
    check_grads(host_grads(outs), K.exact([K.problem(c)]), True, f"d={d} k={k}")
    rc, outs = reduce(G, d, slabs, k, gb2=False)                 # gb2 is nullable
    G._lib.check(rc)
    assert outs["b2"].untouched() and np.array_equal(outs["b1"].host(), K.exact([K.problem(c)])[2])


@pytest.mark.parametrize("k", K.REDUCE_K)
def test_reduce_sums_every_slice_once(G, k):
    """every tail of wgrad_reduce_kernel's summation loops (64, 32, 16 and 4 slices per trip), integers: exact"""
    reduce_tail(G, 64, k)


@pytest.mark.parametrize("k", K.REDUCE_K_SIMPLE)
@pytest.mark.parametrize("d", K.REDUCE_D_SIMPLE)
def test_reduce_sums_every_slice_once_simple_kernel(G, d, k):
    """the same behind wgrad_simple_kernel; d = 48 has 19 output tiles: wgrad_wgs = 19 k asks for k slices"""
    if d == 48:
        with knobs(G, wgrad_wgs=max(8, 19 * k)):
            reduce_tail(G, d, k)
    else:
        reduce_tail(G, d, k)


@pytest.mark.parametrize("regime", ["int", "unit"])
@pytest.mark.parametrize("d", K.PAIR_D + (48,))
def test_problems_share_a_buffer(G, d, regime):
    """problem A: n = 300 full rows; problem B: b = 100 gathered rows, dP compact.  gss_wgrad_partial_pair -- one launch at d = 64, 128, 256,
    its two-launch fallback at d = 48 -- against two gss_wgrad_partial calls: equal bits; the reduce over both problems' slices"""
    a, b = K.wgrad(regime, K.PAIR_NA, K.PAIR_NA, d, False), K.wgrad(regime, K.PAIR_NA, K.PAIR_NB, d, True)
    Da, Db = on_device(a), on_device(b)
    ns_a, ns_b = slices(G, a["n"], d), slices(G, b["n"], d)
    total = ns_a + ns_b
    want = K.exact([K.problem(a), K.problem(b)]) if regime == "int" else M.wgrad([K.problem(a), K.problem(b)])
    for s_a, s_b in ((0, ns_a), (ns_b, 0)):          # A first, as the issue lays them out; B first, as a plan's step does
        what = f"{regime} d={d} A at {s_a}, B at {s_b}"
        one, two = Slabs(total, d), Slabs(total, d)
        rc, got_a, got_b = pair(G, d, a, Da, s_a, b, Db, s_b, one)
        G._lib.check(rc, what)
        assert (got_a, got_b) == (ns_a, ns_b)
        rc, got = partial(G, a, Da, two, s_a)
        G._lib.check(rc, what)
        rc, got = partial(G, b, Db, two, s_b)
        G._lib.check(rc, what)
        for x, y in zip(one.host(), two.host()):
            written(x, what)
            assert np.array_equal(bits(x), bits(y)), f"{what}: one launch and two differ"
        rc, g1 = reduce(G, d, one, total)
        G._lib.check(rc, what)
        rc, g2 = reduce(G, d, two, total)
        G._lib.check(rc, what)
        g1, g2 = host_grads(g1), host_grads(g2)
        assert all(np.array_equal(bits(g1[k]), bits(g2[k])) for k in NAMES)
        check_grads(g1, want, regime == "int", what)


@pytest.mark.parametrize("d", [64, 48])
def test_pair_with_an_empty_problem_and_accumulate(G, d):
    a, b = K.wgrad("int", K.PAIR_NA, K.PAIR_NA, d, False), K.wgrad("int", K.PAIR_NA, K.PAIR_NB, d, True)
    Da, Db = on_device(a), on_device(b)
    ns_a = slices(G, a["n"], d)
    assert slices(G, 0, d) == 1
    # n1 = 0 through the pair's fallback: the empty problem's slice reads as zero
    slabs = Slabs(ns_a + 1, d)
    rc, got_a, got_b = pair(G, d, a, Da, 0, b, Db, ns_a, slabs, n1=0)
    G._lib.check(rc)
    assert (got_a, got_b) == (ns_a, 1)
    w, bb = slabs.host()
    assert not w[ns_a].any() and not bb[ns_a].any() and not prefilled(w[ns_a]).any()
    want = K.exact([K.problem(a)])
    rc, outs = reduce(G, d, slabs, ns_a + 1)
    G._lib.check(rc)
    check_grads(host_grads(outs), want, True, f"d={d}, n1 = 0")
    # accumulate = 1 adds the sum to what the outputs hold: twice the gradient, exactly
    rc, outs = reduce(G, d, slabs, ns_a + 1, outs=outs, accumulate=1)
    G._lib.check(rc)
    check_grads(host_grads(outs), tuple(2 * v for v in want), True, f"d={d}, accumulate")
    # n = 0 alone: one slice of zeros, a gradient of zeros
    alone = Slabs(1, d)
    rc, ns = partial(G, a, Da, alone, 0, n=0)
    G._lib.check(rc)
    assert ns == 1
    rc, outs = reduce(G, d, alone, 1)
    G._lib.check(rc)
    assert all(not written(v, k).any() for k, v in host_grads(outs).items())


def test_wgrad_refusals(G):
    """slice0 + ns > total_slices and nslices > total_slices: GSS_EINVAL by name, nothing launched"""
    d = 64
    a, b = K.wgrad("int", K.PAIR_NA, K.PAIR_NA, d, False), K.wgrad("int", K.PAIR_NA, K.PAIR_NB, d, True)
    Da, Db = on_device(a), on_device(b)
    ns_a, ns_b = slices(G, a["n"], d), slices(G, b["n"], d)
    slabs = Slabs(ns_a + ns_b, d)
    rc, got = partial(G, a, Da, slabs, ns_b + 1)
    assert rc == EINVAL and got == -1 and "wgrad_partial: slices" in last_error(G), last_error(G)
    rc, got = partial(G, a, Da, slabs, -1)
    assert rc == EINVAL and "wgrad_partial: slices" in last_error(G), last_error(G)
    rc, got_a, got_b = pair(G, d, a, Da, 0, b, Db, ns_a + 1, slabs)
    assert rc == EINVAL and (got_a, got_b) == (-1, -1) and "wgrad_partial_pair: slices exceed" in last_error(G), last_error(G)
    rc, outs = reduce(G, d, slabs, ns_a + ns_b + 1)
    assert rc == EINVAL and "wgrad_reduce: bad argument" in last_error(G), last_error(G)
    torch.cuda.synchronize()
    assert slabs.out.untouched() and all(v.untouched() for v in outs.values()), "a refused call wrote"
    # the same arguments, unrefused, run
    assert partial(G, a, Da, slabs, ns_b) == (0, ns_a) and pair(G, d, a, Da, 0, b, Db, ns_a, slabs) == (0, ns_a, ns_b)
    assert reduce(G, d, slabs, ns_a + ns_b)[0] == 0
    torch.cuda.synchronize()


# ================================================================ the optimizer step
class AdamSet:
    """parameters, moments, gradients and transposed copies of one optimizer, all guarded, and the fp32 reference that follows it"""

    def __init__(self, d):
        params, state = K.adam_start(d)
        self.d = d
        self.p = {k: filled(params[k]) for k in NAMES}
        self.m = {k: filled(state["m_" + k]) for k in NAMES}
        self.v = {k: filled(state["v_" + k]) for k in NAMES}
        self.g = grads_out(d)
        self.wt = dict(W1=Out(d, d), W2=Out(d, d))
        self.ref_p, self.ref_state = {k: v.copy() for k, v in params.items()}, {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in state.items()}

    @staticmethod
    def four(outs):
        return (C.c_void_p * 4)(*[outs[k].ptr for k in NAMES])

    def before(self):
        """the reference starts every step from the parameters and moments the launch is about to read: the bound is one launch's (1-2 ulp,
        as test_adam_matches_torch_semantics says).  A reference that ran five steps on its own would also count the ulp by which two
        correct fp32 evaluations of v * beta2 + (1 - beta2) g^2 part ways at every step (one rounding with an FMA, two without): measured
        on an MI355X at d = 128, v of the fused form against such a reference: 0.7, 0.6, 1.3, 1.9, 2.5e-7 of the largest entry over the
        five steps, against 0.6e-7 at every step for the unfused form -- a drift of the comparison, not an error of a launch"""
        for k in NAMES:
            self.ref_p[k] = self.p[k].host("param").copy()
            self.ref_state["m_" + k], self.ref_state["v_" + k] = self.m[k].host("m").copy(), self.v[k].host("v").copy()

    def check(self, want, what):
        """the gradients against the fp64 mirror; then Adam from THOSE gradients (the parameter bound of test_adam_matches_torch_semantics holds
        for the update, whatever rounding the gradient carries); m and v relative to their own largest entry; the transposed copies"""
        g = host_grads(self.g)
        check_grads(g, want, False, what)
        M.adam(self.ref_p, g, self.ref_state, K.ADAM_LR, BETA1, BETA2, ADAM_EPS)
        for k in NAMES:
            p, m, v = self.p[k].host("param"), self.m[k].host("m"), self.v[k].host("v")
            err = np.abs(p - self.ref_p[k]).max() / max(1.0, np.abs(self.ref_p[k]).max())
            em = np.abs(m - self.ref_state["m_" + k]).max() / np.abs(self.ref_state["m_" + k]).max()
            ev = np.abs(v - self.ref_state["v_" + k]).max() / np.abs(self.ref_state["v_" + k]).max()
            print(f"{what} {k}: param err {err:.3e}, m {em:.3e}, v {ev:.3e} (bound {T.DENSE_STEP_ADAM:.1e})")
            assert err <= T.DENSE_STEP_ADAM and em <= T.DENSE_STEP_ADAM and ev <= T.DENSE_STEP_ADAM, f"{what} {k}"
        for k in ("W1", "W2"):
            assert np.array_equal(bits(self.wt[k].host("wt")), bits(self.p[k].host().T)), f"{what}: {k}'s transposed copy"


def check_reset(pos, idx, what):
    want = np.full(K.POS_N, POS_FREE, np.int32)
    if idx is not None:
        want[idx[idx >= 0]] = -1
    assert np.array_equal(pos.host("the position map"), want), f"{what}: exactly the members' entries are -1"


@pytest.mark.parametrize("d", K.ADAM_D)
def test_reduce_adam_and_the_unfused_form(G, d):
    """five steps of gss_wgrad_reduce_adam, and of gss_wgrad_reduce + gss_adam_step4 from the same start, over the slices of two problems;
    the position-map reset with b = 1 (d = 48), b = 2,500 beyond the reduce's own grid (d = 16) and b = 100"""
    fused, plain = AdamSet(d), AdamSet(d)
    start = {k: fused.p[k].host().copy() for k in NAMES}
    idx = K.adam_idx(d)
    idx_d = cu(idx)
    counts = (C.c_int64 * 4)(d * d, d, d * d, d)
    for step in range(1, K.ADAM_STEPS + 1):
        a, b = K.adam_step_problems(d, step)
        Da, Db = on_device(a), on_device(b)
        ns_a, ns_b = slices(G, a["n"], d), slices(G, b["n"], d)
        slabs = Slabs(ns_a + ns_b, d)
        rc, _, _ = pair(G, d, a, Da, 0, b, Db, ns_a, slabs)
        G._lib.check(rc)
        want = M.wgrad([K.problem(a), K.problem(b)])
        # steps 1, 2: the reset; step 3: ids without a map; from step 4 on neither
        reset = step <= 2
        ids, nb = (idx_d, len(idx)) if step <= 3 else (None, 0)
        pos_f = Out(K.POS_N, fill=POS_FREE, dtype=torch.int32)
        pos_p = Out(K.POS_N, fill=POS_FREE, dtype=torch.int32)
        fused.before(), plain.before()
        G._lib.check(G.lib.gss_wgrad_reduce_adam(d, slabs.ptr, slabs.total, slabs.total, fused.four(fused.g), fused.four(fused.p), fused.four(fused.m),
                                                 fused.four(fused.v), step, K.ADAM_LR, BETA1, BETA2, ADAM_EPS, fused.wt["W1"].ptr, fused.wt["W2"].ptr,
                                                 pos_f.ptr if reset else None, ptr(ids), nb, G.st()), "gss_wgrad_reduce_adam")
        rc, _ = reduce(G, d, slabs, slabs.total, outs=plain.g)
        G._lib.check(rc)
        G._lib.check(G.lib.gss_adam_step4(plain.four(plain.p), plain.four(plain.g), plain.four(plain.m), plain.four(plain.v), counts, step, K.ADAM_LR,
                                          BETA1, BETA2, ADAM_EPS, plain.wt["W1"].ptr, plain.wt["W2"].ptr, d, pos_p.ptr if reset else None, ptr(ids), nb,
                                          G.st()), "gss_adam_step4")
        fused.check(want, f"d={d} step {step} fused")
        plain.check(want, f"d={d} step {step} unfused")
        check_reset(pos_f, idx if reset else None, "fused")
        check_reset(pos_p, idx if reset else None, "unfused")
        same = all(np.array_equal(bits(fused.p[k].host()), bits(plain.p[k].host())) for k in NAMES)
        print(f"d={d} step {step}: the fused and the unfused form agree bit for bit: {same}")
        if step == 1:    # one gradient, two states: b1 and b2 move differently
            g = host_grads(fused.g)
            assert np.array_equal(bits(g["b1"]), bits(g["b2"]))
            assert not np.array_equal(fused.p["b1"].host() - start["b1"], fused.p["b2"].host() - start["b2"])


@pytest.mark.parametrize("dim", K.TRANSPOSE_DIMS)
def test_transpose2(G, dim):
    rng = np.random.RandomState(dim)
    a, b = rng.randn(dim, dim).astype(np.float32), rng.randn(dim, dim).astype(np.float32)
    at, bt = Out(dim, dim), Out(dim, dim)
    a_d, b_d = cu(a), cu(b)
    G._lib.check(G.lib.gss_transpose2(dim, ptr(a_d), ptr(b_d), at.ptr, bt.ptr, G.st()))
    assert np.array_equal(bits(at.host("at")), bits(a.T)) and np.array_equal(bits(bt.host("bt")), bits(b.T))
