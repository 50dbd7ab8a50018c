"""-m gpu: the dense backward hops of csrc/spmm.hip, op by op, against their fp64 contract (tests/sparse_hop_mirror.py: bwd1_dense,
bwd2_dense): SPMM_BWD1 (gss_spmm_bwd1, gss_spmm_bwd1_ex) and SPMM_BWD2 (gss_spmm_bwd2, gss_spmm_bwd2_ex) with dense operands at every
lane-group class of launch_balanced (d = 16 ... 1024), in both SpMM variants, as the second pass of a two-pass product with y_in
aliasing the output (what a shard's overlapped hop launches), under an own-row limit (the in-place transposed shard), chunked into
giant rows (spmm_giant = 64) and cut into feature slices.

What every value check asserts is the mirror's derived bound, per element: |got - ref| <= (k + 4) 2^-24 S, k the row's stored entries
(+ 1 for the first pass's sum) and S the mode's expression over absolute values -- checked for these very inputs on the CPU in
test_dense_hop_mirror.py; no measured tolerance.  Every output is pre-filled with a NaN of a known payload and every row must be
written in full.  No test provokes a fault: every launch that runs gets valid arguments (operands that end at an own-row limit sit in
front of larger buffers), the refusals are refused before any launch.

Largest error / bound ratios observed on the MI355X over all tests of this file (GSS_RECORD_PARITY; 1.0 would be the bound itself):
u 0.36, t 0.40, gx 0.37, dp 0.73 -- dp's on rows of few entries under c = 0.3, where the epilogue's four roundings and expf's own
error are most of the allowance; with c = 1.0 (an exact scale) dp stays below 0.56.  One-pass, row-per-wave, second-pass, limit and
sliced launches all lie in the same range (0.21 ... 0.73)."""
import contextlib
import functools

import numpy as np
import pytest

import dense_hop_cases as D
import sparse_hop_cases as K
import sparse_hop_mirror as M
from conftest import record_measured
from gpu_hop_common import G, assert_rows, cu, dev_csr, fully_written, host, knobs, prefilled, ptr, torch, untouched  # noqa: F401 (G: the fixture)

pytestmark = pytest.mark.gpu

GIANT = 64      # spmm_giant for the chunked runs: rows above 64 entries are summed chunk by chunk in three launches


@contextlib.contextmanager
def measured(name):
    """collects the worst error / bound ratio per output; printed and recorded whether or not an assertion of the body fails"""
    worst = {}
    try:
        yield worst
    finally:
        print(f"dense_hops.{name}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
        record_measured("dense_hops." + name, **worst)


def check(worst, key, got, ref, s, k, what):
    """every row written in full and inside the bound; the worst error / bound ratio goes to worst[key] before anything is asserted"""
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - np.asarray(ref, np.float64))
        r = np.where(err == 0, 0.0, err / M.bound(k, s))
    r = np.nan_to_num(r, nan=np.inf)   # (an element that still holds the pre-fill)
    worst[key] = max(worst.get(key, 0.0), float(r.max()))
    assert_rows(got, ref, s, k, np.ones(len(k), bool), what)


def same_bits(a, b):
    return np.array_equal(a.view(np.int32), b.view(np.int32))


def giant_knob(kind):
    return GIANT if kind == "giant" else 32768


def csr_of(G, g):
    return dev_csr(G, g.a, ("dense", g.kind))


def halves(G, g):
    """the entries split by column at n_cols // 3 (a shard's own-column / halo-column halves), as device CSRs"""
    first, second = K.split_by_column(g.a, g.n_cols // 3)
    one_sided = (np.diff(first.indptr) == 0) | (np.diff(second.indptr) == 0)
    return dev_csr(G, first, ("dense", g.kind, "first")), dev_csr(G, second, ("dense", g.kind, "second")), one_sided


# ================================================================ SPMM_BWD1
@functools.lru_cache(maxsize=None)
def bwd1_ref(kind, d):
    cs = D.bwd1_case(kind, d)
    return M.bwd1_dense(cs.g.a, cs.g_am, cs.g_ax, cs.x_in, cs.ax)


def bwd1_dev(cs):
    if not hasattr(cs, "dev"):
        cs.dev = {k: cu(getattr(cs, k)) for k in ("g_am", "g_ax", "x_in", "ax")}
    return cs.dev


def bwd1_args(cs, csr, u, t, y_in):
    dv = bwd1_dev(cs)
    return [csr.handle, cs.d, ptr(dv["g_am"]), ptr(dv["g_ax"]), ptr(dv["x_in"]), ptr(dv["ax"]), ptr(u), ptr(t), ptr(y_in)]


def run_bwd1(G, cs, csr, y_in=None, t=None, entry="ex"):
    """t: the buffer the pass writes t to (pre-filled when not given); y_in may be that buffer"""
    n = cs.g.n_rows
    u = prefilled(n, cs.d)
    t = prefilled(n, cs.d) if t is None else t
    if entry == "ex":
        G._lib.check(G.lib.gss_spmm_bwd1_ex(*bwd1_args(cs, csr, u, t, y_in), G.st()))
    else:
        assert y_in is None
        G._lib.check(G.lib.gss_spmm_bwd1(*bwd1_args(cs, csr, u, t, None)[:-1], G.st()))
    return host(u), host(t)


def check_bwd1(worst, out, ref, what, extra_k=0):
    check(worst, "u", out[0], ref.u, ref.s_u, ref.k + extra_k, what + " u")
    check(worst, "t", out[1], ref.t, ref.s_t, ref.k + extra_k, what + " t")


@pytest.mark.parametrize("kind,d", D.BWD1_CASES)
def test_bwd1_one_pass(G, kind, d):
    """gss_spmm_bwd1_ex without y_in: the bound on every element of u and t (an empty row: u = g_ax, t = 0), the bits of the
    9-argument gss_spmm_bwd1, the same bits twice; the giant graph whole and chunked (spmm_giant = 64)"""
    cs, ref = D.bwd1_case(kind, d), bwd1_ref(kind, d)
    g = cs.g
    csr = csr_of(G, g)
    with measured(f"bwd1_one_pass[{kind}-{d}]") as worst:
        for giant in sorted({32768, giant_knob(kind)}):
            with knobs(G, spmm_giant=giant):
                out = run_bwd1(G, cs, csr)
                again = run_bwd1(G, cs, csr)
                old = run_bwd1(G, cs, csr, entry="9-argument")
            check_bwd1(worst, out, ref, f"spmm_giant={giant}")
            for e in g.empty:
                assert same_bits(out[0][e], cs.g_ax[e]) and not out[1][e].any()
            assert same_bits(out[0], again[0]) and same_bits(out[1], again[1]), "two runs differ"
            assert same_bits(out[0], old[0]) and same_bits(out[1], old[1]), "gss_spmm_bwd1_ex differs from gss_spmm_bwd1"


# ================================================================ SPMM_BWD2
@functools.lru_cache(maxsize=None)
def bwd2_ref(kind, d, c, limit, with_res):
    cs = D.bwd2_case(kind, d, limit)
    return M.bwd2_dense(cs.g.a, cs.u, cs.t, cs.p, c, res=cs.res if with_res else None, own_row_limit=limit)


def bwd2_dev(cs):
    """limit > 0: t and res ARE `limit` rows long; they sit at the front of buffers of n_rows rows whose tail holds values of 100-200,
    so that a kernel that read them behind the limit would stay inside an allocation and show a wrong value"""
    if not hasattr(cs, "dev"):
        cs.dev = {k: cu(getattr(cs, k)) for k in ("u", "p")}
        rng = np.random.RandomState(cs.limit + cs.d)
        tail = cs.g.n_rows - cs.t.shape[0]
        for k in ("t", "res"):
            cs.dev[k] = cu(np.concatenate([getattr(cs, k), 100 + 100 * rng.rand(tail, cs.d).astype(np.float32)]))
    return cs.dev


def bwd2_args(cs, csr, c, res, dp, gx, y_in, limit):
    dv = bwd2_dev(cs)
    return [csr.handle, cs.d, ptr(dv["u"]), ptr(dv["t"]), ptr(dv["p"]), c, ptr(dv["res"]) if res else None, ptr(dp), ptr(gx), ptr(y_in), limit]


def run_bwd2(G, cs, csr, c, res=True, want_gx=True, y_in=None, dp=None, entry="ex"):
    """dp: the buffer the pass writes dp to (pre-filled when not given); y_in may be that buffer"""
    n = cs.g.n_rows
    dp = prefilled(n, cs.d) if dp is None else dp
    gx = prefilled(n, cs.d) if want_gx else None
    if entry == "ex":
        G._lib.check(G.lib.gss_spmm_bwd2_ex(*bwd2_args(cs, csr, c, res, dp, gx, y_in, cs.limit), G.st()))
    else:
        assert y_in is None and cs.limit == 0
        G._lib.check(G.lib.gss_spmm_bwd2(*bwd2_args(cs, csr, c, res, dp, gx, None, 0)[:-2], G.st()))
    return host(dp), (host(gx) if want_gx else None)


def check_bwd2(worst, out, ref, what, extra_k=0):
    check(worst, "dp", out[0], ref.dp, ref.s_dp, ref.k + extra_k, what + " dp")
    if out[1] is not None:
        check(worst, "gx", out[1], ref.gx, ref.s_gx, ref.k + extra_k, what + " gx")


@pytest.mark.parametrize("kind,d,c", D.BWD2_CASES)
def test_bwd2_one_pass(G, kind, d, c):
    """gss_spmm_bwd2_ex without y_in and limit: the bound on every element of dp and gx with and without the residual (an empty row:
    gx = t), the bits of the 10-argument gss_spmm_bwd2, the same bits twice; gx_out = NULL changes no bit of dp, res = NULL none of gx;
    the planted pre-activations (+0, -0, the smallest normal: elu' = 1; -20) sit in rows the bound covers like any other"""
    cs = D.bwd2_case(kind, d)
    g = cs.g
    csr = csr_of(G, g)
    with measured(f"bwd2_one_pass[{kind}-{d}-{c}]") as worst:
        for giant in sorted({32768, giant_knob(kind)}):
            with knobs(G, spmm_giant=giant):
                out = run_bwd2(G, cs, csr, c)
                again = run_bwd2(G, cs, csr, c)
                old = run_bwd2(G, cs, csr, c, entry="10-argument")
                nores = run_bwd2(G, cs, csr, c, res=False)
                old_nores = run_bwd2(G, cs, csr, c, res=False, entry="10-argument")
                nogx = run_bwd2(G, cs, csr, c, want_gx=False)
                neither = run_bwd2(G, cs, csr, c, res=False, want_gx=False)
            check_bwd2(worst, out, bwd2_ref(kind, d, c, 0, True), f"spmm_giant={giant}")
            check_bwd2(worst, nores, bwd2_ref(kind, d, c, 0, False), f"spmm_giant={giant}, no residual")
            for e in g.empty:
                assert same_bits(out[1][e], cs.t[e])
            assert same_bits(out[0], again[0]) and same_bits(out[1], again[1]), "two runs differ"
            assert same_bits(out[0], old[0]) and same_bits(out[1], old[1]), "gss_spmm_bwd2_ex differs from gss_spmm_bwd2"
            assert same_bits(nores[0], old_nores[0]) and same_bits(nores[1], old_nores[1]), "gss_spmm_bwd2_ex differs from gss_spmm_bwd2 (no residual)"
            assert same_bits(nores[1], out[1]), "res = NULL changed gx"
            assert same_bits(nogx[0], out[0]), "gx_out = NULL changed dp"
            assert same_bits(neither[0], nores[0]), "gx_out = NULL changed dp (no residual)"


# ================================================================ the row-per-wave variant
@pytest.mark.parametrize("mode,kind,d", [c for c in D.ONE_PASS if c[1] != "giant"])
def test_row_per_wave_variant_meets_the_same_bound(G, mode, kind, d):
    """spmm_variant = 1 (spmm_rows_kernel, and spmm_long_kernel for the rows above 512 entries) runs the same epilogues: the same
    cases against the same mirror and bound"""
    with measured(f"variant1[{mode}-{kind}-{d}]") as worst, knobs(G, spmm_variant=1):
        if mode == "bwd1":
            cs = D.bwd1_case(kind, d)
            assert (cs.g.lens > 512).any()
            check_bwd1(worst, run_bwd1(G, cs, csr_of(G, cs.g)), bwd1_ref(kind, d), "variant 1")
        else:
            cs = D.bwd2_case(kind, d)
            c = dict((k[:2], k[2]) for k in D.BWD2_CASES)[(kind, d)]
            assert (cs.g.lens > 512).any()
            check_bwd2(worst, run_bwd2(G, cs, csr_of(G, cs.g), c), bwd2_ref(kind, d, c, 0, True), "variant 1")
            nores = run_bwd2(G, cs, csr_of(G, cs.g), c, res=False, want_gx=False)
            check_bwd2(worst, nores, bwd2_ref(kind, d, c, 0, False), "variant 1, no residual, no gx")


# ================================================================ the second pass, in place
def first_pass(G, csr_first, d, x, out):
    """the plain product of the first half into the buffer the second pass writes: exactly what a plan's overlapped hop launches first"""
    G._lib.check(G.lib.gss_spmm(csr_first.handle, d, ptr(x), ptr(out), None, None, G.st()))


@pytest.mark.parametrize("mode,kind,d", D.TWO_PASS_CASES)
def test_second_pass_in_place(G, mode, kind, d):
    """The entries split by column at n_cols // 3.  First pass: gss_spmm of the first half into the buffer the second pass writes (t
    for bwd1, dp for bwd2); second pass: the second half with y_in = that buffer.  Within the one-pass mirror's bound with k + 1
    terms on every element; the bits of the one-pass kernel on the rows whose entries all lie in one half; and the bits of the same
    second pass with y_in in a buffer of its own.  The giant graph runs chunked (spmm_giant = 64): its finish pass must add y_in
    exactly once, its short pass on every other row"""
    g = D.graph(kind)
    csr = csr_of(G, g)
    first, second, one_sided = halves(G, g)
    assert one_sided.sum() > 50 and not one_sided[list(g.hubs)].any()
    with measured(f"second_pass[{mode}-{kind}-{d}]") as worst, knobs(G, spmm_giant=giant_knob(kind)):
        if mode == "bwd1":
            cs, ref = D.bwd1_case(kind, d), bwd1_ref(kind, d)
            x = bwd1_dev(cs)["g_am"]
            one = run_bwd1(G, cs, csr)
            buf = prefilled(g.n_rows, d)
            first_pass(G, first, d, x, buf)
            apart = buf.clone()
            two = run_bwd1(G, cs, second, y_in=buf, t=buf)
            sep = run_bwd1(G, cs, second, y_in=apart)
            check_bwd1(worst, two, ref, "two passes", extra_k=1)
        else:
            c = D.two_pass_c(d)
            cs, ref = D.bwd2_case(kind, d), bwd2_ref(kind, d, c, 0, True)
            x = bwd2_dev(cs)["u"]
            one = run_bwd2(G, cs, csr, c)
            buf = prefilled(g.n_rows, d)
            first_pass(G, first, d, x, buf)
            apart = buf.clone()
            two = run_bwd2(G, cs, second, c, y_in=buf, dp=buf)
            sep = run_bwd2(G, cs, second, c, y_in=apart)
            check_bwd2(worst, two, ref, "two passes", extra_k=1)
        assert fully_written(host(apart)).all(), "the first pass left a row unwritten"
        for k in (0, 1):
            assert same_bits(two[k], sep[k]), "y_in in place and y_in apart differ"
            assert np.array_equal(two[k][one_sided], one[k][one_sided]), \
                f"output {k}: a row with all its entries in one half differs from the one-pass kernel: rows {np.flatnonzero((two[k] != one[k]).any(1) & one_sided)[:8]}"


# ================================================================ the own-row limit
def behind_the_limit(cs, c, limit):
    """rows behind the limit, stated without the mirror: gx = A u, dp = c (A u) (.) elu'(p), from a scipy fp64 product"""
    au = (cs.g.a.astype(np.float64) @ cs.u.astype(np.float64))[limit:]
    return au, c * au * np.where(cs.p[limit:] > 0, 1.0, np.exp(np.minimum(cs.p[limit:], 0).astype(np.float64)))


@pytest.mark.parametrize("kind,d,c,limit", D.LIMIT_CASES)
def test_bwd2_rows_behind_the_own_row_limit_have_neither_t_nor_a_residual(G, kind, d, c, limit):
    """own_row_limit on the rectangular operand: t and res have exactly `limit` rows and what lies behind them in memory is 100-200
    (bwd2_dev), so a kernel that read them for a row behind the limit would show a wrong value.  With and without the residual, as one
    pass and as the second pass in place, whole and chunked (spmm_giant = 64: on rect_tail a giant row on each side of the limit)"""
    cs = D.bwd2_case(kind, d, limit)
    g = cs.g
    assert 0 < limit < g.n_rows and cs.t.shape[0] == limit and cs.res.shape[0] == limit
    csr = csr_of(G, g)
    first, second, _ = halves(G, g)
    au, want_dp = behind_the_limit(cs, c, limit)
    with measured(f"limit[{kind}-{d}-{c}-{limit}]") as worst:
        for giant in (32768, GIANT):
            for res in (True, False):
                ref = bwd2_ref(kind, d, c, limit, res)
                for two_pass in (False, True):
                    what = f"spmm_giant={giant} res={res} two_pass={two_pass}"
                    with knobs(G, spmm_giant=giant):
                        if two_pass:
                            buf = prefilled(g.n_rows, d)
                            first_pass(G, first, d, bwd2_dev(cs)["u"], buf)
                            out = run_bwd2(G, cs, second, c, res=res, y_in=buf, dp=buf)
                        else:
                            out = run_bwd2(G, cs, csr, c, res=res)
                    check_bwd2(worst, out, ref, what, extra_k=int(two_pass))
                    lim_k = ref.k + int(two_pass)
                    assert np.all(np.abs(out[1][limit:] - au) <= (M.bound(lim_k, ref.s_gx) + 1e-13 * ref.s_gx)[limit:]), what
                    assert np.all(np.abs(out[0][limit:] - want_dp) <= (M.bound(lim_k, ref.s_dp) + 1e-13 * ref.s_dp)[limit:]), what


# ================================================================ feature slices
@pytest.mark.parametrize("d,slices,pin", D.SLICE_CASES)
def test_feature_sliced_dense_backward_hops(G, d, slices, pin):
    """The balanced kernel cut into feature slices (knob spmm_slices; time-separated or pinned to XCDs): y_in, the epilogue's operands
    and the outputs are then addressed by slice.  Both modes as the second pass in place, SPMM_BWD2 under the own-row limit, against
    the same bound and write set; and the sliced one-pass launches too"""
    with measured(f"slices[{d}-{slices}-{pin}]") as worst, knobs(G, spmm_slices=slices, spmm_pin=pin):
        cs, ref = D.bwd1_case("hub", d), bwd1_ref("hub", d)
        first, second, _ = halves(G, cs.g)
        check_bwd1(worst, run_bwd1(G, cs, csr_of(G, cs.g)), ref, "bwd1 one pass")
        buf = prefilled(cs.g.n_rows, d)
        first_pass(G, first, d, bwd1_dev(cs)["g_am"], buf)
        check_bwd1(worst, run_bwd1(G, cs, second, y_in=buf, t=buf), ref, "bwd1 second pass", extra_k=1)
        c, limit = D.SLICE_C, D.SLICE_LIMIT
        cs = D.bwd2_case("rect_tail", d, limit)
        first, second, _ = halves(G, cs.g)
        au, want_dp = behind_the_limit(cs, c, limit)
        for res in (True, False):
            ref = bwd2_ref("rect_tail", d, c, limit, res)
            check_bwd2(worst, run_bwd2(G, cs, csr_of(G, cs.g), c, res=res), ref, f"bwd2 one pass, limit, res={res}")
            buf = prefilled(cs.g.n_rows, d)
            first_pass(G, first, d, bwd2_dev(cs)["u"], buf)
            out = run_bwd2(G, cs, second, c, res=res, y_in=buf, dp=buf)
            check_bwd2(worst, out, ref, f"bwd2 second pass, limit, res={res}", extra_k=1)
            assert np.all(np.abs(out[0][limit:] - want_dp) <= (M.bound(ref.k + 1, ref.s_dp) + 1e-13 * ref.s_dp)[limit:])
            assert np.all(np.abs(out[1][limit:] - au) <= (M.bound(ref.k + 1, ref.s_gx) + 1e-13 * ref.s_gx)[limit:])


# ================================================================ refusals
def test_refusals_name_the_function_and_launch_nothing(G):
    c1, c2 = D.bwd1_case("hub", 128), D.bwd2_case("rect_tail", 128, 600)
    csr1, csr2 = csr_of(G, c1.g), csr_of(G, c2.g)
    u, t = prefilled(c1.g.n_rows, 128), prefilled(c1.g.n_rows, 128)
    dp, gx = prefilled(c2.g.n_rows, 128), prefilled(c2.g.n_rows, 128)
    y1 = cu(np.zeros((c1.g.n_rows, 128), np.float32))
    y2 = cu(np.zeros((c2.g.n_rows, 128), np.float32))
    good1 = bwd1_args(c1, csr1, u, t, None) + [G.st()]
    good2 = bwd2_args(c2, csr2, 0.3, True, dp, gx, None, 0) + [G.st()]     # (limit 0: t and res are n_rows rows long in memory)

    def refused(fn, args, text):
        assert fn(*args) != 0
        assert text in G.lib.gss_last_error().decode(), G.lib.gss_last_error()

    def swap(args, i, v):
        return args[:i] + [v] + args[i + 1:]

    refused(G.lib.gss_spmm_bwd1_ex, swap(good1, 0, None), "gss_spmm_bwd1_ex")
    for i in (2, 3, 4, 5, 6, 7):
        refused(G.lib.gss_spmm_bwd1_ex, swap(good1, i, None), "spmm_bwd1")
    refused(G.lib.gss_spmm_bwd2_ex, swap(good2, 0, None), "gss_spmm_bwd2_ex")
    for i in (2, 3, 4, 7):
        refused(G.lib.gss_spmm_bwd2_ex, swap(good2, i, None), "spmm_bwd2")
    refused(G.lib.gss_spmm_bwd1_ex, swap(good1, 1, 20), "d=20")
    refused(G.lib.gss_spmm_bwd2_ex, swap(good2, 1, 20), "d=20")
    with knobs(G, spmm_variant=1):      # the row-per-wave SpMM has neither a second pass nor a row limit
        refused(G.lib.gss_spmm_bwd1_ex, swap(good1, 8, ptr(y1)), "spmm_bwd1: a two-pass product needs the balanced SpMM (spmm_variant 2)")
        refused(G.lib.gss_spmm_bwd2_ex, swap(good2, 9, ptr(y2)), "spmm_bwd2: a two-pass product needs the balanced SpMM (spmm_variant 2)")
        refused(G.lib.gss_spmm_bwd2_ex, swap(good2, 10, 600), "spmm_bwd2: a row limit needs the balanced SpMM (spmm_variant 2)")
    for x in (u, t, dp, gx):
        assert untouched(host(x)).all()       # nothing was launched
    # ... and the same arguments run once the knob is back
    G._lib.check(G.lib.gss_spmm_bwd1_ex(*swap(good1, 8, ptr(y1))))
    G._lib.check(G.lib.gss_spmm_bwd2_ex(*swap(swap(good2, 9, ptr(y2)), 10, 600)))
    for x in (u, t, dp, gx):
        assert fully_written(host(x)).all()
    with measured("after_refusals") as worst:
        check_bwd1(worst, (host(u), host(t)), bwd1_ref("hub", 128), "y_in = 0", extra_k=1)
        check_bwd2(worst, (host(dp), host(gx)), bwd2_ref("rect_tail", 128, 0.3, 600, True), "y_in = 0, limit", extra_k=1)
