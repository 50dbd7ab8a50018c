"""-m gpu: the input-gradient GEMM gss_dense_bwd_input (dense_bwd_input -> launch_gemm<EPI_SPLIT>, csrc/dense.hip) at every one of the 14
tile classes launch_gemm can pick for it -- whole lines x nt {2, 4, 8} x mt {1, 2} and the MFMA-layout epilogue x nt {1, 2, 4, 8} x mt
{1, 2} -- on both sides of every threshold, of a tile edge and of the three branches of xcd_ids.  Cases, references and the port of the
decision: tests/input_grad_cases.py, checked on the CPU by tests/test_input_grad_cases.py.

  int regime    bit equality with the integer product: exact in fp32 in any order, so a K chunk dropped or doubled, a column tile fed
                from the wrong weight half, a row staged from the clamp row or a tile computed in another's place is an exact mismatch.
  unit regime   per element |got - ref| <= 1.01 d 2^-24 (|dP| @ |W|) against fp64, rows of dP scaled by 2^-20 and 2^10 among the others.

Both outputs sit between canaries and start as a NaN of a known payload.  Without a list rows [0, n) are written in full and the
GUARD_ROWS rows behind them keep the pre-fill; with a list exactly the listed rows of BOTH g_ax and g_am are written, with the bits of
the pass without a list, and every other row of the 3 n keeps the pre-fill.  gemm_variant 2, 3 and 5 and a second run give the same
bits (the code's contract: "same MFMA order per output, same bits").  No test provokes a fault: every row list holds unique valid
rows, the refusals are refused on the host before any launch.

Largest error / bound ratio of the unit regime observed on the MI355X (GSS_RECORD_PARITY; 1.0 would be the bound): g_ax 0.16 (d = 16,
n = 17), g_am 0.20 (d = 16, n = 15).  By width, over both outputs and all n: d = 16 0.20, 32 0.13, 48 0.076, 64 0.086, 96 0.082, 128
0.052, 192 0.031, 256 0.024, 272 0.016, 288 0.020, 320 0.017, 384 0.018, 512 0.015, 1024 0.0056 -- the error grows like sqrt(d), the
bound like d.  The int regime, the write sets and every bit-equality claim (list against no list, gemm_variant 2 / 3 / 5, two runs)
held in all 14 classes; no class had to be excepted."""
import numpy as np
import pytest

import input_grad_cases as C
from conftest import record_measured
from guarded import PREFILL, Out, bits, cu, knobs, ptr

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


def launch(G, n, d, dp, w1t, w2t, rows, out_rows):
    """-> rc, g_ax, g_am as guarded, pre-filled [out_rows][d] buffers"""
    gax, gam = Out(out_rows, d), Out(out_rows, d)
    rc = G.lib.gss_dense_bwd_input(n, d, ptr(dp), ptr(w1t), ptr(w2t), ptr(rows), gax.ptr, gam.ptr, G.st())
    return rc, gax, gam


def run(G, D, n, d, listed, variant=2):
    """one launch under gemm_variant -> (g_ax, g_am) on the host, canaries checked"""
    with knobs(G, gemm_variant=variant):
        rc, gax, gam = launch(G, n, d, D["dp"], D["w1t"], D["w2t"], D["rows"] if listed else None, 3 * n if listed else n + C.GUARD_ROWS)
    G._lib.check(rc)
    return gax.host("g_ax"), gam.host("g_am")


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def prefilled(x):
    return bits(x) == np.int32(PREFILL)


def check_values(c, got, worst, what):
    """rows [0, n) of a pass without a list, in the case's regime"""
    n = c["n"]
    if c["regime"] == "int":
        for name, g, r in zip(("g_ax", "g_am"), got, C.exact(c["dp"], c["w1t"], c["w2t"])):
            bad = np.flatnonzero((bits(g[:n]) != bits(r)).any(1))
            assert not len(bad), f"{what} {name}: {len(bad)} rows differ from the integer product, first {bad[:8]}"
        return
    ref, lim = C.reference(c["dp"], c["w1t"], c["w2t"])
    for name, g, r, b in zip(("g_ax", "g_am"), got, ref, lim):
        assert not prefilled(g[:n]).any(), f"{what} {name}: a piece of rows [0, n) keeps the pre-fill"
        err = np.abs(g[:n].astype(np.float64) - r)
        ratio = np.nan_to_num(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300)), nan=np.inf)
        worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
        print(f"{what} {name}: error / bound {ratio.max():.3f}")
        assert (err <= b).all(), f"{what} {name}: {int((err > b).sum())} elements beyond 1.01 d 2^-24 (|dP| @ |W|), worst row {int(ratio.max(1).argmax())}"


@pytest.mark.parametrize("d,n", C.CASES)
def test_every_tile_class_without_and_with_a_row_list(G, d, n):
    worst = {}
    try:
        for regime in ("int", "unit"):
            c = C.case(regime, d, n)
            D = {k: cu(c[k]) for k in ("dp", "w1t", "w2t", "rows")}
            what = f"{regime} d={d} n={n} {C.tile_class(n, d, False)}"
            dense = {v: run(G, D, n, d, False, v) for v in C.VARIANTS}
            again = run(G, D, n, d, False)
            check_values(c, dense[2], worst, what)
            for g in dense[2]:
                assert prefilled(g[n:]).all(), f"{what}: a row behind n was written: {n + np.flatnonzero(~prefilled(g[n:]).all(1))[:8]}"
            for k, name in enumerate(("g_ax", "g_am")):
                assert same(dense[2][k], again[k]), f"{what} {name}: two runs differ"
                for v in (3, 5):
                    assert same(dense[2][k], dense[v][k]), f"{what} {name}: gemm_variant {v} {C.tile_class(n, d, False, v)} differs from 2"
            rows = c["rows"].astype(np.int64)
            other = np.ones(3 * n, bool)
            other[rows] = False
            for v in C.VARIANTS:
                scattered = run(G, D, n, d, True, v)
                for k, name in enumerate(("g_ax", "g_am")):
                    w = f"{what} {name}, a row list under gemm_variant {v} {C.tile_class(n, d, True, v)}"
                    assert prefilled(scattered[k][other]).all(), f"{w}: an unlisted row was written: {np.flatnonzero(other)[~prefilled(scattered[k][other]).all(1)][:8]}"
                    bad = np.flatnonzero((bits(scattered[k][rows]) != bits(dense[2][k][:n])).any(1))
                    assert not len(bad), f"{w}: {len(bad)} listed rows differ from the pass without a list, first tile rows {bad[:8]}"
    finally:
        if worst:
            record_measured(f"input_grad[{d}-{n}]", **worst)


@pytest.mark.parametrize("n", C.BIG_N)
def test_both_sides_of_the_row_threshold_of_mt(G, n):
    """d = 32 at 262143 and 262144 rows: <2, 1> and <2, 2> whole-line tiles, 4096 and 2048 node tiles; exact"""
    c = C.big_case(n)
    assert C.tile_class(n, 32, False) == (2, 1 if n < 262144 else 2, True)
    D = {k: cu(c[k]) for k in ("dp", "w1t", "w2t")}
    rc, gax, gam = launch(G, n, 32, D["dp"], D["w1t"], D["w2t"], None, n + C.GUARD_ROWS)
    G._lib.check(rc)
    for name, out in (("gax", gax), ("gam", gam)):
        g = out.host(name)
        bad = np.flatnonzero((bits(g[:n]) != bits(c[name])).any(1))
        assert not len(bad), f"n={n} {name}: {len(bad)} rows differ from the integer product, first {bad[:8]}"
        assert prefilled(g[n:]).all(), f"n={n} {name}: a row behind n was written"


def test_no_rows_is_no_launch_and_refusals_name_the_function(G):
    d, n = 32, 65
    c = C.case("int", d, n)
    D = {k: cu(c[k]) for k in ("dp", "w1t", "w2t", "rows")}
    outs = []
    for rows in (None, D["rows"]):
        rc, gax, gam = launch(G, 0, d, D["dp"], D["w1t"], D["w2t"], rows, 3 * n)
        assert rc == 0
        outs += [gax, gam]
    rc, gax, gam = launch(G, n, 20, D["dp"], D["w1t"], D["w2t"], None, 3 * n)
    assert rc != 0 and "d=20" in last_error(G), last_error(G)
    outs += [gax, gam]
    for rows in (None, D["rows"]):
        for null in ("dp", "w1t", "w2t"):
            rc, gax, gam = launch(G, n, d, *(None if k == null else D[k] for k in ("dp", "w1t", "w2t")), rows, 3 * n)
            assert rc != 0 and "dense_bwd_input: null operand" in last_error(G), (null, last_error(G))
            outs += [gax, gam]
        gax, gam = Out(3 * n, d), Out(3 * n, d)
        for a, b in ((None, gam.ptr), (gax.ptr, None)):
            rc = G.lib.gss_dense_bwd_input(n, d, ptr(D["dp"]), ptr(D["w1t"]), ptr(D["w2t"]), ptr(rows), a, b, G.st())
            assert rc != 0 and "dense_bwd_input: null operand" in last_error(G), last_error(G)
        outs += [gax, gam]
    rc, gax, gam = launch(G, -1, d, D["dp"], D["w1t"], D["w2t"], None, 3 * n)
    assert rc != 0 and "dense_bwd_input" in last_error(G), last_error(G)
    outs += [gax, gam]
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs), "a refused or empty call wrote an output"
