"""-m gpu: the per-op libgssgcn.so entry points of the training step against the numpy oracle / scipy on seeded inputs (called through
the C ABI with ctypes, device buffers held in torch tensors).  The row-sparse SpMM modes (gss_spmm_bwd1_sparse[_ex],
gss_spmm_bwd2_sparse_res, gss_spmm_filtered), their bitmap builders and gss_scatter_add_rows are in test_gpu_sparse_ops.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import golden_batches, golden_csr, golden_params, load_golden
from oracle import gss_oracle as O
from sparse_hop_cases import random_graph

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import gcn_drug_repurposing_amd as pkg
    from gcn_drug_repurposing_amd import _lib, graph
    lib = pkg.load()

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib, ns.graph = lib, _lib, graph
    ns.st = lambda: _lib.current_stream()
    return ns


def cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def rel_err(got, ref):
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


# ---------------------------------------------------------------- K11
def test_normalize_adj_matches_reference_fixture(G, op_case):
    name, g = op_case
    gg = G.graph.GssGraph(golden_csr(g, "A"))
    ref = golden_csr(g, "Ahat")
    assert np.array_equal(gg.a.h_indptr, ref.indptr)
    assert np.array_equal(gg.a.col.cpu().numpy(), ref.indices)
    got = gg.a.val.cpu().numpy()
    assert got.dtype == np.float32
    # fp64 pipeline then fp32 cast: equal to the reference's cast up to 1 ulp
    np.testing.assert_allclose(got, ref.data.astype(np.float32), rtol=1.2e-7, atol=0)
    np.testing.assert_allclose(gg.rowsum.cpu().numpy(), g["rowsum"], rtol=1e-13)
    # the transposed operand is the same matrix transposed
    t = gg.at.to_scipy()
    assert abs(t - gg.a.to_scipy().T).max() == 0


def test_non_positive_row_sum_is_counted_and_refused_and_reproduces_the_reference_nans(G):
    """helpers/helper.py:85 takes rowsum ** -0.5 of a negative row sum without a word.  gss_rowsum_check counts such rows;
    GssGraph refuses the graph naming the first of them; under allow_nan the device normalisation has NaN at exactly the entries the
    reference's preprocess_graph has them (fixture generated from the reference: one node that points away from all others) and its values elsewhere, and one hop spreads
    the NaN to exactly the rows the reference's sparse product spreads it to"""
    import warnings
    from conftest import load_golden
    g = load_golden("knn_negative_rowsum_n96_d8")
    n = g["X"].shape[0]
    bad = int(g["bad_rows"][0])
    adj = G.graph.knn_descriptor_adj_device(g["X"].astype(np.float64), int(g["k"]))          # the device kNN builder keeps negative similarities
    ref_a = sp.csr_matrix((g["A_data"], g["A_indices"], g["A_indptr"]), shape=(n, n))
    adj = sp.csr_matrix(adj); adj.sort_indices()
    assert np.array_equal(adj.indptr, ref_a.indptr) and np.array_equal(adj.indices, ref_a.indices)
    with pytest.raises(G.graph.NonPositiveRowSum, match=f"first: node {bad} = 'n{bad}'") as ei:
        G.graph.GssGraph(adj, name_of=lambda i: f"n{i}")
    assert ei.value.count == 1 and ei.value.first == bad and ei.value.n == n
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        gg = G.graph.GssGraph(adj, allow_nan=True)
    assert any("sum <= 0" in str(x.message) for x in w)
    assert (gg.bad_rows, gg.first_bad_row) == (1, bad)
    np.testing.assert_allclose(gg.rowsum.cpu().numpy(), g["rowsum"], rtol=1e-13)
    assert np.array_equal(gg.a.h_indptr, g["Ahat_indptr"]) and np.array_equal(gg.a.col.cpu().numpy(), g["Ahat_indices"])
    got = gg.a.val.cpu().numpy()
    nan_ref = ~np.isfinite(g["Ahat_data"])
    assert np.array_equal(~np.isfinite(got), nan_ref) and np.array_equal(np.isnan(got), np.isnan(g["Ahat_data"]))
    np.testing.assert_allclose(got[~nan_ref], g["Ahat_data"][~nan_ref].astype(np.float32), rtol=1.2e-7, atol=0)
    # one hop: rows that read the bad node's row of X through a NaN weight, i.e. the bad row and its neighbours (torch.sparse.mm, model.py:163)
    x = torch.from_numpy(g["X"]).cuda()
    xp = torch.zeros(n, 16, device="cuda"); xp[:, :8] = x
    y = torch.empty(n, 16, device="cuda")
    G._lib.check(G.lib.gss_spmm(gg.a.handle, 16, xp.data_ptr(), y.data_ptr(), None, None, G._lib.current_stream()))
    rows = np.repeat(np.arange(n), np.diff(g["Ahat_indptr"]))
    expect = np.zeros(n, bool); expect[rows[nan_ref]] = True
    torch.cuda.synchronize()
    assert np.array_equal((~np.isfinite(y[:, :8].cpu().numpy())).any(1), expect)
    # the raw entry point on healthy and empty inputs
    cnt, first = G.graph.rowsum_check(torch.ones(1000, dtype=torch.float64, device="cuda"), 1000)
    assert (cnt, first) == (0, -1)
    v = torch.ones(1000, dtype=torch.float64, device="cuda"); v[[7, 300, 999]] = torch.tensor([0.0, -1.0, float("nan")], dtype=torch.float64, device="cuda")
    assert G.graph.rowsum_check(v, 1000) == (3, 7)
    assert G.graph.rowsum_check(v, 0) == (0, -1)


def test_spmm_row_sums_within_1e5(G, op_case):
    """north_star: SpMM row sums within 1e-5 (fp32) of the host preprocess_graph result."""
    name, g = op_case
    gg = G.graph.GssGraph(golden_csr(g, "A"))
    n = gg.n
    ones = torch.ones(n, 16, device="cuda")
    y = torch.empty(n, 16, device="cuda")
    G._lib.check(G.lib.gss_spmm(gg.a.handle, 16, ones.data_ptr(), y.data_ptr(), None, None, G.st()))
    ref = np.asarray(golden_csr(g, "Ahat").sum(1)).reshape(-1)
    assert np.abs(y[:, 0].cpu().numpy() - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())


# ---------------------------------------------------------------- K1 / K2 / K9
@pytest.fixture(params=[1, 2, 22, 42, 122, 142])
def spmm_variant(request, G):
    """1 = row-per-wave, 2 = nnz-balanced (automatic slicing), 22 / 42 = nnz-balanced with 2 / 4 forced time-separated
    feature slices, 122 / 142 = the same slices pinned to XCDs"""
    v = request.param
    G._lib.check(G.lib.gss_debug_set_option(b"spmm_variant", min(v, 2) if v < 10 else 2))
    G._lib.check(G.lib.gss_debug_set_option(b"spmm_slices", (v % 100) // 10))
    G._lib.check(G.lib.gss_debug_set_option(b"spmm_pin", 1 if v >= 100 else 0))
    yield v
    G._lib.check(G.lib.gss_debug_set_option(b"spmm_variant", 2))
    G._lib.check(G.lib.gss_debug_set_option(b"spmm_slices", 0))
    G._lib.check(G.lib.gss_debug_set_option(b"spmm_pin", 0))


@pytest.mark.parametrize("d", [16, 48, 64, 128, 256, 512, 1024])
def test_spmm_all_widths_with_hub_and_empty_rows(G, d, spmm_variant):
    rng = np.random.RandomState(d)
    n = 1500
    a = random_graph(rng, n, 7, hub_rows=(3, 700), hub_deg=1200, empty_rows=(0, 11, n - 1))
    a32 = sp.csr_matrix((a.data.astype(np.float32), a.indices, a.indptr), shape=a.shape)
    csr = G.graph.DeviceCSR(a32.indptr, a32.indices, a32.data, n, n, "cuda")
    assert csr.h_indptr[4] - csr.h_indptr[3] > 512  # exercises the long-row kernel
    x = rng.randn(n, d).astype(np.float32)
    h = rng.randn(n, d).astype(np.float32)
    xd, hd = cu(x), cu(h)
    y = torch.full((n, d), float("nan"), device="cuda")
    m = torch.full((n, d), float("nan"), device="cuda")
    G._lib.check(G.lib.gss_spmm(csr.handle, d, xd.data_ptr(), y.data_ptr(), hd.data_ptr(), m.data_ptr(), G.st()))
    ref = a32.astype(np.float64) @ x.astype(np.float64)
    assert rel_err(y.cpu().numpy(), ref) < 2e-6
    assert rel_err(m.cpu().numpy(), ref * h) < 2e-6
    assert np.all(y.cpu().numpy()[[0, 11, n - 1]] == 0)
    y2 = torch.full((n, d), float("nan"), device="cuda")
    G._lib.check(G.lib.gss_spmm(csr.handle, d, xd.data_ptr(), y2.data_ptr(), None, None, G.st()))
    assert torch.equal(y, y2)  # bitwise reproducible, with and without the fused epilogue


@pytest.mark.parametrize("d", [16, 128, 256])
def test_spmm_add_second_pass_of_a_two_pass_product(G, d):
    """gss_spmm_add: the entries of every row split over two CSRs by column (a shard's own-column / boundary-column halves): the plain
    product of the first, then y = y_in + A2 x with the fused epilogue, in place, equals the one-pass product up to the changed
    summation order -- and bit for bit on rows whose entries all sit in one half"""
    rng = np.random.RandomState(100 + d)
    n, c0 = 1400, 500
    a = random_graph(rng, n, 9, hub_rows=(5, 900), hub_deg=1100, empty_rows=(2, n - 1))
    a32 = sp.csr_matrix((a.data.astype(np.float32), a.indices, a.indptr), shape=a.shape)
    coo = a32.tocoo()
    halves = []
    for mask in (coo.col < c0, coo.col >= c0):
        h = sp.csr_matrix((coo.data[mask], (coo.row[mask], coo.col[mask])), shape=a32.shape)
        h.sort_indices()
        halves.append(h)
    full = G.graph.DeviceCSR(a32.indptr, a32.indices, a32.data, n, n, "cuda")
    own = G.graph.DeviceCSR(halves[0].indptr, halves[0].indices, halves[0].data, n, n, "cuda")
    rest = G.graph.DeviceCSR(halves[1].indptr, halves[1].indices, halves[1].data, n, n, "cuda")
    x, hh = rng.randn(n, d).astype(np.float32), rng.randn(n, d).astype(np.float32)
    xd, hd = cu(x), cu(hh)
    y1, m1 = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
    G._lib.check(G.lib.gss_spmm(full.handle, d, xd.data_ptr(), y1.data_ptr(), hd.data_ptr(), m1.data_ptr(), G.st()))
    y2, m2 = torch.full((n, d), float("nan"), device="cuda"), torch.full((n, d), float("nan"), device="cuda")
    G._lib.check(G.lib.gss_spmm(own.handle, d, xd.data_ptr(), y2.data_ptr(), None, None, G.st()))
    G._lib.check(G.lib.gss_spmm_add(rest.handle, d, xd.data_ptr(), y2.data_ptr(), y2.data_ptr(), hd.data_ptr(), m2.data_ptr(), G.st()))
    ref = a32.astype(np.float64) @ x.astype(np.float64)
    assert rel_err(y2.cpu().numpy(), ref) < 2e-6 and rel_err(m2.cpu().numpy(), ref * hh) < 2e-6
    assert rel_err(y2.cpu().numpy(), y1.cpu().numpy()) < 1e-6
    one_sided = np.flatnonzero((np.diff(halves[0].indptr) == 0) | (np.diff(halves[1].indptr) == 0))
    assert len(one_sided) > 50
    sel = torch.from_numpy(one_sided).cuda()
    assert torch.equal(y1.index_select(0, sel), y2.index_select(0, sel)) and torch.equal(m1.index_select(0, sel), m2.index_select(0, sel))


@pytest.mark.parametrize("d", [64, 128, 256])
def test_spmm_hot_cold_split_and_deeper_queues_do_not_change_a_bit(G, d):
    """gss_csr_set_hot / the large-table kernel path (non-temporal gathers of the rows outside the hubs' set, 8 gathers in
    flight): cache policy and queue depth only -- the same bits as the default path, for every epilogue"""
    rng = np.random.RandomState(d + 1)
    n = 1300
    a = random_graph(rng, n, 9, hub_rows=(1, 400), hub_deg=900, empty_rows=(7,))
    a32 = sp.csr_matrix((a.data.astype(np.float32), a.indices, a.indptr), shape=a.shape)
    csr = G.graph.DeviceCSR(a32.indptr, a32.indices, a32.data, n, n, "cuda")
    x, h = cu(rng.randn(n, d).astype(np.float32)), cu(rng.randn(n, d).astype(np.float32))

    def run():
        y, m = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
        G._lib.check(G.lib.gss_spmm(csr.handle, d, x.data_ptr(), y.data_ptr(), h.data_ptr(), m.data_ptr(), G.st()))
        return y, m

    base = run()
    try:
        for hot in (n // 3, 5, 0, n // 2):
            G._lib.check(G.lib.gss_debug_set_option(b"spmm_hot_rows", hot))      # overrides the size threshold: forces the split path
            got = run()
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), hot
    finally:
        G._lib.check(G.lib.gss_debug_set_option(b"spmm_hot_rows", -1))
    # the per-CSR declaration (what shards.build_shard sets) is accepted and validated
    G._lib.check(G.lib.gss_csr_set_hot(csr.handle, 100, n, n))
    assert G.lib.gss_csr_set_hot(csr.handle, 100, n + 1, n) != 0
    assert torch.equal(run()[0], base[0])


@pytest.mark.parametrize("d", [16, 64, 128, 256])
def test_giant_rows_are_summed_chunk_by_chunk_across_workgroups(G, d):
    """Rows with more stored entries than knob spmm_giant (default 32,768; 64 here) are cut into chunks of a quarter of it: a chunk pass
    sums them into a scratch, the product proper runs over the other rows, and a finish pass adds a giant row's chunks in order and runs
    the caller's epilogue (spmm.hip GiantRows).  Every dense form -- plain, Hadamard-fused, both backward epilogues, the second pass of a
    two-pass product -- must equal the fp64 product to the usual tolerance and the unchunked kernel to rounding; rows below the
    threshold keep their bits; empty rows and a row that holds every column are covered."""
    rng = np.random.RandomState(3 * d + 1)
    n = 2100
    a = random_graph(rng, n, 7, hub_rows=(5, 900, 1500), hub_deg=1300, empty_rows=(2, n - 1))
    a = sp.lil_matrix(a)
    a[40, :] = rng.uniform(0.1, 1.0, n)                      # one row with every column: 33 chunks of 16
    a = sp.csr_matrix(a)
    a.sort_indices()
    a32 = sp.csr_matrix((a.data.astype(np.float32), a.indices, a.indptr), shape=a.shape)
    A = a32.astype(np.float64)
    lens = np.diff(a32.indptr)
    giant = np.flatnonzero(lens > 64)
    small = torch.from_numpy(np.flatnonzero(lens <= 64)).cuda()
    assert len(giant) >= 4 and lens.max() == n
    x, hh, gam, gax, xin, ax, pp, res = (rng.randn(n, d).astype(np.float32) for _ in range(8))
    xd, hd, gam_d, gax_d, xin_d, ax_d, p_d, res_d = (cu(v) for v in (x, hh, gam, gax, xin, ax, pp, res))

    def run(thr):
        G._lib.check(G.lib.gss_debug_set_option(b"spmm_giant", thr))
        try:
            csr = G.graph.DeviceCSR(a32.indptr, a32.indices, a32.data, n, n, "cuda")     # a handle looks at the knob with its first launch
            ng, nc = C.c_int32(-1), C.c_int32(-1)
            G._lib.check(G.lib.gss_csr_giant_rows(csr.handle, C.byref(ng), C.byref(nc)))
            assert (ng.value, nc.value) == ((len(giant), int(sum(-(-int(l) // 16) for l in lens[giant]))) if thr else (0, 0))
            out = {}
            y, m = torch.full((n, d), float("nan"), device="cuda"), torch.full((n, d), float("nan"), device="cuda")
            G._lib.check(G.lib.gss_spmm(csr.handle, d, xd.data_ptr(), y.data_ptr(), None, None, G.st()))
            out["plain"] = y.clone()
            G._lib.check(G.lib.gss_spmm(csr.handle, d, xd.data_ptr(), y.data_ptr(), hd.data_ptr(), m.data_ptr(), G.st()))
            out["fwd1_y"], out["fwd1_m"] = y.clone(), m.clone()
            u, t = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
            G._lib.check(G.lib.gss_spmm_bwd1(csr.handle, d, gam_d.data_ptr(), gax_d.data_ptr(), xin_d.data_ptr(), ax_d.data_ptr(), u.data_ptr(),
                                             t.data_ptr(), G.st()))
            out["u"], out["t"] = u.clone(), t.clone()
            dp, gx = torch.empty(n, d, device="cuda"), torch.empty(n, d, device="cuda")
            G._lib.check(G.lib.gss_spmm_bwd2(csr.handle, d, gam_d.data_ptr(), gax_d.data_ptr(), p_d.data_ptr(), 0.3, res_d.data_ptr(), dp.data_ptr(),
                                             gx.data_ptr(), G.st()))
            out["dp"], out["gx"] = dp.clone(), gx.clone()
            # second pass of a two-pass product: y_in + A x, then the Hadamard epilogue
            y2, m2 = out["plain"].clone(), torch.empty(n, d, device="cuda")
            G._lib.check(G.lib.gss_spmm_add(csr.handle, d, xd.data_ptr(), y2.data_ptr(), y2.data_ptr(), hd.data_ptr(), m2.data_ptr(), G.st()))
            out["add_y"], out["add_m"] = y2.clone(), m2.clone()
            torch.cuda.synchronize()
            return out
        finally:
            G._lib.check(G.lib.gss_debug_set_option(b"spmm_giant", 32768))

    whole, chunked = run(0), run(64)
    ax_ref = A @ x.astype(np.float64)
    dm = A @ gam.astype(np.float64)
    gref = gax.astype(np.float64) + A @ gam.astype(np.float64)          # bwd2 called with u := gam, t := gax
    refs = {"plain": ax_ref, "fwd1_y": ax_ref, "fwd1_m": ax_ref * hh, "u": gax + dm * xin, "t": dm * ax, "gx": gref,
            "dp": 0.3 * gref * np.where(pp > 0, 1.0, np.exp(np.minimum(pp, 0).astype(np.float64))) + res,
            "add_y": 2 * ax_ref, "add_m": 2 * ax_ref * hh}
    for k, ref in refs.items():
        assert rel_err(chunked[k].cpu().numpy(), ref) < 3e-6, k
        assert rel_err(chunked[k].cpu().numpy(), whole[k].cpu().numpy()) < 1e-6, k
        assert torch.equal(chunked[k].index_select(0, small), whole[k].index_select(0, small)), k      # rows below the threshold: same bits
    for r in (2, n - 1):                                                     # empty rows: zeros / the epilogue of a zero sum
        assert float(chunked["plain"][r].abs().max()) == 0.0


def test_spmm_backward_epilogues(G, spmm_variant):
    rng = np.random.RandomState(5)
    n, d = 900, 128
    a = random_graph(rng, n, 9, hub_rows=(5,), hub_deg=700)
    a32 = sp.csr_matrix((a.data.astype(np.float32), a.indices, a.indptr), shape=a.shape)
    csr = G.graph.DeviceCSR(a32.indptr, a32.indices, a32.data, n, n, "cuda")
    A = a32.astype(np.float64)
    gam, gax, xin, ax, p, res = (rng.randn(n, d).astype(np.float32) for _ in range(6))
    u = torch.empty(n, d, device="cuda")
    t = torch.empty(n, d, device="cuda")
    gam_d, gax_d, xin_d, ax_d, p_d, res_d = (cu(v) for v in (gam, gax, xin, ax, p, res))  # keep alive across the calls
    G._lib.check(G.lib.gss_spmm_bwd1(csr.handle, d, gam_d.data_ptr(), gax_d.data_ptr(), xin_d.data_ptr(),
                                     ax_d.data_ptr(), u.data_ptr(), t.data_ptr(), G.st()))
    dm = A @ gam.astype(np.float64)
    assert rel_err(u.cpu().numpy(), gax + dm * xin) < 2e-6
    assert rel_err(t.cpu().numpy(), dm * ax) < 2e-6
    uu, tt = u.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
    for use_res, want_gx in ((False, False), (True, True)):
        dp = torch.empty(n, d, device="cuda")
        gx = torch.empty(n, d, device="cuda")
        G._lib.check(G.lib.gss_spmm_bwd2(csr.handle, d, u.data_ptr(), t.data_ptr(), p_d.data_ptr(), 0.3,
                                         res_d.data_ptr() if use_res else None, dp.data_ptr(),
                                         gx.data_ptr() if want_gx else None, G.st()))
        gref = tt + A @ uu
        dref = 0.3 * gref * np.where(p > 0, 1.0, np.exp(np.minimum(p, 0).astype(np.float64)))
        if use_res:
            dref = dref + res
            assert rel_err(gx.cpu().numpy(), gref) < 2e-6
        assert rel_err(dp.cpu().numpy(), dref) < 2e-6


# ---------------------------------------------------------------- K3 / K4 / K8
@pytest.fixture(params=[2, 3, 5])
def gemm_variant(request, G):
    G._lib.check(G.lib.gss_debug_set_option(b"gemm_variant", request.param))
    yield request.param
    G._lib.check(G.lib.gss_debug_set_option(b"gemm_variant", 2))


@pytest.mark.parametrize("n,d", [(1000, 128), (77, 16), (300, 32), (513, 64), (200, 256), (130, 48), (129, 192)])
def test_dense_fwd(G, n, d, gemm_variant):
    rng = np.random.RandomState(n + d)
    ax, am, pprev = (rng.randn(n, d).astype(np.float32) for _ in range(3))
    w1, w2 = (np.eye(d, dtype=np.float32) + 0.1 * rng.randn(d, d).astype(np.float32) for _ in range(2))
    b1, b2 = (0.1 * rng.randn(d).astype(np.float32) for _ in range(2))
    ax_d, am_d, w1_d, b1_d, w2_d, b2_d, pp_d = (cu(v) for v in (ax, am, w1, b1, w2, b2, pprev))
    for prev in (None, pprev):
        p = torch.full((n, d), float("nan"), device="cuda")
        xn = torch.full((n, d), float("nan"), device="cuda")
        G._lib.check(G.lib.gss_dense_fwd(n, d, ax_d.data_ptr(), am_d.data_ptr(), w1_d.data_ptr(), b1_d.data_ptr(),
                                         w2_d.data_ptr(), b2_d.data_ptr(), pp_d.data_ptr() if prev is not None else None,
                                         0.3, p.data_ptr(), xn.data_ptr(), G.st()))
        pref = ax.astype(np.float64) @ w1.T.astype(np.float64) + b1 + am.astype(np.float64) @ w2.T.astype(np.float64) + b2
        o = np.where(pref > 0, pref, np.expm1(np.minimum(pref, 0)))
        xref = o if prev is None else prev + 0.3 * o
        assert rel_err(p.cpu().numpy(), pref) < 3e-6
        assert rel_err(xn.cpu().numpy(), xref) < 3e-6


@pytest.mark.parametrize("n", [1, 15, 16, 17, 1000, 8200, 29960, 140003])
def test_dense_fwd_weight_stationary_equals_the_staged_tiles(G, n):
    """Round 5: the d = 128 forward projection as a weight-stationary persistent kernel (proj_ws_kernel: a wave keeps its K x 32 slice
    of [W1 | W2] in registers, 16-row tiles of [AX | AM] stream through an LDS ring) accumulates every output chunk by chunk in the
    staged kernel's order: P and x_next must not differ by a bit -- for one tile and for thousands, ragged last tiles, more
    workgroups than tiles, few workgroups that walk hundreds of tiles, with and without the staggered start."""
    d = 128
    rng = np.random.RandomState(n)
    ax, am, pprev = (cu(rng.randn(n, d).astype(np.float32)) for _ in range(3))
    w1, w2 = (cu(np.eye(d, dtype=np.float32) + 0.1 * rng.randn(d, d).astype(np.float32)) for _ in range(2))
    b1, b2 = (cu(0.1 * rng.randn(d).astype(np.float32)) for _ in range(2))

    def run(prev, **knobs):
        try:
            for k, v in knobs.items():
                G._lib.check(G.lib.gss_debug_set_option(k.encode(), v))
            p = torch.full((n + 1, d), float("nan"), device="cuda")      # one guard row behind the outputs
            xn = torch.full((n + 1, d), float("nan"), device="cuda")
            G._lib.check(G.lib.gss_dense_fwd(n, d, ax.data_ptr(), am.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                             pprev.data_ptr() if prev else None, 0.3, p.data_ptr(), xn.data_ptr(), G.st()))
            torch.cuda.synchronize()
            assert bool(torch.isnan(p[n]).all()) and bool(torch.isnan(xn[n]).all()), "a row behind the outputs was written"
            return p[:n].clone(), xn[:n].clone()
        finally:
            G.lib.gss_debug_set_option(b"gemm_ws", -1)

    for prev in (False, True):
        ref = run(prev, gemm_ws=0)
        assert bool(torch.isfinite(ref[0]).all())
        got = run(prev, gemm_ws=1)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), (n, prev, "gemm_ws=1")
        got = run(prev)                     # the default: by row count (weight-stationary from 32,769 rows on)
        assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1]), (n, prev, "default")


@pytest.mark.parametrize("n,d", [(700, 128), (50, 16), (333, 64)])
def test_dense_bwd_input_dense_and_scattered(G, n, d, gemm_variant):
    rng = np.random.RandomState(n)
    dp = rng.randn(n, d).astype(np.float32)
    w1, w2 = (rng.randn(d, d).astype(np.float32) for _ in range(2))
    gax = torch.empty(n, d, device="cuda")
    gam = torch.empty(n, d, device="cuda")
    dp_d, w1t_d, w2t_d = cu(dp), cu(w1.T.copy()), cu(w2.T.copy())
    G._lib.check(G.lib.gss_dense_bwd_input(n, d, dp_d.data_ptr(), w1t_d.data_ptr(), w2t_d.data_ptr(), None,
                                           gax.data_ptr(), gam.data_ptr(), G.st()))
    assert rel_err(gax.cpu().numpy(), dp.astype(np.float64) @ w1) < 3e-6
    assert rel_err(gam.cpu().numpy(), dp.astype(np.float64) @ w2) < 3e-6
    big = 3 * n
    rows = rng.permutation(big)[:n].astype(np.int32)
    gax2 = torch.zeros(big, d, device="cuda")
    gam2 = torch.zeros(big, d, device="cuda")
    rows_d = cu(rows)
    G._lib.check(G.lib.gss_dense_bwd_input(n, d, dp_d.data_ptr(), w1t_d.data_ptr(), w2t_d.data_ptr(),
                                           rows_d.data_ptr(), gax2.data_ptr(), gam2.data_ptr(), G.st()))
    ref = np.zeros((big, d))
    ref[rows] = dp.astype(np.float64) @ w1
    assert rel_err(gax2.cpu().numpy(), ref) < 3e-6
    assert torch.equal(gax2[cu(rows).long()], gax)


@pytest.mark.parametrize("n,d", [(5000, 128), (100, 16), (2048, 64), (999, 256), (64, 32)])
def test_dense_bwd_weight(G, n, d):
    rng = np.random.RandomState(n + d)
    dp, ax, am = (rng.randn(n, d).astype(np.float32) for _ in range(3))
    ws = torch.empty(G.lib.gss_wgrad_workspace_bytes(n, d), dtype=torch.uint8, device="cuda")
    gw1 = torch.full((d, d), float("nan"), device="cuda")
    gw2 = torch.full((d, d), float("nan"), device="cuda")
    gb = torch.full((d,), float("nan"), device="cuda")
    dp_d, ax_d, am_d = cu(dp), cu(ax), cu(am)
    args = (n, d, dp_d.data_ptr(), ax_d.data_ptr(), am_d.data_ptr())
    G._lib.check(G.lib.gss_dense_bwd_weight(*args, None, gw1.data_ptr(), gw2.data_ptr(), gb.data_ptr(), 0, ws.data_ptr(), G.st()))
    r1 = dp.T.astype(np.float64) @ ax
    r2 = dp.T.astype(np.float64) @ am
    rb = dp.astype(np.float64).sum(0)
    assert rel_err(gw1.cpu().numpy(), r1) < 3e-6
    assert rel_err(gw2.cpu().numpy(), r2) < 3e-6
    assert rel_err(gb.cpu().numpy(), rb) < 3e-6
    first = gw1.clone()
    G._lib.check(G.lib.gss_dense_bwd_weight(*args, None, gw1.data_ptr(), gw2.data_ptr(), gb.data_ptr(), 1, ws.data_ptr(), G.st()))
    assert rel_err(gw1.cpu().numpy(), 2 * r1) < 3e-6 and rel_err(gb.cpu().numpy(), 2 * rb) < 3e-6
    G._lib.check(G.lib.gss_dense_bwd_weight(*args, None, gw1.data_ptr(), gw2.data_ptr(), gb.data_ptr(), 0, ws.data_ptr(), G.st()))
    assert torch.equal(gw1, first)  # reproducible
    # gathered rows: dp compact [b][d], ax/am indexed
    b = max(1, n // 3)
    rows = rng.permutation(n)[:b].astype(np.int32)
    rows_d = cu(rows)
    G._lib.check(G.lib.gss_dense_bwd_weight(b, d, dp_d.data_ptr(), ax_d.data_ptr(), am_d.data_ptr(), rows_d.data_ptr(),
                                            gw1.data_ptr(), gw2.data_ptr(), gb.data_ptr(), 0, ws.data_ptr(), G.st()))
    assert rel_err(gw1.cpu().numpy(), dp[:b].T.astype(np.float64) @ ax[rows]) < 3e-6
    assert rel_err(gw2.cpu().numpy(), dp[:b].T.astype(np.float64) @ am[rows]) < 3e-6


# ---------------------------------------------------------------- K5
@pytest.mark.parametrize("n,d", [(1000, 128), (33, 16), (257, 64), (100, 512), (64, 1024)])
def test_rownorm_fwd_and_bwd(G, n, d):
    rng = np.random.RandomState(d)
    x = rng.randn(n, d).astype(np.float32)
    x[0] = 0  # norm below eps -> 0 / eps
    e = torch.empty(n, d, device="cuda")
    inv = torch.empty(n, device="cuda")
    x_d = cu(x)
    G._lib.check(G.lib.gss_rownorm_fwd(n, d, x_d.data_ptr(), e.data_ptr(), inv.data_ptr(), G.st()))
    den = np.maximum(np.sqrt((x.astype(np.float64) ** 2).sum(1)), 1e-12)
    assert rel_err(e.cpu().numpy(), x / den[:, None]) < 1e-6
    assert np.all(e.cpu().numpy()[0] == 0)
    b = max(1, n // 2)
    rows = rng.permutation(np.arange(1, n))[:b].astype(np.int32)
    de = rng.randn(b, d).astype(np.float32)
    p = rng.randn(n, d).astype(np.float32)
    dx = torch.empty(b, d, device="cuda")
    dpb = torch.empty(b, d, device="cuda")
    de_d, rows_d, p_d = cu(de), cu(rows), cu(p)
    G._lib.check(G.lib.gss_rownorm_elu_bwd(d, de_d.data_ptr(), rows_d.data_ptr(), b, e.data_ptr(), inv.data_ptr(),
                                           p_d.data_ptr(), 0.4, dx.data_ptr(), dpb.data_ptr(), G.st()))
    eb = (x / den[:, None])[rows]
    dxr = (de - eb * (eb * de).sum(1, keepdims=True)) / den[rows][:, None]
    assert rel_err(dx.cpu().numpy(), dxr) < 3e-6
    assert rel_err(dpb.cpu().numpy(), 0.4 * dxr * np.where(p[rows] > 0, 1.0, np.exp(np.minimum(p[rows], 0)))) < 3e-6


# ---------------------------------------------------------------- K6 / K7
@pytest.mark.parametrize("n,d,b", [(3000, 128, 2048), (500, 16, 500), (400, 64, 1), (900, 256, 333), (300, 32, 17), (2000, 128, 1288),
                                   (700, 192, 200), (600, 512, 130), (500, 320, 77), (400, 48, 50), (2100, 256, 2048),
                                   (200, 576, 33), (200, 1024, 50)])      # d > 512: the sweep's second 512-feature slab, masked and exact
def test_loss_fwd_bwd(G, n, d, b):
    loss_fwd_bwd_case(G, n, d, b)


@pytest.mark.parametrize("wgs", [64, 4096])
def test_loss_fwd_bwd_loss_wgs(G, wgs):
    """the knob that sets the j split: 65 row tiles at loss_wgs = 64 / 4096 sweep with js = 1 / 16 (the cap)"""
    try:
        G._lib.check(G.lib.gss_debug_set_option(b"loss_wgs", wgs))
        loss_fwd_bwd_case(G, 2100, 64, 1040)
    finally:
        G._lib.check(G.lib.gss_debug_set_option(b"loss_wgs", 256))


def loss_fwd_bwd_case(G, n, d, b):
    rng = np.random.RandomState(b)
    x = rng.randn(n, d)
    x[:, 0] += 1.0  # mostly positive similarities, some negative
    e = (x / np.sqrt((x ** 2).sum(1, keepdims=True))).astype(np.float32)
    idx = rng.permutation(n)[:b].astype(np.int32)
    beta, alpha = 0.25, 1.7
    loss = torch.zeros(1, device="cuda")
    de = torch.full((b, d), float("nan"), device="cuda")
    ws = torch.empty(G.lib.gss_loss_workspace_bytes(b, d), dtype=torch.uint8, device="cuda")
    e_d, idx_d = cu(e), cu(idx)
    G._lib.check(G.lib.gss_loss_fwd_bwd(n, d, e_d.data_ptr(), idx_d.data_ptr(), b, beta, alpha, loss.data_ptr(),
                                        de.data_ptr(), ws.data_ptr(), G.st()))
    e64 = e.astype(np.float64)
    lref = O.gss_loss(e64, beta, idx, alpha)
    dref = O.loss_grad_emb(e64, beta, idx, alpha)[idx]
    assert abs(loss.item() - lref) < 2e-6 * abs(lref)
    assert rel_err(de.cpu().numpy(), dref) < 5e-6


# ---------------------------------------------------------------- K10
def test_adam_matches_torch_semantics(G):
    rng = np.random.RandomState(0)
    d = 48
    params = {k: rng.randn(*s).astype(np.float32) for k, s in (("W1", (d, d)), ("b1", (d,)), ("W2", (d, d)), ("b2", (d,)))}
    ref = {k: v.copy() for k, v in params.items()}
    dev = {k: cu(v) for k, v in params.items()}
    m = {k: torch.zeros_like(v) for k, v in dev.items()}
    v2 = {k: torch.zeros_like(v) for k, v in dev.items()}
    wt = torch.empty(d, d, device="cuda")
    state = {}
    for step in range(1, 6):
        grads = {k: (rng.randn(*v.shape) * 10 ** rng.uniform(-6, 0)).astype(np.float32) for k, v in params.items()}
        O.adam_step(ref, grads, state, 3e-4)
        gd = {k: cu(v) for k, v in grads.items()}
        for k in dev:
            G._lib.check(G.lib.gss_adam_step(dev[k].numel(), dev[k].data_ptr(), gd[k].data_ptr(), m[k].data_ptr(),
                                             v2[k].data_ptr(), step, 3e-4, 0.9, 0.999, 1e-8,
                                             wt.data_ptr() if k == "W1" else None, d if k == "W1" else 0, G.st()))
        for k in dev:
            assert np.abs(dev[k].cpu().numpy() - ref[k]).max() < 2.5e-7 * max(1.0, np.abs(ref[k]).max())  # 1-2 ulp
        assert torch.equal(wt, dev["W1"].t())


# ---------------------------------------------------------------- K12
@pytest.mark.parametrize("n,d,q", [(700, 64, 98.0), (129, 16, 50.0), (1000, 128, 99.9), (300, 32, 0.0), (300, 32, 100.0)])
def test_percentile_exact(G, n, d, q):
    rng = np.random.RandomState(n)
    x = rng.randn(n, d)
    e = (x / np.sqrt((x ** 2).sum(1, keepdims=True))).astype(np.float32)
    ed = cu(e)
    out = C.c_float()
    G._lib.check(G.lib.gss_percentile(n, d, ed.data_ptr(), q, C.byref(out), G.st()))
    ref = np.percentile((e.astype(np.float64) @ e.astype(np.float64).T).flatten(), q)
    assert abs(out.value - ref) < 2e-6


def test_bad_arguments_fail_loudly(G):
    x = torch.zeros(10, 20, device="cuda")
    with pytest.raises(G._lib.GssError, match="multiple of 16"):
        G._lib.check(G.lib.gss_rownorm_fwd(10, 20, x.data_ptr(), x.data_ptr(), x.data_ptr(), G.st()))
    with pytest.raises(G._lib.GssError):
        G._lib.check(G.lib.gss_dense_fwd(10, 16, None, None, None, None, None, None, None, 0.3, None, None, G.st()))


# ---------------------------------------------------------------- a1 (kNN graph on device)
@pytest.mark.parametrize("name", ["knn_n200_d16_L2", "knn_n2000_d64_L3"])
def test_knn_graph_device_matches_reference_gen_graph(G, name):
    g = load_golden(name)
    ref = golden_csr(g, "A")
    adj = G.graph.knn_descriptor_adj_device(g["X"].astype(np.float64), 5)
    assert np.array_equal(adj.indptr, ref.indptr) and np.array_equal(adj.indices, ref.indices)
    np.testing.assert_allclose(adj.data, ref.data, rtol=1e-12)


def test_knn_topk_values_and_odd_sizes(G):
    rng = np.random.RandomState(3)
    for n, d, k in ((333, 24, 7), (65, 8, 64), (1000, 128, 5)):
        x = rng.randn(n, d)
        xd = cu(x)
        tv = torch.empty(n, k, dtype=torch.float64, device="cuda")
        ti = torch.empty(n, k, dtype=torch.int32, device="cuda")
        G._lib.check(G.lib.gss_knn_topk(n, d, xd.data_ptr(), k, tv.data_ptr(), ti.data_ptr(), G.st()))
        sim = x @ x.T
        ref_idx = np.argpartition(sim, -k, 1)[:, -k:]
        got_idx = ti.cpu().numpy()
        assert np.array_equal(np.sort(got_idx, 1), np.sort(ref_idx, 1))
        np.testing.assert_allclose(np.sort(tv.cpu().numpy(), 1), np.sort(np.take_along_axis(sim, ref_idx, 1), 1), rtol=1e-12)


def test_knn_topk_k_sweep_writes_only_its_outputs(G):
    """every k the entry point accepts (1 .. 64: its LDS footprint grows with k) at node counts around the 64-row tile, outputs embedded
    in canary-filled buffers: results equal numpy's, nothing outside [n][k] is written"""
    rng = np.random.RandomState(4)
    for n in (64, 65, 127, 130):
        x = rng.randn(n, 16)
        xd = cu(x)
        sim = x @ x.T
        for k in (1, 2, 3, 5, 8, 13, 21, 34, 55, 63, 64):
            pad = 257
            tv = torch.full((n * k + 2 * pad,), -7.25, dtype=torch.float64, device="cuda")
            ti = torch.full((n * k + 2 * pad,), -77, dtype=torch.int32, device="cuda")
            G._lib.check(G.lib.gss_knn_topk(n, 16, xd.data_ptr(), k, tv[pad:].data_ptr(), ti[pad:].data_ptr(), G.st()))
            torch.cuda.synchronize()
            assert bool((tv[:pad] == -7.25).all()) and bool((tv[pad + n * k:] == -7.25).all()), (n, k)
            assert bool((ti[:pad] == -77).all()) and bool((ti[pad + n * k:] == -77).all()), (n, k)
            got_idx = ti[pad:pad + n * k].view(n, k).cpu().numpy()
            ref_idx = np.argpartition(sim, -k, 1)[:, -k:]
            assert np.array_equal(np.sort(got_idx, 1), np.sort(ref_idx, 1)), (n, k)
    with pytest.raises(G._lib.GssError):
        G._lib.check(G.lib.gss_knn_topk(10, 16, xd.data_ptr(), 65, tv.data_ptr(), ti.data_ptr(), G.st()))


def test_percentile_size_sweep(G):
    """node counts around the 64-row tiles of the select kernel (1 row .. just past two tiles), the percentiles at both ends included"""
    rng = np.random.RandomState(6)
    for n in (1, 2, 3, 63, 64, 65, 127, 128, 129, 200):
        x = rng.randn(n, 16)
        e = (x / np.sqrt((x ** 2).sum(1, keepdims=True))).astype(np.float32)
        ed = cu(e)
        s = (e.astype(np.float64) @ e.astype(np.float64).T).flatten()
        for q in (0.0, 37.5, 50.0, 98.0, 100.0):
            out = C.c_float()
            G._lib.check(G.lib.gss_percentile(n, 16, ed.data_ptr(), q, C.byref(out), G.st()))
            assert abs(out.value - np.percentile(s, q)) < 2e-6, (n, q)


def test_library_loaded_before_torch_still_sees_the_gpu():
    """torch ships its own HIP runtime; a process that loads libgssgcn.so first (build() then smoke() in one interpreter)
    must end up with ONE runtime.  Run in a child process so the import order is really this one."""
    import os
    import subprocess
    import sys
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import __graft_entry__ as g\n"
        "g.build()\n"                       # loads the library before anything imported torch
        "import torch, numpy as np\n"
        "import gcn_drug_repurposing_amd as pkg\n"
        "from gcn_drug_repurposing_amd.graph import GssGraph\n"
        "import scipy.sparse as sp\n"
        "a = sp.random(300, 300, density=0.03, random_state=1, format='csr'); a = a + a.T\n"
        "gg = GssGraph(a)\n"
        "x = torch.ones(300, 16, device='cuda'); y = torch.empty_like(x)\n"
        "pkg._lib.check(pkg.load().gss_spmm(gg.a.handle, 16, x.data_ptr(), y.data_ptr(), None, None, pkg._lib.current_stream()))\n"
        "torch.cuda.synchronize(); print('rowsum', float(y[:, 0].sum()))\n"
    ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "rowsum" in out.stdout


@pytest.mark.parametrize("workload", ["whole_graph", "rmat_300k"])
def test_full_size_spmm_properties(G, workload):
    """size-independent properties of the SpMM pair (CSR of A_hat and of its transpose) at full size: the row sums
    A_hat 1, adjointness <A x, y> = <x, A^T y>, linearity, and the fused Hadamard epilogue against two launches"""
    from gcn_drug_repurposing_amd import synth
    if workload == "whole_graph":
        adj = synth.whole_graph_standin(seed=1)[0]
    else:
        adj = synth.rmat_adj(300_000, 6_000_000, seed=4)     # table 150 MB: the time-separated slicing path
    gg = G.graph.GssGraph(adj)
    n, d = gg.n, 128
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(n, d, device="cuda", generator=gen)
    y = torch.randn(n, d, device="cuda", generator=gen)
    ax, aty = torch.empty_like(x), torch.empty_like(x)
    st = G.st()
    G._lib.check(G.lib.gss_spmm(gg.a.handle, d, x.data_ptr(), ax.data_ptr(), None, None, st))
    G._lib.check(G.lib.gss_spmm(gg.at.handle, d, y.data_ptr(), aty.data_ptr(), None, None, st))
    lhs, rhs = (ax.double() * y.double()).sum().item(), (x.double() * aty.double()).sum().item()
    assert abs(lhs - rhs) < 1e-5 * max(abs(lhs), abs(rhs), 1.0)
    ones = torch.ones(n, 16, device="cuda")
    rs = torch.empty(n, 16, device="cuda")
    G._lib.check(G.lib.gss_spmm(gg.a.handle, 16, ones.data_ptr(), rs.data_ptr(), None, None, st))
    a_hat, _ = O.preprocess_graph(adj)
    ref = np.asarray(a_hat.sum(1)).reshape(-1)
    assert np.abs(rs[:, 0].cpu().numpy() - ref).max() < 1e-5 * max(1.0, np.abs(ref).max())   # row sums within 1e-5
    axy = torch.empty_like(x)
    x2y = x + 2 * y                                    # named: the kernel reads it after this statement
    G._lib.check(G.lib.gss_spmm(gg.a.handle, d, x2y.data_ptr(), axy.data_ptr(), None, None, st))
    ay = torch.empty_like(x)
    G._lib.check(G.lib.gss_spmm(gg.a.handle, d, y.data_ptr(), ay.data_ptr(), None, None, st))
    assert (axy - (ax + 2 * ay)).abs().max().item() < 2e-5 * max(1.0, axy.abs().max().item())
    ax2, m = torch.empty_like(x), torch.empty_like(x)
    G._lib.check(G.lib.gss_spmm(gg.a.handle, d, x.data_ptr(), ax2.data_ptr(), y.data_ptr(), m.data_ptr(), st))
    assert torch.equal(ax2, ax) and torch.equal(m, ax * y)
