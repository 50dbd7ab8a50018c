"""-m gpu: a shard's rows have the bits of the one-GPU product's rows where the SpMM's automatic slice policy would decide differently
on the shard's own operand than on the whole graph's (tests/shard_grouping_cases.py: N just above the 8 MiB threshold at d = 1024, 256
and 128, every shard far below it, planted rows either side of every regrouping length).

Op level: gss_spmm plain and Hadamard-fused, gss_spmm_add in place and gss_spmm_fwd_pair, on the whole-graph handle and on every node
range's shard handle (shard_of: the trainer's renumbering).  With the job's operand rows declared on the shard handle
(gss_csr_set_job_cols) every output row equals the whole graph's bit for bit; without it -- the behaviour before the declaration
existed, kept here as the proof that the cases can see the defect -- every planted row above the regrouping length differs on some
feature while the rows of <= 64 entries agree.  Both sides always meet sparse_hop_mirror.bound(k, S) against the fp64 product, which
depends on neither kernel.  (Measured on the library before the declaration: 12 of 20 planted rows differed at d = 128, 24 of 30 at
d = 256, 16 of 20 at d = 1024 -- on 36 to 888 of a row's features --, no other row did.)  The straddle itself is asserted through gss_spmm_auto_slices, not through a copied constant.

Plan level: the sharded plan through both shard builders (an A_hat sliced on the host; build_shard normalising on the device)
against GssEngine on one GPU: embeddings array-equal, loss ==, every rank's matrices report the job's N."""
import contextlib
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import shard_grouping_cases as SG
import sparse_hop_mirror as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEFAULTS = {"spmm_giant": 32768, "spmm_slices": 0, "spmm_pin": 0}
PREFILL = 0x7FC0DEAD
CASES = [(d, k) for d in sorted(SG.SIZES) for k in range(SG.SIZES[d][1])]
PRODUCTS = ("plain", "fwd1_y", "fwd1_m", "add_y", "add_m", "pair_y0", "pair_m0", "pair_y1", "pair_m1")


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import gcn_drug_repurposing_amd as pkg
    from gcn_drug_repurposing_amd import _lib, graph

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib, ns.graph = pkg.load(), _lib, graph
    ns.whole = {}
    return ns


@contextlib.contextmanager
def knobs(G, **kv):
    try:
        for k, v in kv.items():
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), v))
        yield
    finally:
        for k in kv:
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), DEFAULTS[k]))


def auto_slices(G, d, cols):
    ns, pin = C.c_int32(-1), C.c_int32(-1)
    G._lib.check(G.lib.gss_spmm_auto_slices(d, int(cols), C.byref(ns), C.byref(pin)), "gss_spmm_auto_slices")
    return ns.value, pin.value


def job_cols(G, csr):
    out = C.c_int64(-1)
    G._lib.check(G.lib.gss_csr_job_cols(csr.handle, C.byref(out)), "gss_csr_job_cols")
    return out.value


def handle(G, a, declare=None):
    csr = G.graph.DeviceCSR(a.indptr, a.indices, a.data, a.shape[0], a.shape[1], "cuda")
    if declare is not None:
        G._lib.check(G.lib.gss_csr_set_job_cols(csr.handle, int(declare)), "gss_csr_set_job_cols")
    return csr


@functools.lru_cache(maxsize=None)
def operands(d):
    """the second operand of the pair and the first pass's sums of the two-pass product, [N][d] like x"""
    rng = np.random.RandomState(7000 + d)
    n = SG.SIZES[d][0]
    return rng.randn(n, d).astype(np.float32), rng.randn(n, d).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(d):
    """fp64 values and bounds of every product, per row of the whole graph; computed once, never written to.  k = a row's stored entries
    (+ 1 with y_in), S = the expression with the absolute value of every term."""
    c = SG.case(d)
    x1, yin = operands(d)
    a64 = sp.csr_matrix(c.a, dtype=np.float64)
    aabs = abs(a64)
    k = np.diff(c.a.indptr)
    out = {}
    for name, x in (("x", c.x), ("x1", x1)):
        x64 = x.astype(np.float64)
        y, s = a64 @ x64, aabs @ np.abs(x64)
        out[name] = (y, M.bound(k, s), y * x64, M.bound(k, s * np.abs(x64)))
    y, by, m, bm = out["x"]
    s = aabs @ np.abs(c.x.astype(np.float64)) + np.abs(yin.astype(np.float64))
    ya = yin.astype(np.float64) + y
    ref = {"plain": (y, by), "fwd1_y": (y, by), "fwd1_m": (m, bm), "pair_y0": (y, by), "pair_m0": (m, bm),
           "pair_y1": out["x1"][:2], "pair_m1": out["x1"][2:],
           "add_y": (ya, M.bound(k + 1, s)), "add_m": (ya * c.x.astype(np.float64), M.bound(k + 1, s * np.abs(c.x.astype(np.float64))))}
    for v, b in ref.values():
        v.setflags(write=False)
        b.setflags(write=False)
    return ref


def ptr(t):
    return None if t is None else t.data_ptr()


def prefilled(n, d):
    return torch.full((n, d), PREFILL, dtype=torch.int32, device="cuda").view(torch.float32)


def run_products(G, csr, d, x, h, x1, h1, yin, which=PRODUCTS):
    """x, x1: [n_cols][d] operands; h, h1: [n_rows][d] Hadamard operands; yin: [n_rows][d] -> {product: [n_rows][d] numpy}"""
    lib, st, n = G.lib, G._lib.current_stream(), csr.n_rows
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(x=x, h=h, x1=x1, h1=h1).items()}
    out = {}
    if "plain" in which:
        y = prefilled(n, d)
        G._lib.check(lib.gss_spmm(csr.handle, d, ptr(t["x"]), ptr(y), None, None, st), "gss_spmm")
        out["plain"] = y
    if "fwd1_y" in which:
        y, m = prefilled(n, d), prefilled(n, d)
        G._lib.check(lib.gss_spmm(csr.handle, d, ptr(t["x"]), ptr(y), ptr(t["h"]), ptr(m), st), "gss_spmm")
        out["fwd1_y"], out["fwd1_m"] = y, m
    if "add_y" in which:
        y, m = torch.from_numpy(np.ascontiguousarray(yin)).cuda(), prefilled(n, d)      # in place: y_in is the buffer the pass writes
        G._lib.check(lib.gss_spmm_add(csr.handle, d, ptr(t["x"]), ptr(y), ptr(y), ptr(t["h"]), ptr(m), st), "gss_spmm_add")
        out["add_y"], out["add_m"] = y, m
    if "pair_y0" in which:
        y0, m0, y1, m1 = (prefilled(n, d) for _ in range(4))
        paired = C.c_int32(-1)
        G._lib.check(lib.gss_spmm_fwd_pair(csr.handle, d, ptr(t["x"]), ptr(y0), ptr(t["h"]), ptr(m0), ptr(t["x1"]), ptr(y1), ptr(t["h1"]), ptr(m1),
                                           None, 0, None, None, None, None, C.byref(paired), st), "gss_spmm_fwd_pair")
        out["pair_y0"], out["pair_m0"], out["pair_y1"], out["pair_m1"] = y0, m0, y1, m1
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def whole_products(G, d, key="auto", which=PRODUCTS, csr=None):
    """the whole-graph side, once per (d, knob setting)"""
    if (d, key) not in G.whole:
        c = SG.case(d)
        x1, yin = operands(d)
        csr = csr if csr is not None else handle(G, c.a)
        assert job_cols(G, csr) == c.n                       # an untouched handle: its own operand
        G.whole[(d, key)] = run_products(G, csr, d, c.x, c.x, x1, x1, yin, which)
        for v in G.whole[(d, key)].values():
            v.setflags(write=False)
    return G.whole[(d, key)]


def shard_products(G, d, sh, csr, which=PRODUCTS):
    x1, yin = operands(d)
    x1_local = np.concatenate([x1[sh.lo:sh.hi], x1[sh.halo]])
    return run_products(G, csr, d, sh.x, sh.x[:sh.hi - sh.lo], x1_local, x1[sh.lo:sh.hi], yin[sh.lo:sh.hi], which)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def assert_within_bound(d, got, lo, hi, what):
    ref = reference(d)
    for name, v in got.items():
        want, bnd = ref[name]
        err = np.abs(v.astype(np.float64) - want[lo:hi])
        assert not (bits(v) == PREFILL).any(), (what, name, "rows keep the pre-fill")
        bad = err > bnd[lo:hi]
        assert not bad.any(), (what, name, "rows", np.flatnonzero(bad.any(1))[:5] + lo, float((err / np.maximum(bnd[lo:hi], 1e-300)).max()))


def straddles(G, d, n, n_cols_shard):
    ns, _ = auto_slices(G, d, n)
    return ns > 1 and auto_slices(G, d, n_cols_shard) == (1, 0)


@pytest.mark.parametrize("d,k", CASES)
def test_a_declared_shard_gives_the_whole_graphs_bits(G, d, k):
    c = SG.case(d)
    lo, hi = c.ranges[k]
    sh = SG.shard_of(c.a, lo, hi, c.x)
    assert straddles(G, d, c.n, sh.n_cols)
    whole = whole_products(G, d)
    assert_within_bound(d, whole, 0, c.n, ("whole", d))
    csr = handle(G, sh.a)
    assert job_cols(G, csr) == sh.n_cols
    assert G.lib.gss_csr_set_job_cols(csr.handle, sh.n_cols - 1) != 0          # a job holds at least this handle's operand
    G._lib.check(G.lib.gss_csr_set_job_cols(csr.handle, c.n))
    assert job_cols(G, csr) == c.n
    got = shard_products(G, d, sh, csr)
    assert sorted(got) == sorted(PRODUCTS)
    assert_within_bound(d, got, lo, hi, ("shard", d, k))
    for name in PRODUCTS:
        diff = (bits(got[name]) != bits(whole[name][lo:hi])).any(1)
        assert not diff.any(), (d, k, name, "rows (global)", np.flatnonzero(diff)[:8] + lo, "lengths", np.diff(c.a.indptr)[lo:hi][diff][:8])


@pytest.mark.parametrize("d,k", CASES)
def test_an_undeclared_shard_regroups_its_long_rows(G, d, k):
    """the behaviour before gss_csr_set_job_cols, and still that of a handle nobody declares anything on: the shard decides from its own
    operand, runs unsliced, and every planted row above the regrouping length is rounded differently from the whole graph's -- within
    the bound, but not the same bits.  Rows of <= 64 entries (at most two segments: one addition, whatever the grouping) agree."""
    c = SG.case(d)
    lo, hi = c.ranges[k]
    sh = SG.shard_of(c.a, lo, hi, c.x)
    assert straddles(G, d, c.n, sh.n_cols)
    whole = whole_products(G, d)
    csr = handle(G, sh.a)
    which = ("plain", "fwd1_y", "fwd1_m")
    got = shard_products(G, d, sh, csr, which)
    assert job_cols(G, csr) == sh.n_cols
    assert_within_bound(d, got, lo, hi, ("undeclared shard", d, k))
    lens = np.diff(c.a.indptr)[lo:hi]
    for name in which:
        diff = (bits(got[name]) != bits(whole[name][lo:hi])).any(1)
        short = lens <= SG.REGROUP_ABOVE[d]          # (>= 64; at d = 128 three or four segments are (s0+s1)+(s2+s3) under both groupings)
        assert not diff[short].any(), (d, k, name, np.flatnonzero(diff & short)[:8] + lo)
        for r, ln in c.planted[k]:
            if ln > SG.REGROUP_ABOVE[d]:
                assert diff[r - lo], (d, k, name, "planted row", r, "of", ln, "entries has the whole graph's bits on every feature")


@pytest.mark.parametrize("k", range(SG.SIZES[1024][1]))
def test_giant_rows_group_alike_in_all_three_passes(G, k):
    """spmm_giant = 64 on both sides: every row above 64 entries is summed as chunks of 16, in three launches (chunks, the other rows,
    finish) over three views of the handle.  The views carry the handle's declaration -- the finish view too, whose own operand is the
    few chunk sums -- also when it arrives after they were built."""
    d = 1024
    c = SG.case(d)
    lo, hi = c.ranges[k]
    sh = SG.shard_of(c.a, lo, hi, c.x)
    which = ("plain", "fwd1_y", "fwd1_m", "add_y", "add_m")
    with knobs(G, spmm_giant=64):
        whole = whole_products(G, d, "giant64", which)
        csr = handle(G, sh.a)
        ng, nc = C.c_int32(-1), C.c_int32(-1)
        G._lib.check(G.lib.gss_csr_giant_rows(csr.handle, C.byref(ng), C.byref(nc)))     # (builds the views, undeclared)
        lens = np.diff(sh.a.indptr)
        assert ng.value == int((lens > 64).sum()) >= 8 and nc.value == int(sum(-(-int(ln) // 16) for ln in lens[lens > 64]))
        G._lib.check(G.lib.gss_csr_set_job_cols(csr.handle, c.n))
        got = shard_products(G, d, sh, csr, which)
    assert_within_bound(d, whole, 0, c.n, ("whole, giant rows", d))
    assert_within_bound(d, got, lo, hi, ("shard, giant rows", d, k))
    for name in which:
        diff = (bits(got[name]) != bits(whole[name][lo:hi])).any(1)
        assert not diff.any(), (k, name, np.flatnonzero(diff)[:8] + lo)


@pytest.mark.parametrize("d,k", CASES)
def test_forced_slices_give_the_same_bits_whatever_the_handles_declare(G, d, k):
    c = SG.case(d)
    lo, hi = c.ranges[k]
    sh = SG.shard_of(c.a, lo, hi, c.x)
    which = ("plain", "fwd1_y", "fwd1_m")
    with knobs(G, spmm_slices=4):
        whole = whole_products(G, d, "slices4", which)
        got = [shard_products(G, d, sh, handle(G, sh.a, declare), which) for declare in (None, c.n)]
    for g in got:
        assert_within_bound(d, g, lo, hi, ("forced slices", d, k))
        for name in which:
            assert np.array_equal(bits(g[name]), bits(whole[name][lo:hi])), (d, k, name)


def test_an_untouched_handle_of_the_benchmarks_shape_keeps_its_launches(G):
    """N = 29,960, d = 128: the handle reports its own operand and the policy picks two slices pinned to XCDs, as before the job count existed"""
    n = 29960
    indptr = np.arange(17, dtype=np.int32)
    a = sp.csr_matrix((np.ones(16, np.float32), np.arange(16, dtype=np.int32) * 1800, indptr), shape=(16, n))
    csr = handle(G, a)
    assert job_cols(G, csr) == n
    assert auto_slices(G, 128, job_cols(G, csr)) == (2, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# plan level
# ---------------------------------------------------------------------------------------------------------------------------------
BETA, DECAY, ALPHA, LR, BATCH = 0.25, 0.3, 1.0, 3e-4, 256


def _threaded(world, fn, comms):
    results, errors = [None] * world, []

    def worker(rank):
        try:
            torch.cuda.set_device(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                results[rank] = fn(rank)
                torch.cuda.current_stream().synchronize()
        except Exception as e:  # noqa: BLE001
            import traceback
            errors.append((rank, repr(e), traceback.format_exc()))
            comms[rank].abort()               # release the peers now instead of after the barrier timeout

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(600) for t in ts]
    assert not errors, errors
    assert all(r is not None for r in results), "a rank thread did not finish"
    return results


@pytest.mark.parametrize("d,world,path", [(256, 3, "a_hat"), (1024, 2, "build_shard")])
def test_sharded_plan_equals_single_gpu_plan_across_the_slice_threshold(G, d, world, path):
    """L = 2.  One forward + loss + backward, then one lazy step, on `world` in-process ranks and on one GPU.  Every rank's own operand
    is below the slice threshold, the job's N above it (asserted per rank on the rank's real matrices): embeddings and both losses are
    the one-GPU plan's bit for bit, gradients to fp32 summation order (the bound of test_native_sharded_plan_first_step_equals_single_gpu_plan)."""
    from gcn_drug_repurposing_amd.dist import local_comms, sharded_plan_engine
    from gcn_drug_repurposing_amd.engine import GssEngine
    from gcn_drug_repurposing_amd.graph import GssGraph
    from oracle import gss_oracle as O
    c = SG.case(d)
    adj = SG.adjacency(c)
    X = np.ascontiguousarray(c.x * np.float32(0.125))
    np.random.seed(d)
    p0 = O.init_layer_weights(d, 1e-2)
    idx = np.random.RandomState(d + 1).permutation(c.n)[:BATCH].astype(np.int32)
    a_hat = None
    if path == "a_hat":
        a_hat = O.to_fp32_csr(O.preprocess_graph(adj)[0])
        graph = GssGraph.from_normalized(a_hat)
    else:
        graph = GssGraph(adj)                # both normalise on the device: the same A_hat bits
    kw = dict(num_layers=2, layer_decay=DECAY, alpha=ALPHA, lr=LR, max_batch=BATCH)
    single = GssEngine(graph, torch.from_numpy(X).cuda(), [torch.from_numpy(p0[k].copy()).cuda() for k in ("W1", "b1", "W2", "b2")], **kw)
    assert job_cols(G, graph.a) == job_cols(G, graph.at) == c.n
    t1 = torch.from_numpy(idx).cuda()
    single.forward()
    emb1 = single.emb.cpu().numpy().copy()
    single.loss_backward(t1, BETA)
    loss1 = single.loss.item()
    grads1 = [g.cpu().numpy().copy() for g in single.grads]
    single.step_lazy(t1, BETA)
    lazy1 = single.loss.item()
    assert np.isfinite(emb1).all() and np.isfinite(loss1) and np.isfinite(lazy1) and loss1 != 0.0
    comms = local_comms(world)

    def rank_fn(rank):
        eng = sharded_plan_engine(adj, X, p0, comms[rank], device=torch.device("cuda:0"), a_hat=a_hat, **kw)
        t = torch.from_numpy(idx).cuda()
        eng.forward()
        eng.loss_backward(t, BETA)
        res = dict(emb=eng.gather_embeddings().cpu().numpy(), loss=eng.loss.item(), grads=[g.cpu().numpy() for g in eng.grads], rows=eng.n,
                   overlapped=eng.layout.overlapped, relabelled=eng.node_map is not None,
                   cols=[(m.n_cols, job_cols(G, m)) for m in (eng.graph.a, eng.graph.at)])
        eng.step_lazy(t, BETA)
        eng.check_guards()
        res["lazy"] = eng.loss.item()
        return res

    out = _threaded(world, rank_fn, comms)
    assert sum(o["rows"] for o in out) == c.n
    assert auto_slices(G, d, c.n)[0] > 1
    for rank, o in enumerate(out):
        assert not o["overlapped"] and not o["relabelled"]          # (a split row is two sums; these plans keep rows whole)
        for n_cols, declared in o["cols"]:
            assert declared == c.n, (rank, n_cols, declared)
            assert n_cols < c.n and auto_slices(G, d, n_cols) == (1, 0), (rank, n_cols)
        np.testing.assert_array_equal(o["emb"], emb1)
        assert o["loss"] == loss1
        assert o["lazy"] == lazy1
        for got, ref in zip(o["grads"], grads1):
            assert np.abs(got - ref).max() < 1e-5 * np.abs(ref).max() + 1e-12
