"""-m gpu: gss_spmm_fwd_pair -- two forward products over one matrix in ONE launch of the balanced SpMM (spmm.hip
spmm_balanced_pair_kernel), or in two where no paired form exists.

The contract is bit identity with two launches: a workgroup of the second half runs the same block code on the second operand set, so every
row is summed by the same lane groups in the same order.  Every comparison is torch.equal against gss_spmm run twice under the same
knobs; outputs are pre-filled with a NaN of a recognisable payload, so a row that a launch left unwritten differs too.

One graph of 2,500 rows reaches every shape of the schedule at the three widths: row 0 (2,300 entries) takes a whole workgroup with
longer segments (more than 16 waves x lane groups x 32 entries at d = 64, 128 and 256), row 2 (400 entries) spans several waves of a
workgroup, row 1 (100 entries) several segments of one wave, a tenth of the rows and the last twenty are empty, and the row count leaves
the last segment block partly filled.  Slicing: automatic (unsliced at this size), 2 and 4 feature slices pinned to XCDs (grid.x carries
the slice: the second half must keep `linear id mod slices`), 2 slices time-separated (grid.y).

The entry point takes no row or gather filter (a filtered product is never paired: the plan calls the filtered launcher on its own), so
the fallbacks it can report are the giant-row passes and spmm_variant 1."""
import contextlib
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 2500
PREFILL = 0x7FC0DEAD
DEFAULTS = {"spmm_giant": 32768, "spmm_variant": 2, "spmm_slices": 0, "spmm_pin": 0}
SLICING = {"auto": {}, "pin2": {"spmm_slices": 2, "spmm_pin": 1}, "pin4": {"spmm_slices": 4, "spmm_pin": 1}, "time2": {"spmm_slices": 2, "spmm_pin": 0}}


@functools.lru_cache(maxsize=None)
def _matrix():
    import scipy.sparse as sp
    rng = np.random.RandomState(11)
    deg = rng.randint(1, 9, size=N)
    deg[rng.rand(N) < 0.1] = 0
    deg[-20:] = 0
    deg[0], deg[1], deg[2] = 2300, 100, 400
    indptr = np.zeros(N + 1, np.int32)
    indptr[1:] = np.cumsum(deg)
    indices = np.concatenate([np.sort(rng.choice(N, k, replace=False)) for k in deg]).astype(np.int32)
    data = (rng.rand(indptr[-1]) + 0.1).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(N, N))


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
    ns.csr = {}
    return ns


def _csr(G, key="default"):
    """one handle per knob setting that shapes what a handle caches (the giant-row views)"""
    if key not in G.csr:
        a = _matrix()
        G.csr[key] = G.graph.DeviceCSR(a.indptr, a.indices, a.data, N, N, "cuda")
    return G.csr[key]


@contextlib.contextmanager
def knobs(G, **kv):
    try:
        for k, v in kv.items():
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), v))
        yield
    finally:
        for k in kv:
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), DEFAULTS[k]))


def prefilled(d):
    return torch.full((N, d), PREFILL, dtype=torch.int32, device="cuda").view(torch.float32)


@functools.lru_cache(maxsize=None)
def _operands(d):
    rng = np.random.RandomState(d)
    return tuple(torch.from_numpy(rng.randn(N, d).astype(np.float32)).cuda() for _ in range(2))


def ptr(t):
    return None if t is None else t.data_ptr()


def single(G, csr, d, x, hadamard):
    y = prefilled(d)
    m = prefilled(d) if hadamard else None
    G._lib.check(G.lib.gss_spmm(csr.handle, d, ptr(x), ptr(y), ptr(x) if hadamard else None, ptr(m), G._lib.current_stream()), "gss_spmm")
    return y, m


def pair(G, csr, d, x0, x1, hadamard, prep=None):
    import ctypes as C
    y0, y1 = prefilled(d), prefilled(d)
    m0, m1 = (prefilled(d), prefilled(d)) if hadamard else (None, None)
    paired = C.c_int32(-1)
    pi, pb, pm, prl, ppid, ppos = prep if prep else (None, 0, None, None, None, None)
    G._lib.check(G.lib.gss_spmm_fwd_pair(csr.handle, d, ptr(x0), ptr(y0), ptr(x0) if hadamard else None, ptr(m0), ptr(x1), ptr(y1),
                                         ptr(x1) if hadamard else None, ptr(m1), ptr(pi), pb, ptr(pm), ptr(prl), ptr(ppid), ptr(ppos),
                                         C.byref(paired), G._lib.current_stream()), "gss_spmm_fwd_pair")
    return (y0, m0, y1, m1), paired.value


def same(a, b):
    """bit for bit (NaN payloads included)"""
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


def written(t):
    return t is None or not bool((t.view(torch.int32) == PREFILL).any())


@pytest.mark.parametrize("slicing", list(SLICING))
@pytest.mark.parametrize("hadamard", [True, False], ids=["fwd1", "plain"])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_a_paired_launch_gives_the_bits_of_two_launches(G, d, hadamard, slicing):
    x0, x1 = _operands(d)
    with knobs(G, **SLICING[slicing]):
        csr = _csr(G)
        ref = single(G, csr, d, x0, hadamard) + single(G, csr, d, x1, hadamard)
        got, paired = pair(G, csr, d, x0, x1, hadamard)
    assert paired == 1
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same(g, r), (d, hadamard, slicing, "output", k)
        assert written(g), (d, hadamard, slicing, "output", k, "keeps the pre-fill")
    assert not same(got[0], got[2])   # (the halves really used their own operands)


@pytest.mark.parametrize("mapped", [False, True], ids=["ids", "node_map"])
@pytest.mark.parametrize("slicing", list(SLICING))
@pytest.mark.parametrize("d", [64, 128, 256])
def test_the_batch_preparation_rides_first_and_both_halves_keep_their_bits(G, d, slicing, mapped):
    """the launch has one workgroup more, its first: the prepared lists and the position map are what batch_prepare writes, and the
    products behind it are unchanged -- with pinned slices every workgroup id is shifted by one in both halves alike"""
    x0, x1 = _operands(d)
    rng = np.random.RandomState(5)
    b = 77
    idx = rng.permutation(N)[:b].astype(np.int32)
    node_map = rng.permutation(N).astype(np.int32) if mapped else None
    rows = node_map[idx] if mapped else idx
    t_idx = torch.from_numpy(idx).cuda()
    t_map = torch.from_numpy(node_map).cuda() if mapped else None
    rloc = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    pid = torch.full((b,), -7, dtype=torch.int32, device="cuda")
    pos = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    with knobs(G, **SLICING[slicing]):
        csr = _csr(G)
        ref = single(G, csr, d, x0, True) + single(G, csr, d, x1, True)
        got, paired = pair(G, csr, d, x0, x1, True, prep=(t_idx, b, t_map, rloc, pid, pos))
    assert paired == 1
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same(g, r), (d, slicing, mapped, "output", k)
    want_pos = np.full(N, -1, np.int32)
    want_pos[rows] = np.arange(b, dtype=np.int32)
    assert np.array_equal(pos.cpu().numpy(), want_pos)
    assert np.array_equal(rloc.cpu().numpy(), rows) and np.array_equal(pid.cpu().numpy(), rows)


@pytest.mark.parametrize("d", [64, 128, 256])
def test_what_the_second_half_writes_feeds_the_next_paired_launch(G, d):
    """the plan's use: the Hadamard-fused pair writes M of both products, the plain pair right behind it gathers from both"""
    x0, x1 = _operands(d)
    csr = _csr(G)
    r0, r1 = single(G, csr, d, x0, True), single(G, csr, d, x1, True)
    ref = (single(G, csr, d, r0[1], False)[0], single(G, csr, d, r1[1], False)[0])
    (_, m0, _, m1), p1 = pair(G, csr, d, x0, x1, True)
    (z0, _, z1, _), p2 = pair(G, csr, d, m0, m1, False)
    assert (p1, p2) == (1, 1)
    assert same(z0, ref[0]) and same(z1, ref[1])


@pytest.mark.parametrize("hadamard", [True, False], ids=["fwd1", "plain"])
@pytest.mark.parametrize("why,kv", [("giant_rows", {"spmm_giant": 64}), ("row_per_wave", {"spmm_variant": 1})])
def test_requests_without_a_paired_form_run_two_launches_and_say_so(G, why, kv, hadamard):
    """spmm_giant = 64: rows 0, 1 and 2 are summed chunk by chunk in three passes per product; spmm_variant = 1 has no balanced launch"""
    d = 128
    x0, x1 = _operands(d)
    with knobs(G, **kv):
        csr = _csr(G, why)
        ref = single(G, csr, d, x0, hadamard) + single(G, csr, d, x1, hadamard)
        got, paired = pair(G, csr, d, x0, x1, hadamard)
    assert paired == 0
    for k, (g, r) in enumerate(zip(got, ref)):
        assert same(g, r) and written(g), (why, hadamard, k)


def test_mixed_modes_are_refused_before_any_launch(G):
    d = 64
    x0, x1 = _operands(d)
    y0, y1, m0 = prefilled(d), prefilled(d), prefilled(d)
    rc = G.lib.gss_spmm_fwd_pair(_csr(G).handle, d, ptr(x0), ptr(y0), ptr(x0), ptr(m0), ptr(x1), ptr(y1), None, None, None, 0, None, None, None,
                                 None, None, G._lib.current_stream())
    assert rc != 0 and "both" in G.lib.gss_last_error().decode()
    torch.cuda.synchronize()
    assert bool((y0.view(torch.int32) == PREFILL).all()) and bool((y1.view(torch.int32) == PREFILL).all())
