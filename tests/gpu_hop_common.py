"""What the op-by-op GPU tests of the SpMM modes share (tests/test_gpu_sparse_ops.py, tests/test_gpu_dense_hops.py, tests/test_gpu_spmm_ladder.py): the library
fixture, the NaN pre-fill that tells a written element from a skipped one, the per-element check of a write set and of the mirror's
derived bound (tests/sparse_hop_mirror.py), the knob context manager and the cache of device CSR handles.  No test lives here."""
import contextlib

import numpy as np
import pytest

import sparse_hop_mirror as M

torch = pytest.importorskip("torch")

PREFILL = 0x7FC0DEAD                 # a quiet NaN with a payload no computation produces
DEFAULTS = {"spmm_list_blocks": 2048, "spmm_giant": 32768, "spmm_variant": 2, "spmm_slices": 0, "spmm_pin": 0, "spmm_hot_rows": -1}


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
    ns.st = lambda: _lib.current_stream()
    ns.csr = {}
    return ns


@contextlib.contextmanager
def knobs(G, **kv):
    """set tuning knobs for the body, restore the defaults whatever happens"""
    try:
        for k, v in kv.items():
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), v))
        yield
    finally:
        for k in kv:
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), DEFAULTS[k]))


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def prefilled(n, d):
    return torch.full((n, d), PREFILL, dtype=torch.int32, device="cuda").view(torch.float32)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def dev_csr(G, a, key):
    if key not in G.csr:
        G.csr[key] = G.graph.DeviceCSR(a.indptr, a.indices, a.data, a.shape[0], a.shape[1], "cuda")
    return G.csr[key]


def untouched(x):
    """per row: every element still holds the pre-fill, bit for bit"""
    return (x.view(np.int32) == np.int32(PREFILL)).all(1)


def fully_written(x):
    """per row: no element holds the pre-fill"""
    return (x.view(np.int32) != np.int32(PREFILL)).all(1)


def assert_rows(got, ref, s, k, written, what):
    """the write set, then the derived bound on the written rows"""
    assert untouched(got)[~written].all(), f"{what}: a row the contract skips was written: {np.flatnonzero(~untouched(got) & ~written)[:8]}"
    assert fully_written(got)[written].all(), f"{what}: a piece of a written row keeps the pre-fill: rows {np.flatnonzero(~fully_written(got) & written)[:8]}"
    err = np.abs(got[written].astype(np.float64) - np.asarray(ref, np.float64)[written])
    lim = M.bound(k, s)[written]
    bad = err > lim
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements beyond (k + 4) 2^-24 S; worst row {np.flatnonzero(written)[np.argmax((err - lim).max(1))]}, "
                           f"err {err[bad].max():.3e} vs bound {lim[bad].min():.3e}")
