"""GPU: the entry points that own call-scoped device scratch or a reused status word (csrc/device_scope.h).  Two things:
  gss_walk_prefix's own refusal of a weight that is not positive and finite, by CSR entry number (node2vec.py refuses such weights on
    the host first, so nothing else reaches it);
  a refused call leaves nothing behind: a valid call, a call refused (-22) through the device status word, the valid call again on the
    same stream, and the second result is bit-equal to the first.
Every shape is the smallest the entry point takes; nothing here has a tolerance."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from gcn_drug_repurposing_amd import _lib

pytestmark = pytest.mark.gpu
EINVAL = -22


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _error():
    return _lib.load().gss_last_error().decode()


def _valid_refused_valid(valid, *refused):
    """valid() -> host tensors of a call that succeeds; each of refused is (call -> rc, words of the refusal)"""
    kept = valid()
    for call, words in refused:
        assert call() == EINVAL
        assert words in _error(), _error()
        again = valid()
        assert len(again) == len(kept)
        for a, b in zip(again, kept):
            assert a.dtype == b.dtype and torch.equal(a, b)


# ---- gss_walk_prefix: a 3-node CSR with 4 entries ---------------------------------------------------------------------------------------
ROWPTR3 = np.array([0, 2, 3, 4], np.int32)
VAL3 = np.array([0.5, 1.5, 2.0, 0.25])


def _walk_prefix(val):
    rowptr, v = _dev(ROWPTR3), _dev(np.asarray(val, np.float64))
    cum = torch.full((4,), -7.0, dtype=torch.float64, device="cuda")
    rc = _lib.load().gss_walk_prefix(3, _lib.ptr(rowptr), _lib.ptr(v), _lib.ptr(cum), _lib.current_stream())
    return rc, cum.cpu()


def test_walk_prefix_sums_rows():
    rc, cum = _walk_prefix(VAL3)
    assert rc == 0, _error()
    assert torch.equal(cum, torch.tensor([0.5, 2.0, 2.0, 0.25], dtype=torch.float64))


@pytest.mark.parametrize("bad", [0.0, -1.0, math.nan, math.inf])
def test_walk_prefix_refuses_weight_by_entry(bad):
    val = VAL3.copy()
    val[2] = bad
    rc, _ = _walk_prefix(val)
    assert rc == EINVAL
    assert "walk_prefix: edge weight of CSR entry 2 is not positive and finite" in _error(), _error()


def test_walk_prefix_names_the_smaller_entry():
    val = VAL3.copy()
    val[3] = -1.0
    val[1] = math.nan
    rc, _ = _walk_prefix(val)
    assert rc == EINVAL
    assert "CSR entry 1 is not positive" in _error(), _error()


# ---- a refused call leaves nothing behind ---------------------------------------------------------------------------------------------
def test_walk_prefix_after_refusal():
    bad = VAL3.copy()
    bad[0] = 0.0

    def valid():
        rc, cum = _walk_prefix(VAL3)
        assert rc == 0, _error()
        return [cum]

    _valid_refused_valid(valid, (lambda: _walk_prefix(bad)[0], "CSR entry 0"))


def test_resample_stats_after_refusal():
    lib, S, n, count = _lib.load(), 2, 5, 3
    host = np.arange(S * n, dtype=np.float64).reshape(S, n) * 0.375 - 1.0
    good = _dev(host)
    host[1, 3] = math.nan
    bad = _dev(host)

    def run(v):
        out = torch.full((count, S, 2), -7.0, dtype=torch.float64, device="cuda")
        rc = lib.gss_resample_stats(_lib.ptr(v), n, S, n, 1, 12345, 0, count, _lib.ptr(out), _lib.current_stream())
        return rc, out.cpu()

    def valid():
        rc, out = run(good)
        assert rc == 0, _error()
        return [out]

    _valid_refused_valid(valid, (lambda: run(bad)[0], "series 1, position 3: the value is NaN or infinite"))


def test_embedding_scores_after_refusal():
    lib, n, d = _lib.load(), 4, 3
    host = (np.arange(n * d, dtype=np.float32).reshape(n, d) - 4.0) * 0.5
    emb = _dev(host)
    host[2, 1] = math.inf
    emb_inf = _dev(host)
    rows, cols = _dev(np.array([0, 2], np.int32)), _dev(np.array([3, 1], np.int32))
    rows_bad = _dev(np.array([0, 4], np.int32))

    def run(e, r):
        out = torch.full((2, 2), -7.0, dtype=torch.float64, device="cuda")
        rc = lib.gss_embedding_scores(n, d, _lib.ptr(e), d, 2, _lib.ptr(r), 2, _lib.ptr(cols), 1, _lib.ptr(out), 2, _lib.current_stream())
        return rc, out.cpu()

    def valid():
        rc, out = run(emb, rows)
        assert rc == 0, _error()
        return [out]

    _valid_refused_valid(valid, (lambda: run(emb, rows_bad)[0], "rows[1] = 4 is not a row index in [0, 4)"),
                         (lambda: run(emb_inf, rows)[0], "row 2 of emb holds a NaN or infinite value"))


def test_pair_sums_lists_after_refusal():
    lib, n = _lib.load(), 4
    d = _dev(np.arange(n * n, dtype=np.float64).reshape(n, n) * 0.25)
    ptr = _dev(np.array([0, 2, 4], np.int32))
    idx, idx_bad = _dev(np.array([0, 1, 2, 3], np.int32)), _dev(np.array([0, 1, 4, 3], np.int32))

    def run(i):
        out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
        rc = lib.gss_pair_sums_lists(n, _lib.ptr(d), n, 2, _lib.ptr(ptr), _lib.ptr(i), _lib.ptr(out), _lib.current_stream())
        return rc, out.cpu()

    def valid():
        rc, out = run(idx)
        assert rc == 0, _error()
        return [out]

    _valid_refused_valid(valid, (lambda: run(idx_bad)[0], "idx[2] = 4 is outside [0, n=4)"))


def test_profile_dist_after_refusal():
    lib, n, ld = _lib.load(), 3, 4
    x = _dev((np.arange(n * ld, dtype=np.float64).reshape(n, ld) % 5) + 0.5)
    a, b, b_bad = _dev(np.array([0, 1], np.int32)), _dev(np.array([2, 3], np.int32)), _dev(np.array([2, 4], np.int32))

    def run(cb):
        out = torch.full((2, 2), -7.0, dtype=torch.float64, device="cuda")
        rc = lib.gss_profile_dist(n, _lib.ptr(x), ld, 2, _lib.ptr(a), 2, _lib.ptr(cb), 3, _lib.ptr(out), 2, _lib.current_stream())
        torch.cuda.current_stream().synchronize()
        return rc, out.cpu()

    def valid():
        rc, out = run(b)
        assert rc == 0, _error()
        return [out]

    _valid_refused_valid(valid, (lambda: run(b_bad)[0], "cols_b[1] = 4 is outside [0, ld=4)"))


def test_profile_topk_after_refusal():
    lib, n, k = _lib.load(), 8, 2
    x = _dev(np.array([3.0, 1.0, 4.0, 1.5, 5.0, 9.0, 2.0, 6.0]).reshape(n, 1))
    need = int(lib.gss_profile_topk_workspace_bytes(n, 1, 1, k))
    assert need > 0
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device="cuda")
    col, col_bad = _dev(np.array([0], np.int32)), _dev(np.array([1], np.int32))

    def run(c):
        idx = torch.full((1, 1, k), -7, dtype=torch.int32, device="cuda")
        val = torch.full((1, 1, k), -7.0, dtype=torch.float64, device="cuda")
        cnt = torch.full((1, 1), -7, dtype=torch.int32, device="cuda")
        rc = lib.gss_profile_topk(n, _lib.ptr(x), 1, 1, _lib.ptr(c), 1, None, k, _lib.ptr(idx), _lib.ptr(val), _lib.ptr(cnt), _lib.ptr(ws), need,
                                  _lib.current_stream())
        return rc, [idx.cpu(), val.cpu(), cnt.cpu()]

    def valid():
        rc, out = run(col)
        assert rc == 0, _error()
        return out

    _valid_refused_valid(valid, (lambda: run(col_bad)[0], "cols[0] = 1 is outside [0, ld=1)"))
    assert valid()[0].flatten().tolist() == [5, 7]


PATH4_ROWPTR = np.array([0, 1, 3, 5, 6], np.int32)   # the path 0 - 1 - 2 - 3, both directions
PATH4_COL = np.array([1, 0, 2, 1, 3, 2], np.int32)


def test_prox_random_sets_after_refusal():
    lib, n = _lib.load(), 4
    rowptr, col = _dev(PATH4_ROWPTR), _dev(PATH4_COL)
    st = _lib.current_stream()
    h = C.c_void_p()
    assert lib.gss_prox_create(C.byref(h), n, _lib.ptr(rowptr), _lib.ptr(col), 1 << 20, st) == 0, _error()
    try:
        set_ptr = _dev(np.array([0, 2], np.int32))
        members, members_bad = _dev(np.array([0, 2], np.int32)), _dev(np.array([0, 4], np.int32))
        node_bin, bin_ptr, bin_nodes = _dev(np.zeros(n, np.int32)), _dev(np.array([0, n], np.int32)), _dev(np.arange(n, dtype=np.int32))
        n_random, max_size = 2, 2

        def run(m):
            nodes = torch.full((1, n_random + 1, max_size), -1, dtype=torch.int32, device="cuda")
            sizes = torch.full((1, n_random + 1), -7, dtype=torch.int32, device="cuda")
            rc = lib.gss_prox_random_sets(h, 0, 1, _lib.ptr(set_ptr), _lib.ptr(m), max_size, _lib.ptr(node_bin), _lib.ptr(bin_ptr),
                                          _lib.ptr(bin_nodes), n_random, 99, _lib.ptr(nodes), _lib.ptr(sizes), st)
            return rc, [nodes.cpu(), sizes.cpu()]

        def valid():
            rc, out = run(members)
            assert rc == 0, _error()
            return out

        _valid_refused_valid(valid, (lambda: run(members_bad)[0], "a set member is not a node index in [0, 4)"))
    finally:
        lib.gss_prox_destroy(h)


def test_paths_run_and_count_after_refusal():
    lib, n, q = _lib.load(), 4, 1
    st = _lib.current_stream()
    h = C.c_void_p()
    assert lib.gss_paths_create(C.byref(h), n, len(PATH4_COL), PATH4_ROWPTR.ctypes.data, PATH4_COL.ctypes.data, 0, 1 << 20, st) == 0, _error()
    try:
        targets = np.array([0], np.int32)
        dist = torch.full((q, n), 77, dtype=torch.uint8, device="cuda")
        nxt = torch.full((q, n), -7, dtype=torch.int32, device="cuda")
        sigma = torch.full((q, n), -7.0, dtype=torch.float64, device="cuda")
        lv = C.c_int32(-1)

        def count(levels):
            return lib.gss_paths_count(h, q, targets.ctypes.data, _lib.ptr(dist), levels, None, _lib.ptr(sigma), None, None, st)

        def valid():
            dist.fill_(77), nxt.fill_(-7), sigma.fill_(-7.0)
            assert lib.gss_paths_run(h, q, targets.ctypes.data, _lib.ptr(dist), _lib.ptr(nxt), C.byref(lv), st) == 0, _error()
            assert lv.value == 3
            assert count(lv.value) == 0, _error()
            return [dist.cpu(), nxt.cpu(), sigma.cpu()]

        _valid_refused_valid(valid, (lambda: count(2), "levels=2 is smaller than the distance of node 3 from target 0 (node 0)"))
        d, nx, s = valid()
        assert d.flatten().tolist() == [0, 1, 2, 3] and s.flatten().tolist() == [1.0, 1.0, 1.0, 1.0]
        assert nx.flatten().tolist()[1:] == [0, 1, 2]
    finally:
        lib.gss_paths_destroy(h)
