"""-m gpu: the five kernels of csrc/proximity.hip op by op against tests/proximity_mirror.py on the inputs of tests/proximity_cases.py,
through the C entry points (gss_prox_create, gss_prox_random_sets, gss_prox_set_stats, gss_prox_score with a hand-built ProxSets).
What these inputs are for, and that a wrong rule cannot hide behind the comparisons used here, is established on the CPU in
tests/test_proximity_mirror.py.  No test loads the 2016 fixture; the largest input is the 4,100-node graph of the ns = 4096 case.

Bit for bit (np.array_equal on the raw bits): the distance bytes and the diameter; the random-set nodes and sizes; centres, n_centres
and inner; d and m of closest, shortest, center and separation (integer sums divided once; m summed in sample order).
Toleranced, against stats_sequential of the mirror's values, with the tolerances of test_gpu_proximity.py::test_statistics_equal_mirror
(TOL_REL = 1e-12 relative, or 1e-12 absolute; 1e-11 absolute on z), never tuned to the device: s, z and pval of every measure and all
five fields of `kernel`.  Measured maxima per case (MI355X), relative for d / m / s / pval, absolute for z; the last column is the
largest error as a share of its tolerance:
                      integer measures                   kernel measure
    case              s        z        pval             d        m        s        z        pval        error / tolerance
    grid              1.9e-16  2.2e-16  1.8e-15          6.6e-16  5.0e-16  4.8e-14  2.2e-13  5.5e-14     0.022
    grid_all          0        0        3.1e-14          1.7e-16  3.4e-16  2.1e-15  9.9e-14  5.2e-13     0.0099
    pairs_unordered   1.5e-16  2.2e-16  5.5e-16          (all five of kernel <= 6.9e-15, its z 2.2e-13)  0.022
    lds_4096          0        0        2.5e-15          0        0        2.3e-14  5.6e-14  1.6e-13     0.0056
    exhaust           1.9e-16  8.9e-16  3.1e-15          3.4e-16  2.1e-16  4.0e-15  7.7e-14  1.2e-13     0.019
    empties           0        0        3.1e-14          1.7e-16  3.4e-16  4.4e-14  5.6e-14  2.0e-13     0.0056
    sd0               0        0        0                (kernel not asked for: 0)                       0
    batch7            1.9e-16  2.2e-16  1.0e-15          1.7e-16  1.7e-16  4.8e-14  1.2e-13  5.5e-14     0.012
    exhaust_chain     the figures of `exhaust`: the chained device ops give its bits
(in the lower tail a pval's relative error is about |z| times the absolute error of z; pvals that small are held by the absolute
1e-12, which is why the last column stays at z's share).  All 30 tests came out equal to the mirror on
the first run: neither the kernels nor the mirror needed a change.
Every output buffer lies between guard rows that must come back untouched, and entries of a row past sizes / n_centres must still be
the sentinel.  Each op is run twice and must give the same bits.  The score kernel is handed the MIRROR's tables and set statistics, so
a failure names one kernel; one test chains the three device ops on the `exhaust` sets.

No test provokes a fault: the refusals below are host-side argument checks that launch nothing, except a set longer than max_size,
which random_sets_kernel flags without writing the row."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proximity_cases as K  # noqa: E402
import proximity_mirror as M  # noqa: E402
from conftest import record_measured  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 3                    # guard rows before and after every output
SENT = -77                   # sentinel of the integer outputs; -77.0 of the fp64 ones
EINVAL = -22
TOL_REL, TOL_ABS, TOL_ABS_Z = 1e-12, 1e-12, 1e-11
EXACT = (0, 1, 3, 4)         # closest, shortest, center, separation: d and m bit for bit
KERNEL = 2
ALL_MASK = 31


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _error():
    return _lib.load().gss_last_error().decode()


def _valid_refused_valid(valid, *refused):
    """valid() -> host arrays of a call that succeeds; each of refused is (call -> rc, words of the refusal)"""
    kept = valid()
    for call, words in refused:
        assert call() == EINVAL, words
        assert words in _error(), _error()
        again = valid()
        assert len(again) == len(kept)
        for a, b in zip(again, kept):
            assert a.dtype == b.dtype and np.array_equal(bits(a), bits(b)), words


def guarded(rows, shape, dtype):
    """a device buffer of `rows` rows of `shape` between GUARD sentinel rows on either side"""
    return torch.full((rows + 2 * GUARD,) + tuple(shape), SENT, dtype=dtype, device="cuda")


def inside(buf, rows):
    """host copy of the rows between the guards; the guards are checked"""
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENT).all() and (h[GUARD + rows:] == SENT).all(), "a guard row was written"
    return h[GUARD:GUARD + rows]


# ---- handles: one per graph, made on first use ---------------------------------------------------------------------------------------

_handles = {}


def create(name):
    """-> (rc, handle, kept-alive inputs)"""
    g = K.graph(name)
    rowptr, col = _dev(g.rowptr), _dev(g.col if len(g.col) else np.zeros(1, np.int32))
    h = C.c_void_p()
    rc = _lib.load().gss_prox_create(C.byref(h), g.n, _lib.ptr(rowptr), _lib.ptr(col), 1 << 30, _lib.current_stream())
    return rc, h, (rowptr, col)


def handle(name):
    if name not in _handles:
        rc, h, keep = create(name)
        assert rc == 0, _error()
        _handles[name] = (h, keep)
    return _handles[name][0]


@pytest.fixture(scope="module", autouse=True)
def _destroy_handles():
    yield
    for h, _ in _handles.values():
        _lib.load().gss_prox_destroy(h)
    _handles.clear()


def device_distances(h, n):
    lib = _lib.load()
    buf = torch.full((n + 2 * GUARD, n), 7, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gss_memcpy_d2d(_lib.ptr(buf[GUARD:]), lib.gss_prox_distances(h), n * n, _lib.current_stream()), "gss_memcpy_d2d")
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == 7).all() and (host[GUARD + n:] == 7).all()
    return host[GUARD:GUARD + n]


# ---- apsp_kernel ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.APSP_CASES)
def test_distances_and_diameter_equal_bfs(name):
    g, want = K.graph(name), K.distances(name)
    lib = _lib.load()
    got = device_distances(handle(name), g.n)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert lib.gss_prox_diameter(handle(name)) == K.diameter(name)
    if name.startswith("split_"):
        assert (got[np.ix_(g.parts[0], g.parts[1])] == 255).all() and K.diameter(name) == int(want[want != 255].max()) < 255
    if name == "path_255":
        assert got[0, 254] == got[254, 0] == 254 and lib.gss_prox_diameter(handle(name)) == 254
    rc, h2, _keep = create(name)                                   # a second run: the same bytes
    assert rc == 0, _error()
    try:
        assert np.array_equal(device_distances(h2, g.n), got) and lib.gss_prox_diameter(h2) == K.diameter(name)
    finally:
        lib.gss_prox_destroy(h2)


def test_path_of_256_nodes_is_refused_and_255_still_runs():
    def valid():
        rc, h, _keep = create("path_255")
        assert rc == 0, _error()
        try:
            return [device_distances(h, 255), np.array([_lib.load().gss_prox_diameter(h)])]
        finally:
            _lib.load().gss_prox_destroy(h)

    def refused():
        rc, h, _keep = create(K.APSP_REFUSED)
        assert not h.value
        return rc

    _valid_refused_valid(valid, (refused, "255 or more hops"))


# ---- random_sets_kernel -----------------------------------------------------------------------------------------------------------------

def device_random(name, side, max_size=None, n_random=None):
    """-> (rc, nodes [n_sets, R, max_size], sizes [n_sets, R]); rows past their size hold SENT"""
    c = K.random_case(name)
    lib, h = _lib.load(), handle(c.graph)
    max_size = max_size or c.max_size
    n_random = c.n_random if n_random is None else n_random
    ptr = np.zeros(len(c.sets) + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in c.sets])
    flat = np.concatenate(list(c.sets) + [np.zeros(1, np.int64)]).astype(np.int32)
    bin_ptr = np.zeros(len(c.bin_list) + 1, np.int32)
    bin_ptr[1:] = np.cumsum([len(b) for b in c.bin_list])
    d = [_dev(x) for x in (ptr, flat, c.node_bin.astype(np.int32), bin_ptr, np.concatenate(c.bin_list).astype(np.int32))]
    R = n_random + 1
    U = len(c.sets) * R
    nodes, sizes = guarded(U, (max_size,), torch.int32), guarded(U, (), torch.int32)
    rc = lib.gss_prox_random_sets(h, side, len(c.sets), _lib.ptr(d[0]), _lib.ptr(d[1]), max_size, _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]),
                                  n_random, c.seed, _lib.ptr(nodes[GUARD:]), _lib.ptr(sizes[GUARD:]), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, inside(nodes, U).reshape(len(c.sets), R, max_size), inside(sizes, U).reshape(len(c.sets), R)


@pytest.mark.parametrize("name", K.RANDOM_CASES)
def test_random_sets_equal_the_mirror_bit_for_bit(name):
    c = K.random_case(name)
    got = {}
    for side in (0, 1):
        want_nodes, want_sizes = K.table_arrays(K.random_table(name, side), c.max_size, pad=SENT)
        rc, nodes, sizes = device_random(name, side)
        assert rc == 0, _error()
        assert np.array_equal(sizes, want_sizes), (side, np.argwhere(sizes != want_sizes)[:5])
        assert np.array_equal(nodes, want_nodes), (side, np.argwhere(nodes != want_nodes)[:5])        # SENT past every size
        rc, nodes2, sizes2 = device_random(name, side)
        assert rc == 0 and np.array_equal(nodes2, nodes) and np.array_equal(sizes2, sizes)
        got[side] = nodes
    if c.n_random:
        assert not np.array_equal(got[0][:, 1:], got[1][:, 1:])                                       # the sides draw differently
    assert np.array_equal(got[0][:, 0], got[1][:, 0])
    if name == "exhaust":
        assert sizes[0].min() < 32 and (sizes[0][1:] == 32).any()


def test_random_sets_wider_rows_keep_their_padding():
    """max_size above every size: the same sets, the rest of every row untouched"""
    c = K.random_case("mixed")
    want_nodes, want_sizes = K.table_arrays(K.random_table("mixed", 0), c.max_size + 5, pad=SENT)
    rc, nodes, sizes = device_random("mixed", 0, max_size=c.max_size + 5)
    assert rc == 0, _error()
    assert np.array_equal(nodes, want_nodes) and np.array_equal(sizes, want_sizes)


def test_random_sets_refuse_a_set_longer_than_max_size():
    c = K.random_case("mixed")
    assert max(len(s) for s in c.sets) == c.max_size > 3

    def valid():
        rc, nodes, sizes = device_random("mixed", 0)
        assert rc == 0, _error()
        return [nodes, sizes]

    _valid_refused_valid(valid, (lambda: device_random("mixed", 0, max_size=c.max_size - 1)[0], f"a set has more than max_size={c.max_size - 1} members"))


# ---- set_stats_kernel -------------------------------------------------------------------------------------------------------------------

def device_set_stats(gname, nodes, sizes, centres=True):
    """nodes [n_sets, R, max_size], sizes [n_sets, R] host int32 -> inner [n_sets, R], centres like nodes (SENT where unwritten), n_centres"""
    lib, h = _lib.load(), handle(gname)
    n_sets, R, max_size = nodes.shape
    U = n_sets * R
    dn, ds = _dev(nodes.astype(np.int32)), _dev(sizes.astype(np.int32))
    inner = guarded(U, (), torch.float64)
    cen, ncen = guarded(U, (max_size,), torch.int32), guarded(U, (), torch.int32)
    rc = lib.gss_prox_set_stats(h, n_sets, R, max_size, _lib.ptr(dn), _lib.ptr(ds), _lib.ptr(inner[GUARD:]),
                                _lib.ptr(cen[GUARD:]) if centres else None, _lib.ptr(ncen[GUARD:]) if centres else None, _lib.current_stream())
    assert rc == 0, _error()
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy(), nodes) and np.array_equal(ds.cpu().numpy(), sizes)        # inputs left alone
    return inside(inner, U).reshape(n_sets, R), inside(cen, U).reshape(n_sets, R, max_size), inside(ncen, U).reshape(n_sets, R)


def stat_arrays(stats, max_size, pad=-1):
    """the mirror's stats table -> (inner [n_sets, R], centres [n_sets, R, max_size] padded, n_centres [n_sets, R])"""
    cen, ncen = K.table_arrays([[s[1] for s in rows] for rows in stats], max_size, pad)
    return np.array([[s[0] for s in rows] for rows in stats], np.float64), cen, ncen


@pytest.mark.parametrize("name", K.SET_CASES)
def test_set_stats_equal_the_mirror_bit_for_bit(name):
    c = K.set_case(name)
    table, max_size = K.set_table(name)
    nodes, sizes = K.table_arrays(table, max_size)                # padded with -1
    assert max_size > sizes.max()
    want_inner, want_cen, want_ncen = stat_arrays(K.set_mirror(name), max_size, pad=SENT)
    inner, cen, ncen = device_set_stats(c.graph, nodes, sizes)
    assert np.array_equal(ncen, want_ncen), (ncen, want_ncen)
    assert np.array_equal(cen, want_cen), np.argwhere(cen != want_cen)[:5]                            # SENT past n_centres
    assert np.array_equal(bits(inner), bits(want_inner)), (inner, want_inner)
    again = device_set_stats(c.graph, nodes, sizes)
    assert np.array_equal(bits(again[0]), bits(inner)) and np.array_equal(again[1], cen) and np.array_equal(again[2], ncen)
    alone, cen0, ncen0 = device_set_stats(c.graph, nodes, sizes, centres=False)                       # centres = NULL: the same inner,
    assert np.array_equal(bits(alone), bits(inner)) and (cen0 == SENT).all() and (ncen0 == SENT).all()   # no centre buffer touched
    if name == "cycle_tied":
        assert ncen[0, 0] == sizes[0, 0] == 150
    if name == "tie_63_64":
        assert ncen[0, 0] == 2 and cen[0, 0, :2].tolist() == [nodes[0, 0, 63], nodes[0, 0, 64]]
    if name == "sizes":
        assert sizes.ravel().tolist() == list(K.SET_SIZES) and inner.ravel()[0] == 0.0 and inner.ravel()[1] == 0.0 and ncen.ravel()[0] == 0


# ---- score_kernel + stats_kernel --------------------------------------------------------------------------------------------------------

def score_inputs(name):
    """the case's tables and the mirror's set statistics as host arrays: (from nodes, sizes, inner), (to nodes, sizes, inner, centres, n_centres)"""
    c = K.score_case(name)
    fs, ts = K.score_stats(name)
    fn, fz = K.table_arrays(c.ftab, c.from_max_size)
    tn, tz = K.table_arrays(c.ttab, c.to_max_size)
    ti, tc, tnc = stat_arrays(ts, c.to_max_size)
    return (fn, fz, stat_arrays(fs, c.from_max_size)[0]), (tn, tz, ti, tc, tnc)


def device_score(gname, F, T, n_samples, pairs, mask, n_pairs=None, centres=True, to_max_size=None, half_list=False):
    """-> (rc, out [n_pairs, 5, 5]); pairs None = all pairs"""
    lib, h = _lib.load(), handle(gname)
    df, dt = [_dev(x) for x in F], [_dev(x) for x in T]
    n_from, n_to = F[0].shape[0], T[0].shape[0]
    P = (n_from * n_to if pairs is None else len(pairs)) if n_pairs is None else n_pairs
    pf = pt = None
    if pairs is not None:
        pr = np.asarray(pairs, np.int32).reshape(-1, 2)
        assert pr[:, 0].max() < n_from and pr[:, 1].max() < n_to and pr.min() >= 0
        pf, pt = _dev(pr[:, 0].copy()), _dev(pr[:, 1].copy())
    fs = _lib.ProxSets(n_from, F[0].shape[2], _lib.ptr(df[0]), _lib.ptr(df[1]), _lib.ptr(df[2]), None, None)
    ts = _lib.ProxSets(n_to, to_max_size or T[0].shape[2], _lib.ptr(dt[0]), _lib.ptr(dt[1]), _lib.ptr(dt[2]), _lib.ptr(dt[3]) if centres else None,
                       _lib.ptr(dt[4]) if centres else None)
    out = guarded(max(P, 1), (5, 5), torch.float64)
    rc = lib.gss_prox_score(h, C.byref(fs), C.byref(ts), n_samples, P, _lib.ptr(pf), None if half_list else _lib.ptr(pt), mask, _lib.ptr(out[GUARD:]),
                            _lib.current_stream())
    torch.cuda.synchronize()
    return rc, inside(out, max(P, 1))[:P]


_scored = {}


def scored(name, mask=None):
    """the case on the device, once per (case, mask)"""
    c = K.score_case(name)
    mask = sum(K.MASK[m] for m in c.which) if mask is None else mask
    if (name, mask) not in _scored:
        F, T = score_inputs(name)
        rc, out = device_score(c.graph, F, T, c.n_samples, c.pairs, mask)
        assert rc == 0, _error()
        _scored[name, mask] = out
    return _scored[name, mask]


def compare(name, got, want, measures, label=None):
    """d and m of the integer measures bit for bit, the rest within the tolerances; -> the measured maxima"""
    assert got.shape == want.shape
    nan = np.isnan(want[:, 0, 0])
    assert np.isnan(got[nan]).all() and np.array_equal(np.isnan(got[~nan]), np.isnan(want[~nan]))
    got, want = got[~nan], want[~nan]
    worst = dict.fromkeys(("s_rel", "z_abs", "pval_rel", "kernel_d_rel", "kernel_m_rel", "kernel_s_rel", "kernel_z_abs", "kernel_pval_rel",
                           "of_tolerance"), 0.0)
    for k, m in enumerate(M.MEASURES):
        if m not in measures:
            continue
        fields = {"s": 2, "z": 3, "pval": 4}
        if k in EXACT:
            for f in (0, 1):
                assert np.array_equal(bits(got[:, k, f]), bits(want[:, k, f])), (name, m, "dm"[f], got[:, k, f], want[:, k, f])
        else:
            fields.update(d=0, m=1)
        for fname, f in fields.items():
            g, w = got[:, k, f], want[:, k, f]
            err = np.abs(g - w)
            tol = np.maximum(TOL_REL * np.abs(w), TOL_ABS_Z if fname == "z" else TOL_ABS)
            rel = float(np.max(err / np.where(w == 0, 1.0, np.abs(w)), initial=0.0))
            key = ("kernel_" if k == KERNEL else "") + ("z_abs" if fname == "z" else f"{fname}_rel")
            worst[key] = max(worst[key], float(err.max(initial=0.0)) if fname == "z" else rel)
            worst["of_tolerance"] = max(worst["of_tolerance"], float(np.max(err / tol, initial=0.0)))
            assert (err <= tol).all(), (name, m, fname, int(np.argmax(err / tol)), g[np.argmax(err / tol)], w[np.argmax(err / tol)])
    print(f"{label or name}: " + "  ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    record_measured("prox_ops_vs_mirror", **{f"{label or name}_{k}": v for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("name", K.SCORE_CASES)
def test_score_equals_the_mirror(name):
    c = K.score_case(name)
    want = K.score_mirror(name)
    got = scored(name)
    compare(name, got, want, c.which)
    for k, m in enumerate(M.MEASURES):                            # unmasked measures are 0 (pval 0.5) where the pair is not NaN
        if m not in c.which:
            live = ~np.isnan(want[:, 0, 0])
            assert (got[live][:, k, :4] == 0).all() and (got[live][:, k, 4] == 0.5).all()
    F, T = score_inputs(name)
    rc, again = device_score(c.graph, F, T, c.n_samples, c.pairs, sum(K.MASK[m] for m in c.which))
    assert rc == 0 and np.array_equal(bits(again), bits(got))
    if name == "empties":
        nan_pair = np.array([i == 1 or j == 0 for i, j in K.pair_list(c)])
        assert np.isnan(got[nan_pair]).all() and got[nan_pair].size == 5 * 25 and np.isfinite(got[~nan_pair]).all()
    if name == "sd0":
        for k in EXACT:
            assert (got[:, k, 2] == 0).all() and (got[:, k, 3] == 0).all() and (got[:, k, 4] == 0.5).all()
        assert (got[:, [0, 1, 3], :2] == 1.0).all() and (got[:, 4, :2] == 0.0).all()
    if name == "pairs_unordered":
        assert np.array_equal(bits(got[0]), bits(got[2])) and not np.array_equal(bits(got[0]), bits(got[1]))
        grid = scored("grid")
        for q, pair in enumerate(c.pairs):                         # a pair's numbers do not depend on where it stands in the list
            if pair in K.GRID_PAIRS:
                assert np.array_equal(bits(got[q]), bits(grid[K.GRID_PAIRS.index(pair)]))


def test_each_measure_alone_gives_the_bits_of_the_all_measures_run():
    c = K.score_case("grid")
    everything = scored("grid")
    F, T = score_inputs("grid")
    for k, m in enumerate(M.MEASURES):
        rc, alone = device_score(c.graph, F, T, c.n_samples, c.pairs, 1 << k, centres=(m == "center"))
        assert rc == 0, _error()
        assert np.array_equal(bits(alone[:, k]), bits(everything[:, k])), m
        for j in (0, 1):                                           # closest and shortest always come out
            assert np.array_equal(bits(alone[:, j]), bits(everything[:, j])), (m, j)
        for j in (2, 3, 4):
            if j != k:
                assert (alone[:, j, :4] == 0).all() and (alone[:, j, 4] == 0.5).all(), (m, M.MEASURES[j])


def test_chain_of_the_three_ops_on_the_exhaust_sets():
    """random sets -> set stats -> score, device to device, against the mirror of the same chain"""
    c, rc_ = K.score_case("exhaust"), K.random_case("exhaust")
    keep = [0, 1, 3, 4]
    tabs = []
    for side in (0, 1):
        rc, nodes, sizes = device_random("exhaust", side)
        assert rc == 0, _error()
        nodes, sizes = np.ascontiguousarray(nodes[keep]), np.ascontiguousarray(sizes[keep])
        inner, cen, ncen = device_set_stats(rc_.graph, nodes, sizes)
        tabs.append((nodes, sizes, inner, cen, ncen))
    assert (tabs[0][1][:, 1:] != tabs[0][1][:, :1]).any()          # sizes that differ from sample 0's
    rc, got = device_score(c.graph, tabs[0][:3], tabs[1], c.n_samples, c.pairs, ALL_MASK)
    assert rc == 0, _error()
    compare("exhaust", got, K.score_mirror("exhaust"), c.which, label="exhaust_chain")
    assert np.array_equal(bits(got), bits(scored("exhaust")))


def test_batches_of_1_2_3_and_7_pairs_give_the_bits_of_one_batch():
    lib = _lib.load()
    c = K.score_case("batch7")
    F, T = score_inputs("batch7")
    assert len(c.pairs) == 7
    default = scored("batch7")                                     # against the mirror in test_score_equals_the_mirror[batch7]
    try:
        for batch in (1, 2, 3, 7):
            assert lib.gss_debug_set_option(b"prox_batch_pairs", batch) == 0, _error()
            rc, got = device_score(c.graph, F, T, c.n_samples, c.pairs, ALL_MASK)
            assert rc == 0, _error()
            assert np.array_equal(bits(got), bits(default)), batch
    finally:
        assert lib.gss_debug_set_option(b"prox_batch_pairs", 0) == 0
    rc, got = device_score(c.graph, F, T, c.n_samples, c.pairs, ALL_MASK)
    assert rc == 0 and np.array_equal(bits(got), bits(default))


def test_score_refusals_by_name_leave_nothing_behind():
    c = K.score_case("grid_all")
    F, T = score_inputs("grid_all")
    n_all = len(K.pair_list(c))
    some = K.pair_list(c)[:4]

    def run(**kw):
        args = dict(n_samples=c.n_samples, pairs=None, mask=ALL_MASK)
        args.update(kw)
        return device_score(c.graph, F, T, args.pop("n_samples"), args.pop("pairs"), args.pop("mask"), **args)

    def valid():
        rc, out = run()
        assert rc == 0, _error()
        return [out]

    _valid_refused_valid(
        valid,
        (lambda: run(n_samples=2)[0], "n_samples=2: need the set itself and n_random >= 2 random samples"),
        (lambda: run(to_max_size=4097)[0], "to-sets of up to 4096 nodes are supported (max_size=4097)"),
        (lambda: run(mask=0)[0], "measures=0 must be a non-empty mask"),
        (lambda: run(mask=32)[0], "measures=32 must be a non-empty mask"),
        (lambda: run(mask=8, centres=False)[0], "center needs the to-sets' centres"),
        (lambda: run(pairs=some, half_list=True)[0], "pair_from and pair_to go together"),
        (lambda: run(n_pairs=n_all - 1)[0], f"without pair lists n_pairs must be n_from * n_to = {n_all}"))
    assert np.array_equal(bits(valid()[0]), bits(scored("grid_all")))
