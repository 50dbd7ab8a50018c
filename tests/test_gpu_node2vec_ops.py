"""-m gpu: the node2vec kernels (csrc/walk.hip, csrc/sgns.hip) op by op against tests/node2vec_mirror.py on the inputs of
tests/node2vec_cases.py, through the C entry points (gss_walk_prefix, gss_node2vec_walks, gss_sgns_counts, gss_sgns_epoch).  What these
inputs are for, and that a wrong rule cannot hide behind the bounds used here, is established on the CPU in
tests/test_node2vec_mirror.py.

Walks: bit for bit the mirror's, lengths included, twice -- the direct draw after 64 refused candidates (never reached by
tests/test_gpu_node2vec.py), prefix sums with ties, walk lengths 1 and 2, 255 / 256 / 257 walks, a graph of one node with and without
an edge.  Outputs lie between guard rows that must stay untouched.

SGNS, serial (concurrency 1): every case against the fp64 mirror run from the same state and tables, within MARGIN x d32(case), d32 =
max |fp32 mirror - fp64 mirror| computed here from the two mirrors (never from the device).  MARGIN = 8: the kernel and numpy's fp32 do
the same fp32 operations and differ in summation order, fma contraction and expf's last bit, so their distances to fp64 are of one
order.  Measured err / d32 per case (MI355X):
    dims_64 1.16   dims_128 1.00   dims_256 1.04   dims_512 1.06   long_80 0.91   long_130 1.10   window_1 0.85
    window_wider_than_sentence 1.08   negative_1 1.00   negative_63 0.95   f_skip 1.00   keep_boundary 1.06   table_ties 1.00
    epochs_3_e0 1.11   epochs_3_e1 1.01   epochs_3_e2 1.00   min_alpha_clamp 0.93   degenerate_sentences 1.00   partition 0.96
with d32 between 1.4e-7 and 2.4e-6 (1.7e-9 on `partition`) and every case's state moved by 1.8e-2 to 7.3e-1; the wrong rules of
node2vec_mirror.ABLATIONS sit 4.6e4 to 4.0e5 x d32 away.  A ratio of 1.00 is a case whose largest error the device shares with the fp32
mirror to the bit.  All 15 walk cases came out equal to the mirror on the first run: neither the kernels nor the mirror needed a change.
Sentence partition: the `partition` case at concurrency 1, 3, 7, 4096, the library's default and S + 5 gives the same bits.
Counts: gss_sgns_counts adds np.bincount of the valid tokens to what the buffer held.

No test provokes a fault: every launch gets valid arguments (token ids and table entries are checked where the cases are built)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import node2vec_cases as K  # noqa: E402
import node2vec_mirror as M  # noqa: E402
from conftest import record_measured  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
MARGIN = 8
GUARD = 3                    # guard rows before and after every output
SENTINEL = -77


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def at_least_one(x):
    """an empty CSR still hands the entry point non-null arrays"""
    return x if len(x) else np.zeros(1, x.dtype)


def device_walks(name):
    """-> (walks, lengths, prefix sums) of the case; the guard rows around both outputs are checked here"""
    c = K.walk_case(name)
    a = M.csr(c.adj())
    n, nnz = a.shape[0], a.nnz
    lib = _lib.load()
    stream = _lib.current_stream()
    rowptr = torch.from_numpy(a.indptr.astype(np.int32)).cuda()
    col = torch.from_numpy(at_least_one(a.indices.astype(np.int32))).cuda()
    val = torch.from_numpy(at_least_one(a.data.astype(np.float64))).cuda()
    cum = torch.full((max(nnz, 1),), float("nan"), dtype=torch.float64, device="cuda")
    starts = torch.from_numpy(M.start_nodes(n, c.nw, c.seed).astype(np.int32)).cuda()
    W = n * c.nw
    wbuf = torch.full((W + 2 * GUARD, c.L), SENTINEL, dtype=torch.int32, device="cuda")
    lbuf = torch.full((W + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    if nnz:
        _lib.check(lib.gss_walk_prefix(n, _lib.ptr(rowptr), _lib.ptr(val), _lib.ptr(cum), stream), "gss_walk_prefix")
    _lib.check(lib.gss_node2vec_walks(n, _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(cum), W, _lib.ptr(starts), c.L,
                                      float(c.p), float(c.q), c.seed, _lib.ptr(wbuf[GUARD:]), _lib.ptr(lbuf[GUARD:]), stream),
               "gss_node2vec_walks")
    torch.cuda.synchronize()
    w, ln = wbuf.cpu().numpy(), lbuf.cpu().numpy()
    for buf in (w, ln):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + W:] == SENTINEL).all(), name
    return w[GUARD:GUARD + W], ln[GUARD:GUARD + W], cum.cpu().numpy()[:nnz]


@pytest.mark.parametrize("name", K.WALK_CASES)
def test_walks_equal_the_mirror_bit_for_bit(name):
    c = K.walk_case(name)
    mw, ml, stats = K.mirror_walks(name)
    w, ln, cum = device_walks(name)
    assert np.array_equal(bits(cum), bits(M.row_prefix(M.csr(c.adj()))))
    bad = np.flatnonzero((w != mw).any(axis=1))
    print(f"{name}: {len(w)} walks of {c.L}, {stats['direct_draws']} direct draws, {stats['prefix_ties']} tie probes, {len(bad)} walks differ")
    assert np.array_equal(ln, ml), np.flatnonzero(ln != ml)[:5]
    assert len(bad) == 0, (bad[:5], w[bad[:2]], mw[bad[:2]])
    past = np.arange(c.L)[None, :] >= ln[:, None]
    assert (w[past] == -1).all() and (w[~past] >= 0).all()
    w2, ln2, _ = device_walks(name)
    assert np.array_equal(w2, w) and np.array_equal(ln2, ln)


_device = {}


def device_epoch(name, concurrency=1):
    """the case's one epoch on the device from its start state -> (syn0, syn1neg); computed once per (case, concurrency)"""
    key = (name, concurrency)
    if key in _device:
        return _device[key]
    c = K.sgns_case(name)
    lib = _lib.load()
    S, L = c.walks.shape
    walks = torch.from_numpy(c.walks).cuda()
    lengths = torch.from_numpy(c.lengths).cuda()
    cum = torch.from_numpy(c.cum_table.view(np.int32)).cuda()
    keep = torch.from_numpy(c.sample_int).cuda()
    state = []
    for rows in (c.syn0, c.syn1):
        buf = torch.full((c.n + 2 * GUARD, c.d), float("nan"), dtype=torch.float32, device="cuda")
        buf[GUARD:GUARD + c.n] = torch.from_numpy(rows).cuda()
        state.append(buf)
    desc = _lib.SgnsDesc(n=c.n, d=c.d, walk_length=L, window=c.window, negative=c.negative, epochs=c.epochs, n_walks=S, walks=_lib.ptr(walks),
                         lengths=_lib.ptr(lengths), cum_table=_lib.ptr(cum), sample_int=_lib.ptr(keep), cum_last=int(c.cum_table[-1]),
                         alpha=c.alpha, min_alpha=c.min_alpha, seed=c.seed, concurrency=int(concurrency))
    _lib.check(lib.gss_sgns_epoch(desc, c.first_epoch, _lib.ptr(state[0][GUARD:]), _lib.ptr(state[1][GUARD:]), _lib.current_stream()),
               "gss_sgns_epoch")
    torch.cuda.synchronize()
    out = []
    for buf in state:
        h = buf.cpu().numpy()
        assert np.isnan(h[:GUARD]).all() and np.isnan(h[GUARD + c.n:]).all(), name
        out.append(h[GUARD:GUARD + c.n])
    assert np.array_equal(walks.cpu().numpy(), c.walks) and np.array_equal(keep.cpu().numpy(), c.sample_int)      # inputs left alone
    _device[key] = tuple(out)
    return _device[key]


def distance(name, got):
    """max |device - fp64 mirror| over syn0 and syn1neg"""
    m0, m1, _ = K.sgns_mirror(name, np.float64)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    return float(max(np.abs(got[0] - m0).max(), np.abs(got[1] - m1).max()))


@pytest.mark.parametrize("name", K.SERIAL_CASES)
def test_sgns_serial_epoch_against_the_fp64_mirror(name):
    c = K.sgns_case(name)
    unit = K.d32(name)
    got = device_epoch(name)
    err = distance(name, got)
    moved = float(max(np.abs(got[0] - c.syn0).max(), np.abs(got[1] - c.syn1).max()))
    record_measured("sgns_op_vs_fp64", **{name: err / unit})
    print(f"{name}: max |device - fp64 mirror| {err:.3e} = {err / unit:.2f} x d32 ({unit:.3e}); moved {moved:.3e}")
    assert err <= MARGIN * unit, (name, err, unit, err / unit)
    assert moved >= c.moved_min
    if name == "keep_boundary":
        m0, m1, _ = K.sgns_mirror(name, np.float64)
        assert not np.array_equal(bits(got[0][c.v]), bits(c.syn0[c.v])) and not np.array_equal(bits(got[1][c.v]), bits(c.syn1[c.v]))
        assert np.array_equal(bits(got[0][c.u]), bits(c.syn0[c.u]))
        if np.array_equal(m1[c.u], c.syn1[c.u].astype(np.float64)):            # no negative drew u
            assert np.array_equal(bits(got[1][c.u]), bits(c.syn1[c.u]))
    if name == "partition":
        assert np.array_equal(bits(got[1]), bits(c.syn1))                       # every l1 read is zero: no syn1neg row changes


def test_sgns_sentence_partition_gives_the_same_bits_at_every_concurrency():
    S = K.PARTITION_S
    unit = K.d32("partition")
    default = _lib.load().gss_sgns_default_concurrency()
    assert default >= 1
    serial = device_epoch("partition", 1)
    assert distance("partition", serial) <= MARGIN * unit
    for conc in (3, 7, 4096, default, S + 5):
        got = device_epoch("partition", conc)
        same = np.array_equal(bits(got[0]), bits(serial[0])) and np.array_equal(bits(got[1]), bits(serial[1]))
        print(f"concurrency {conc}: same bits {same}, max |device - fp64 mirror| {distance('partition', got):.3e} (bound {MARGIN * unit:.3e})")
        assert same, (conc, np.flatnonzero((got[0] != serial[0]).any(axis=1))[:5])
        assert distance("partition", got) <= MARGIN * unit


def test_sgns_counts_add_the_valid_tokens_to_the_buffer():
    w, ln, n = K.counts_case()
    valid = np.arange(w.shape[1])[None, :] < ln[:, None]
    want = np.bincount(w[valid], minlength=n).astype(np.int64)
    lib = _lib.load()
    walks, lengths = torch.from_numpy(w).cuda(), torch.from_numpy(ln).cuda()
    held = np.arange(n, dtype=np.int64) * 1000 + 5
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    buf[GUARD:GUARD + n] = torch.from_numpy(held).cuda()
    for times in (1, 2):
        _lib.check(lib.gss_sgns_counts(w.shape[0], w.shape[1], _lib.ptr(walks), _lib.ptr(lengths), _lib.ptr(buf[GUARD:]), _lib.current_stream()),
                   "gss_sgns_counts")
        torch.cuda.synchronize()
        h = buf.cpu().numpy()
        assert (h[:GUARD] == SENTINEL).all() and (h[GUARD + n:] == SENTINEL).all()
        assert np.array_equal(h[GUARD:GUARD + n], held + times * want), np.flatnonzero(h[GUARD:GUARD + n] != held + times * want)
    assert want.sum() == ln.sum() and (want == 0).sum() == 1
