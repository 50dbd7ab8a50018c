"""-m gpu: the three ops that run once before the first step, op by op through the C entry points, against tests/setup_ops_mirror.py on
the inputs of tests/setup_ops_cases.py: gss_percentile (csrc/percentile.hip), gss_knn_topk / gss_knn_topk_rows (csrc/knn.hip) and
gss_normalize_adj / gss_rowsum_dinv / gss_scale_adj_shard / gss_rowsum_check (the K11 block of csrc/spmm.hip).  That the mirrors are
right, that the inputs have the properties named here, and that they can tell the wrong rules below from the right one is established
on the CPU in tests/test_setup_ops_mirror.py.

Comparisons are bit equality, or a bound tests/test_gpu_ops.py already holds these ops to (tests/tolerances.py, SETUP_OPS_*): 2e-6 for
the percentile of inexact similarities, 1e-13 for row sums and D^-1/2, 1.2e-7 for A_hat against fp64.  Each test prints its worst figure
before it asserts.

Why each group is red if the code loses a rule (argued from csrc, not demonstrated on a GPU):
  percentile, exact inputs (bit for bit at level boundaries of inputs with tie groups of up to 1,978 entries)
    * `wgt` fixed at 1: an off-diagonal tile's entries count once, every cumulative count above the first such entry is short, and the
      histogram no longer sums to N^2 -- q = 100 finds no bin.  Fixed at 2: the diagonal tiles count twice, n <= 64 included.  Every
      percentile placed one entry before or at a boundary (pos = c - 1, c) then reads the neighbouring level; special_65 has exactly
      the 64 double-weight entries of one off-diagonal tile between its two boundaries.
    * the tile mask `i >= n || j >= n` dropped: rows past n are loaded clamped to row n - 1, so n = 63, 65, 129, 200 (and 1, 2, 3) count
      copies of the last row's similarities; counts shift at every boundary above them.
    * `rank + 1 >= eq_count` as `>`: never true (rank < eq_count), the min pass never runs, every midpoint and 3/4 point between two
      levels returns the lower level.  The same answers come from skipping the min pass, and from a floor taken as `>=`, which finds
      key_lo itself.  The percentiles at frac = 0 run the min pass and must NOT move: a min pass that returned a key other than the next
      level's moves the midpoints instead.  all_equal: the min pass finds nothing (got == init) and must leave key_hi = key_lo.
    * the shift or mask of pass 2 or 3 off by one bit: `adjacent` has 820 distinct keys under one first digit, in 88 second-digit
      prefixes and 365 third digits; a bit that belongs to no digit, or to two, merges or splits bins there and the final prefix is
      another float.  Several of its min passes cross a second-digit bin edge.
    * `ordered_key` without the sign flip: negative similarities sort above the positive ones and backwards; every lattice case with
      n >= 63 has 24 or more negative levels and one percentile whose lo is the largest negative level and hi the smallest non-negative.
  percentile, unit rows: the project's 2e-6, plus the rank of the returned value among the fp64 similarities -- a value that is close
    to SOME similarity but at the wrong rank (a count off by more than the values within 2e-6) is red.
  percentile, non-finite: a NaN, an inf or an fp32 overflow in E E^T must end in an error that names it.  Before this test the code
    returned GSS_OK on all three inputs, with a shifted level at q = 0, 50 and 98 and NaN at q = 100 (the figures are in
    tests/tolerances.py); the host now refuses when the first histogram has a count in the eight bins that only inf and NaN keys reach.
  kNN: the contract is a set property (indices distinct and in range, values are the similarities of their indices, the multiset of the
    k largest, nothing left out beats what is kept), because ties across the k-th place are arbitrary: `v > minv` as `>=` keeps other
    columns on the tied rows (at least a quarter of the rows of the d = 8 cases) and stays green, as it must.
    * `jmax` clamp dropped: the last tile's columns past n (clamped loads of row n - 1) enter as indices >= n -- "index out of [0, n)"
      at n = 1, 2, 63, 65, 130.
    * the `row_lo` offset dropped from the output index: a window writes at row i0 + t instead of i0 + t - row_lo -- outside the window's
      buffer (the canaries) for every window with row_lo > 0, and the window's own rows stay sentinel.
    * `row_lo` dropped from i0: the window holds the top-k of rows 0.., not of its own rows; the bit comparison with the whole table fails.
    * `i0 + threadIdx.x < row_hi` taken as `< n`: [63, 66) and [64, 65) write rows past the window -- the canaries.
  normalisation
    * the `+ lane` stride of rowsum_kernel / scale_kernel taken as 32: lanes 32..63 re-add entries, rows of 33 or more entries (63, 64,
      65, 129, 300) get a larger sum; at 128 entries past 64 are dropped.  Row sums are held to 1e-13.
    * the four-rows-per-block grid: n = 1, 3, 4, 5 and 257 leave one to three rows of the last block idle or put one row in a block of
      its own; a grid of n / 4 blocks loses rows 4.. at n = 5 (sentinel in the output), `row >= n` dropped writes past the outputs.
    * scale_shard_kernel reading dinv[row] for dinv[row0 + row], or the shard's row where the column belongs: other factors, other
      bits on every shard with row0 > 0 of the asymmetric matrix (transposed and not).  The ORDER of the two factors is not observable:
      tests/test_setup_ops_mirror.py shows that swapping them changes 561 fp64 products of this matrix and no fp32 result.
    * rowsum_check_kernel: the ballot's first lane reports popcount(m) -- a wave whose bad rows are lanes 63 or 0 only, bad rows in four
      waves of three blocks, every row bad; `!(x > 0)` as `x <= 0` loses the NaN rows, as `x < 0` the two zeros.
No test provokes a fault: every launch gets valid pointers and sizes; NaN and inf are data values.  The refusals are host-side checks
that launch nothing."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import setup_ops_cases as K  # noqa: E402
import setup_ops_mirror as M  # noqa: E402
import tolerances as T  # noqa: E402
from conftest import record_measured  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 257                    # canary elements before and after every output
SENT = -77                   # canary of the integer outputs; -77.25 of the floating ones
SENTF = -77.25
EINVAL = -22


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()           # a copy: the cases' arrays are read-only


def _error():
    return _lib.load().gss_last_error().decode(errors="replace")


def f32bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def f64bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Inside:
    """where the inside of a padded buffer starts (an empty torch view has no address; an empty output still gets a valid one)"""

    def __init__(self, buf):
        self.address = buf.data_ptr() + PAD * buf.element_size()

    def data_ptr(self):
        return self.address


def padded(count, dtype):
    """a device buffer of `count` elements between PAD canaries on either side -> (buffer, its inside)"""
    buf = torch.full((count + 2 * PAD,), SENT if dtype in (torch.int32, torch.int64) else SENTF, dtype=dtype, device="cuda")
    return buf, Inside(buf)


def inside(buf, count):
    """host copy of the inside; the canaries are checked"""
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    sent = SENT if h.dtype.kind == "i" else SENTF
    assert (h[:PAD] == sent).all() and (h[PAD + count:] == sent).all(), "a canary was written"
    return h[PAD:PAD + count]


# ---- gss_percentile -------------------------------------------------------------------------------------------------------------------

def device_percentile(e_dev, n, d, q):
    """-> (rc, float32 value); the output word holds a sentinel before the call"""
    out = C.c_float(SENTF)
    rc = _lib.load().gss_percentile(n, d, _lib.ptr(e_dev), float(q), C.byref(out), _lib.current_stream())
    return rc, np.float32(out.value)


@pytest.mark.parametrize("name", K.EXACT_CASES)
def test_percentile_of_exact_similarities_equals_the_mirror_bit_for_bit(name):
    e = K.pct_case(name)
    n, d = e.shape
    ed = _dev(e)
    want = K.pct_mirror(name)
    got = np.empty(len(want), np.float32)
    for t, q in enumerate(K.pct_qs(name)):
        rc, got[t] = device_percentile(ed, n, d, q)
        assert rc == 0, (name, q, _error())
    wrong = np.flatnonzero(f32bits(got) != f32bits(want))
    print(f"{name}: {len(want)} percentiles, {len(wrong)} differ from the mirror")
    record_measured("setup_ops_percentile_exact", **{f"{name}_differ": len(wrong)})
    labels = [w for _q, _lo, w in K.pct_plan(name)]
    assert len(wrong) == 0, [(labels[t], K.pct_qs(name)[t], float(got[t]), float(want[t])) for t in wrong[:6]]
    rc, again = device_percentile(ed, n, d, K.pct_qs(name)[0])                       # a second call: nothing of the first survives
    assert rc == 0 and f32bits(again) == f32bits(want[0])


@pytest.mark.parametrize("name", K.UNIT_CASES)
def test_percentile_of_unit_rows_within_2e6_and_at_the_right_rank(name):
    from test_setup_ops_mirror import rank_condition
    e = K.pct_case(name)
    n, d = e.shape
    ed = _dev(e)
    v = K.pct_sorted(name)
    worst, worst_rank = 0.0, 0.0
    for q in K.UNIT_QS:
        rc, got = device_percentile(ed, n, d, q)
        assert rc == 0, _error()
        err = abs(float(got) - np.percentile(v, q))
        print(f"{name} q={q}: |device - fp64| = {err:.3e} (bound {T.SETUP_OPS_PERCENTILE_ABS:g})")
        worst = max(worst, err)
        assert err < T.SETUP_OPS_PERCENTILE_ABS, (name, q, got)
        off, allow = rank_condition(v, n, q, got, T.SETUP_OPS_PERCENTILE_ABS)
        worst_rank = max(worst_rank, off / max(allow, 1))
    print(f"{name}: worst {worst:.3e}; rank off by at most {worst_rank:.2f} of its allowance")
    record_measured("setup_ops_percentile_unit", **{f"{name}_abs": worst, f"{name}_rank_share": worst_rank})


@pytest.mark.parametrize("name", K.NON_FINITE_CASES)
def test_percentile_refuses_non_finite_similarities_by_name(name):
    e = K.pct_case(name)
    n, d = e.shape
    ed = _dev(e)
    seen = []
    for q in K.NON_FINITE_QS:
        rc, got = device_percentile(ed, n, d, q)
        seen.append((q, rc, float(got), _error() if rc else ""))
        print(f"{name} q={q}: rc {rc}, value {got!r}, error {seen[-1][3]!r}")
    for q, rc, got, err in seen:
        assert rc != 0 and "non-finite similarit" in err, (name, q, rc, got, err)
        assert got == np.float32(SENTF), (name, q, got)                              # no value comes out beside the error
    finite = K.pct_case("lat_65_16")                                                 # the handle-free op holds no state: the next call is clean
    rc, got = device_percentile(_dev(finite), 65, 16, 50.0)
    assert rc == 0 and f32bits(got) == f32bits(M.percentile(finite, 50.0))


def test_percentile_refusals_by_name():
    e = _dev(K.pct_case("lat_65_16"))
    lib = _lib.load()
    out = C.c_float(SENTF)
    for args, words in (((65, 24, _lib.ptr(e), 50.0), "d=24 unsupported"), ((65, 16, _lib.ptr(e), 100.5), "q=100.5 outside [0, 100]"),
                        ((65, 16, _lib.ptr(e), -1.0), "q=-1 outside [0, 100]"), ((0, 16, _lib.ptr(e), 50.0), "null operand")):
        assert lib.gss_percentile(*args, C.byref(out), _lib.current_stream()) == EINVAL, words
        assert words in _error(), _error()
        assert out.value == SENTF


# ---- gss_knn_topk / gss_knn_topk_rows -------------------------------------------------------------------------------------------------

def device_knn(x_dev, n, d, k, window=None):
    """-> (rc, top_val [rows][k], top_idx [rows][k]) out of canary-padded buffers; window = (row_lo, row_hi) goes through gss_knn_topk_rows"""
    lib = _lib.load()
    rows = n if window is None else max(window[1] - window[0], 0)
    bv, tv = padded(rows * k, torch.float64)
    bi, ti = padded(rows * k, torch.int32)
    if window is None:
        rc = lib.gss_knn_topk(n, d, _lib.ptr(x_dev), k, tv.data_ptr(), ti.data_ptr(), _lib.current_stream())
    else:
        rc = lib.gss_knn_topk_rows(n, d, _lib.ptr(x_dev), k, window[0], window[1], tv.data_ptr(), ti.data_ptr(), _lib.current_stream())
    return rc, inside(bv, rows * k).reshape(rows, k), inside(bi, rows * k).reshape(rows, k)


_tables = {}


def whole_table(name):
    """the case's whole-table call, once"""
    if name not in _tables:
        x, k = K.knn_case(name)
        rc, val, idx = device_knn(_dev(x), x.shape[0], x.shape[1], k)
        assert rc == 0, _error()
        _tables[name] = (val, idx)
    return _tables[name]


@pytest.mark.parametrize("name", K.KNN_CASES)
def test_knn_topk_keeps_the_contract(name):
    x, k = K.knn_case(name)
    n = x.shape[0]
    val, idx = whole_table(name)
    sim = K.knn_sim(name)
    if name.startswith("gauss"):                                                     # tie-free: argpartition's set, values to the project's 1e-12
        ref = np.argpartition(sim, -k, 1)[:, -k:]
        assert np.array_equal(np.sort(idx, 1), np.sort(ref, 1))
        err = np.abs(np.sort(val, 1) - np.sort(np.take_along_axis(sim, ref, 1), 1)) / np.abs(np.sort(np.take_along_axis(sim, ref, 1), 1))
        print(f"{name}: values against numpy's product, worst relative {err.max():.2e} (bound {T.SETUP_OPS_KNN_RTOL:g})")
        record_measured("setup_ops_knn", **{f"{name}_rel": err.max()})
        assert err.max() <= T.SETUP_OPS_KNN_RTOL
        return
    M.check_topk(sim, val, idx, n)                                                   # integer descriptors: exact in fp64 in any order
    tied = int(M.tie_across_kth(sim, k).sum())
    print(f"{name}: contract holds; {tied} of {n} rows tie across place {k}")
    rc, val2, idx2 = device_knn(_dev(x), n, x.shape[1], k)                           # the same call again: the same bits, ties included
    assert rc == 0 and np.array_equal(f64bits(val2), f64bits(val)) and np.array_equal(idx2, idx)


@pytest.mark.parametrize("name", K.WINDOW_CASES)
def test_knn_row_windows_equal_the_rows_of_the_whole_table_and_write_nothing_else(name):
    x, k = K.knn_case(name)
    n, d = x.shape
    xd = _dev(x)
    val, idx = whole_table(name)
    for lo, hi in K.KNN_WINDOWS:
        rc, wv, wi = device_knn(xd, n, d, k, (lo, hi))                               # the canaries around (hi - lo) * k are checked inside
        assert rc == 0, ((lo, hi), _error())
        assert wv.shape == (hi - lo, k)
        assert np.array_equal(f64bits(wv), f64bits(val[lo:hi])) and np.array_equal(wi, idx[lo:hi]), (name, lo, hi)
        if hi > lo and not name.startswith("gauss"):
            M.check_topk(K.knn_sim(name)[lo:hi], wv, wi, n)
    rc, wv, wi = device_knn(xd, n, d, k, (0, n))                                     # the whole range through the window entry point
    assert rc == 0 and np.array_equal(f64bits(wv), f64bits(val)) and np.array_equal(wi, idx)


def test_knn_refusals_by_name_write_nothing():
    x, _ = K.knn_case("int_130_8_5")
    xd = _dev(x)
    x12 = _dev(np.zeros((130, 12)))
    for (n, d, k, window, data), words in (((130, 8, 0, None, xd), "k=0 out of [1, min(64, n)]"),
                                           ((130, 8, 65, None, xd), "k=65 out of [1, min(64, n)]"),
                                           ((4, 8, 5, None, xd), "k=5 out of [1, min(64, n)]"),          # k > n
                                           ((130, 12, 5, None, x12), "d=12 must be a multiple of 8"),
                                           ((130, 8, 5, (100, 131), xd), "rows [100, 131) out of [0, 130]"),
                                           ((130, 8, 5, (20, 10), xd), "rows [20, 10) out of [0, 130]")):
        lib = _lib.load()
        rows = 130
        bv, tv = padded(rows * 64, torch.float64)
        bi, ti = padded(rows * 64, torch.int32)
        if window is None:
            rc = lib.gss_knn_topk(n, d, _lib.ptr(data), k, tv.data_ptr(), ti.data_ptr(), _lib.current_stream())
        else:
            rc = lib.gss_knn_topk_rows(n, d, _lib.ptr(data), k, window[0], window[1], tv.data_ptr(), ti.data_ptr(), _lib.current_stream())
        assert rc == EINVAL, words
        assert words in _error(), _error()
        torch.cuda.synchronize()
        assert bool((bv == SENTF).all()) and bool((bi == SENT).all()), words
    val, idx = whole_table("int_130_8_5")                                            # and the next valid call is what it was
    rc, v2, i2 = device_knn(xd, 130, 8, 5)
    assert rc == 0 and np.array_equal(f64bits(v2), f64bits(val)) and np.array_equal(i2, idx)


# ---- gss_normalize_adj / gss_rowsum_dinv / gss_scale_adj_shard ------------------------------------------------------------------------

def device_rowsum_dinv(c, rows=None):
    """gss_rowsum_dinv on the CSR (or on its first `rows` rows) -> (dinv, rowsum), canaries checked"""
    n = c.n if rows is None else rows
    rp, val = _dev(c.rowptr), _dev(c.val)
    bd, dinv = padded(n, torch.float64)
    bs, rowsum = padded(n, torch.float64)
    rc = _lib.load().gss_rowsum_dinv(n, _lib.ptr(rp), _lib.ptr(val), dinv.data_ptr(), rowsum.data_ptr(), _lib.current_stream())
    assert rc == 0, _error()
    return inside(bd, n), inside(bs, n)


def device_normalize(c):
    """gss_normalize_adj -> (A_hat values fp32, rowsum)"""
    rp, col, val = _dev(c.rowptr), _dev(c.col), _dev(c.val)
    nnz = len(c.val)
    bo, out = padded(nnz, torch.float32)
    bs, rowsum = padded(c.n, torch.float64)
    rc = _lib.load().gss_normalize_adj(c.n, _lib.ptr(rp), _lib.ptr(col), _lib.ptr(val), out.data_ptr(), rowsum.data_ptr(), _lib.current_stream())
    assert rc == 0, _error()
    got = inside(bo, nnz), inside(bs, c.n)
    assert np.array_equal(val.cpu().numpy(), c.val) and np.array_equal(col.cpu().numpy(), c.col)      # inputs left alone
    return got


def device_scale_shard(row0, rp, col, val, dinv, transposed, rows=None):
    rows = len(rp) - 1 if rows is None else rows
    d = [_dev(x) for x in (rp, col if len(col) else np.zeros(1, np.int32), val if len(val) else np.zeros(1), dinv)]
    bo, out = padded(len(val), torch.float32)
    rc = _lib.load().gss_scale_adj_shard(rows, row0, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), transposed, out.data_ptr(),
                                         _lib.current_stream())
    assert rc == 0, _error()
    return inside(bo, len(val))


@pytest.mark.parametrize("name", K.NORM_CASES)
def test_normalisation_row_sums_to_1e13_and_values_bit_for_bit_from_the_devices_own_dinv(name):
    c = K.norm_case(name)
    want_rowsum, want_dinv = M.rowsum_dinv(c.rowptr, c.val)
    dinv, rowsum = device_rowsum_dinv(c)
    got, rowsum2 = device_normalize(c)
    assert got.dtype == np.float32
    assert np.array_equal(f64bits(rowsum2), f64bits(rowsum))                         # the one kernel behind both entry points
    err_sum = np.abs(rowsum - want_rowsum) / want_rowsum
    err_dinv = np.abs(dinv - want_dinv) / want_dinv
    err_val = np.abs(got - M.scale(c.rowptr, c.col, c.val, want_dinv, as_fp32=False)) / M.scale(c.rowptr, c.col, c.val, want_dinv, as_fp32=False)
    print(f"{name}: rowsum {err_sum.max():.2e}, dinv {err_dinv.max():.2e} (bound {T.SETUP_OPS_ROWSUM_RTOL:g}); "
          f"A_hat against fp64 {err_val.max():.2e} (bound {T.SETUP_OPS_AHAT_RTOL:g})")
    record_measured("setup_ops_normalize", **{f"{name}_rowsum": err_sum.max(), f"{name}_dinv": err_dinv.max(), f"{name}_ahat": err_val.max()})
    assert err_sum.max() <= T.SETUP_OPS_ROWSUM_RTOL and err_dinv.max() <= T.SETUP_OPS_ROWSUM_RTOL
    want = M.scale(c.rowptr, c.col, c.val, dinv)                                     # the device's own D^-1/2: no pow ulp in the comparison
    wrong = np.flatnonzero(f32bits(got) != f32bits(want))
    assert len(wrong) == 0, (name, wrong[:5], got[wrong[:5]], want[wrong[:5]])
    assert err_val.max() <= T.SETUP_OPS_AHAT_RTOL
    only_dinv, _ = device_rowsum_dinv_without_rowsum(c)                              # rowsum_out = NULL: the same D^-1/2
    assert np.array_equal(f64bits(only_dinv), f64bits(dinv))


def device_rowsum_dinv_without_rowsum(c):
    rp, val = _dev(c.rowptr), _dev(c.val)
    bd, dinv = padded(c.n, torch.float64)
    rc = _lib.load().gss_rowsum_dinv(c.n, _lib.ptr(rp), _lib.ptr(val), dinv.data_ptr(), None, _lib.current_stream())
    assert rc == 0, _error()
    return inside(bd, c.n), None


def test_shards_of_the_asymmetric_matrix_and_of_its_transpose_equal_a_hat_bit_for_bit():
    c, t = K.norm_case(K.ASYMMETRIC), K.transpose_case(K.ASYMMETRIC)
    dinv, _ = device_rowsum_dinv(c)
    whole, _ = device_normalize(c)
    t_dinv, t_sum = device_rowsum_dinv(t)
    whole_t = sp.csr_matrix(sp.csr_matrix((whole, c.col, c.rowptr), shape=(c.n, c.n)).T)
    whole_t.sort_indices()
    assert np.array_equal(whole_t.indptr, t.rowptr) and np.array_equal(whole_t.indices, t.col)
    for row0, rows in K.shard_cuts(c.n):
        rp, col, val, e0 = K.cut(c, row0, rows)
        got = device_scale_shard(row0, rp, col, val, dinv, 0)
        assert np.array_equal(f32bits(got), f32bits(whole[e0:e0 + len(val)])), ("rows of A", row0, rows)
        assert np.array_equal(f32bits(got), f32bits(M.scale_shard(row0, rp, col, val, dinv, 0)))
        rp, col, val, e0 = K.cut(t, row0, rows)
        got = device_scale_shard(row0, rp, col, val, dinv, 1)
        assert np.array_equal(f32bits(got), f32bits(whole_t.data[e0:e0 + len(val)])), ("rows of the transpose", row0, rows)
        assert np.array_equal(f32bits(got), f32bits(M.scale_shard(row0, rp, col, val, dinv, 1)))
        part_dinv, part_sum = device_rowsum_dinv(types.SimpleNamespace(n=rows, rowptr=rp, val=val))   # a shard's own rows: the whole matrix's
        assert np.array_equal(f64bits(part_sum), f64bits(t_sum[row0:row0 + rows])) and np.array_equal(f64bits(part_dinv), f64bits(t_dinv[row0:row0 + rows]))
    rp, col, val, _ = K.cut(c, 5, 4)                                                 # an empty shard: success, nothing written or read
    for transposed in (0, 1):
        bo, out = padded(len(val), torch.float32)
        d = [_dev(x) for x in (rp, col, val, dinv)]
        assert _lib.load().gss_scale_adj_shard(0, 5, _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), _lib.ptr(d[3]), transposed, out.data_ptr(),
                                               _lib.current_stream()) == 0
        assert (inside(bo, len(val)) == SENTF).all()
    bd, dv = padded(4, torch.float64)
    assert _lib.load().gss_rowsum_dinv(0, None, None, dv.data_ptr(), None, _lib.current_stream()) == 0
    assert (inside(bd, 4) == SENTF).all()


# ---- gss_rowsum_check -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.CHECK_CASES)
def test_rowsum_check_counts_the_bad_rows_and_names_the_first(name):
    v = K.check_case(name)
    n = len(v)
    vd = _dev(v)
    count, first = C.c_int64(-5), C.c_int32(-5)
    rc = _lib.load().gss_rowsum_check(n, _lib.ptr(vd), C.byref(count), C.byref(first), _lib.current_stream())
    assert rc == 0, _error()
    assert (count.value, first.value) == M.rowsum_check(v), name
    assert np.array_equal(f64bits(vd.cpu().numpy()), f64bits(v))
    count2 = C.c_int64(-5)                                                           # first_out = NULL is allowed
    assert _lib.load().gss_rowsum_check(n, _lib.ptr(vd), C.byref(count2), None, _lib.current_stream()) == 0 and count2.value == count.value
    if name == "planted_1000":
        for m in (1, 63, 64, 65, 256, 257):                                          # a prefix of the vector: rows past n are not read as bad
            rc = _lib.load().gss_rowsum_check(m, _lib.ptr(vd), C.byref(count), C.byref(first), _lib.current_stream())
            assert rc == 0 and (count.value, first.value) == M.rowsum_check(v[:m]), m
