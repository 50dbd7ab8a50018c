"""numpy fp64 mirrors of the three ops that run once before the first step (tests/test_setup_ops_mirror.py on the CPU,
tests/test_gpu_setup_ops.py on the GPU):

  percentile        gss_percentile (csrc/percentile.hip) as its header states it: the order statistic of the N^2 inner products, with the
                    host side's own arithmetic for the position and the interpolation.  For inputs whose inner products are exact in fp32.
  select            the same answer by the device's route -- upper-triangular 64 x 64 tiles with off-diagonal tiles counted twice, three
                    radix passes over the order-preserving key, the min pass -- with the wrong rules a test must be able to see (`mutate`).
  check_topk        the contract of gss_knn_topk / gss_knn_topk_rows as a set property (ties across the k-th place are arbitrary).
  fold_topk         the kernel's running top-k of one row in plain Python, with `v > minv` or `v >= minv`.
  rowsum_dinv, scale, scale_shard, rowsum_check
                    the rounding sequence of the K11 kernels of csrc/spmm.hip.
Nothing here is tuned to a device result."""
import numpy as np

TILE = 64
PASSES = ((21, 11), (10, 11), (0, 10))            # (shift, bits) of the three radix passes
MUTATIONS = ("wgt1", "wgt2", "no_mask", "rank_gt", "no_min", "floor_ge")


class NonFinite(ValueError):
    """E E^T holds an inf or a NaN: np.percentile gives NaN; gss_percentile must refuse"""


# ---- percentile -----------------------------------------------------------------------------------------------------------------------

def similarities(e):
    """S = E E^T in fp64.  `+ 0.0`: the device's accumulators start at +0, so a sum that cancels is +0 there, never -0"""
    e64 = np.asarray(e, np.float64)
    return e64 @ e64.T + 0.0


def exact_in_fp32(s):
    s = np.asarray(s, np.float64)
    return bool(np.isfinite(s).all() and np.array_equal(s.astype(np.float32).astype(np.float64), s))


def finite_in_fp32(s):
    """the device forms S in fp32: a finite fp64 product above 3.4e38 is inf there"""
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.isfinite(np.asarray(s, np.float64).astype(np.float32)).all())


def position(n, q):
    """-> (lo, hi, frac) of gss_percentile's host side"""
    m = n * n
    pos = q / 100 * (m - 1)
    lo = min(int(pos), m - 1)
    return lo, min(lo + 1, m - 1), pos - lo


def percentile(e, q, s=None):
    """float32 result of gss_percentile on an input whose similarities are exact in fp32 (asserted), by sorting"""
    s = similarities(e) if s is None else s
    if not finite_in_fp32(s):
        raise NonFinite("non-finite similarity")
    assert exact_in_fp32(s), "the order of the MFMA sum would matter: S is not exact in fp32"
    v = np.sort(s, axis=None)
    lo, hi, frac = position(s.shape[0], q)
    a, b = v[lo], v[hi]
    return np.float32(a + (b - a) * frac)


def levels(s):
    """-> (distinct values ascending, cumulative counts)"""
    val, cnt = np.unique(np.asarray(s, np.float64), return_counts=True)
    return val, np.cumsum(cnt)


def ordered_key(v):
    """percentile.hip's order-preserving uint32 image of a float32"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ordered_key_no_flip(v):
    """the key without the sign handling: orders negative values backwards and below nothing"""
    return np.ascontiguousarray(v, np.float32).view(np.uint32).copy()


def key_to_float(k):
    k = np.uint32(k)
    u = (k & np.uint32(0x7FFFFFFF)) if (k & np.uint32(0x80000000)) else ~k
    return np.array([u], np.uint32).view(np.float32)[0]


def tile_keys(s32, mutate=None):
    """the (key, weight) pairs pct_kernel counts: tiles (it <= jt) of 64 x 64, rows and columns past n clamped to n - 1 on load and masked"""
    n = s32.shape[0]
    nt = -(-n // TILE)
    at = np.minimum(np.arange(nt * TILE), n - 1)
    live = np.arange(nt * TILE) < n
    keys, wts = [], []
    for it in range(nt):
        for jt in range(it, nt):
            i, j = slice(it * TILE, (it + 1) * TILE), slice(jt * TILE, (jt + 1) * TILE)
            blk = s32[np.ix_(at[i], at[j])]
            keep = np.ones(blk.shape, bool) if mutate == "no_mask" else np.outer(live[i], live[j])
            w = 1 if it == jt else 2
            w = {"wgt1": 1, "wgt2": 2}.get(mutate, w)
            keys.append(ordered_key(blk[keep]))
            wts.append(np.full(int(keep.sum()), w, np.int64))
    return np.concatenate(keys), np.concatenate(wts)


def pass0_histogram(keys, wts):
    return np.bincount((keys >> np.uint32(21)).astype(np.int64), weights=wts, minlength=2048).astype(np.int64)


def non_finite_count(hist0):
    """finite keys lie in [0x00800000, 0xFF7FFFFF]: bins 0..3 hold -inf and the negative NaNs, bins 0x7FC..0x7FF +inf and the positive NaNs"""
    return int(hist0[:4].sum() + hist0[0x7FC:].sum())


def select(e, q, mutate=None, trace=None):
    """gss_percentile by the device's route.  -> float32, or None where the host loop finds no bin for the rank.
    trace (a dict) receives key_lo, key_hi, ran_min and the digits chosen."""
    s = similarities(e)
    if not finite_in_fp32(s):
        raise NonFinite("non-finite similarity")
    s32 = s.astype(np.float32)
    keys, wts = tile_keys(s32, mutate)
    lo, hi, frac = position(s.shape[0], q)
    rank, eq, prefix, mask, digits = lo, 0, np.uint32(0), np.uint32(0), []
    for shift, nbits in PASSES:
        sel = (keys & mask) == prefix
        digit = ((keys[sel] >> np.uint32(shift)) & np.uint32((1 << nbits) - 1)).astype(np.int64)
        hist = np.bincount(digit, weights=wts[sel], minlength=1 << nbits).astype(np.int64)
        cum = np.cumsum(hist)
        chosen = int(np.searchsorted(cum, rank, side="right"))          # the first bin with cum > rank
        if chosen == len(hist):
            return None
        rank -= int(cum[chosen] - hist[chosen])
        eq = int(hist[chosen])
        prefix = prefix | np.uint32(chosen << shift)
        mask = mask | np.uint32(((1 << nbits) - 1) << shift)
        digits.append(chosen)
    key_lo = key_hi = prefix
    needs = rank + 1 > eq if mutate == "rank_gt" else rank + 1 >= eq
    ran_min = hi != lo and needs and mutate != "no_min"
    if ran_min:
        above = keys[keys >= key_lo] if mutate == "floor_ge" else keys[keys > key_lo]
        if len(above):
            key_hi = above.min()
    if trace is not None:
        trace.update(key_lo=int(key_lo), key_hi=int(key_hi), ran_min=bool(ran_min), digits=digits)
    a, b = np.float64(key_to_float(key_lo)), np.float64(key_to_float(key_hi))
    return np.float32(a + (b - a) * frac)


# ---- kNN top-k ------------------------------------------------------------------------------------------------------------------------

def knn_sim(x):
    """fp64 X X^T; exact in any order for the integer-valued descriptors of the cases"""
    x = np.asarray(x, np.float64)
    return x @ x.T


def check_topk(sim_rows, top_val, top_idx, n):
    """the contract, row by row (sim_rows [r][n]: the rows the table is about).  Raises AssertionError naming the row and the clause."""
    sim_rows, top_val, top_idx = np.asarray(sim_rows), np.asarray(top_val), np.asarray(top_idx)
    r, k = top_idx.shape
    assert sim_rows.shape == (r, n) and top_val.shape == (r, k) and 1 <= k <= n
    for i in range(r):
        idx = top_idx[i]
        assert ((idx >= 0) & (idx < n)).all(), (i, "index out of [0, n)", idx)
        assert len(np.unique(idx)) == k, (i, "indices repeat", idx)
        assert np.array_equal(top_val[i], sim_rows[i, idx]), (i, "a value is not the similarity of its index")
        assert np.array_equal(np.sort(top_val[i]), np.sort(sim_rows[i])[n - k:]), (i, "not the k largest as a multiset")
        out = np.ones(n, bool)
        out[idx] = False
        if out.any():
            assert sim_rows[i, out].max() <= top_val[i].min(), (i, "a column left out beats one kept")


def tie_across_kth(sim_rows, k):
    """rows whose k-th and (k+1)-th largest similarities are equal: the kept set is not unique there"""
    v = np.sort(np.asarray(sim_rows), axis=1)
    n = v.shape[1]
    if k >= n:
        return np.zeros(len(v), bool)
    return v[:, n - k] == v[:, n - k - 1]


def fold_topk(row, k, strict=True):
    """knn_topk_kernel's lane: fill k slots, then replace the tracked minimum by every v > minv (strict) or v >= minv"""
    mv, mi = [], []
    minv, minp = -np.inf, 0
    for j, v in enumerate(row):
        if len(mv) < k:
            mv.append(v)
            mi.append(j)
            if len(mv) < k:
                continue
        elif (v > minv) if strict else (v >= minv):
            mv[minp], mi[minp] = v, j
        else:
            continue
        minp = int(np.argmin(mv))                                      # the first of equal minima, as the kernel's `<` scan
        minv = mv[minp]
    return np.array(mv, np.float64), np.array(mi, np.int32)


# ---- normalisation --------------------------------------------------------------------------------------------------------------------

def row_of_entry(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def rowsum_dinv(rowptr, val):
    """-> (rowsum, dinv) in fp64: the row's sum, rowsum ** -0.5"""
    n = len(rowptr) - 1
    rowsum = np.array([np.sum(val[rowptr[r]:rowptr[r + 1]], dtype=np.float64) for r in range(n)], np.float64).reshape(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        return rowsum, np.power(rowsum, -0.5)


def scale(rowptr, col, val, dinv, as_fp32=True):
    """(val * dinv[col]) * dinv[row], rounded to fp32 once"""
    out = (np.asarray(val, np.float64) * dinv[col]) * dinv[row_of_entry(rowptr)]
    return out.astype(np.float32) if as_fp32 else out


def scale_shard(row0, rowptr, col, val, dinv, transposed):
    """rows [row0, row0 + n) of A + I (or of its transpose) with global column ids against the D^-1/2 of every node.  An entry (i, j) of a
    transposed shard is A[j][i]: its column scale is dinv of the SHARD's row and is applied first"""
    rows = row0 + row_of_entry(rowptr)
    v = np.asarray(val, np.float64)
    out = (v * dinv[rows]) * dinv[col] if transposed else (v * dinv[col]) * dinv[rows]
    return out.astype(np.float32)


def rowsum_check(rowsum):
    """-> (rows whose sum is not > 0, the first of them or -1)"""
    with np.errstate(invalid="ignore"):
        bad = ~(np.asarray(rowsum, np.float64) > 0.0)
    return int(bad.sum()), int(np.argmax(bad)) if bad.any() else -1
