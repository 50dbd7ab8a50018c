"""fp64 mirror of the row-sparse SpMM modes of csrc/spmm.hip (SPMM_BWD1S, SPMM_BWD2S, the row- and gather-filtered SPMM_PLAIN /
SPMM_FWD1) and of the bitmap builders they consume: what every mode must compute, which rows it must write, which it must leave alone and
which bits it must set -- stated entry by entry over the stored entries of the CSR, not as a densified product, so that a filter is a
statement about single entries here as it is in the kernel.  tests/test_sparse_hop_mirror.py checks this file against scipy products of
the scattered dense operands; tests/test_gpu_sparse_ops.py holds the kernels to it.  The dense backward modes (SPMM_BWD1, SPMM_BWD2:
bwd1_dense, bwd2_dense at the end of this file) are stated the same way, with the second pass's y_in and the own-row limit a sharded
plan passes; tests/test_dense_hop_mirror.py checks them on the CPU, tests/test_gpu_dense_hops.py holds the kernels to them.

Every mode returns, next to its values, per output row the number k of stored entries that contribute and per element the magnitude S:
the mode's own expression with the absolute value of every term.  A kernel that sums the k products in fp32 in ANY order and runs the
epilogue's few fp32 operations differs from the exact value by at most

    (k + 4) * 2^-24 * S

(the standard forward bound of a k-term fp32 sum of products, gamma_k <= k u (1 + o(1)) with u = 2^-24, plus at most four roundings of
the epilogue: the Hadamard product, the compact operand's addition / t's addition, the scale by c, the residual's addition).  One
dropped or doubled entry in a row of degree 1 moves the result by S itself, 2^21 bounds away.

With dtype = np.float32 the same loops run in fp32, in entry order: the CPU check that this bound holds for an actual fp32 evaluation."""
from collections import namedtuple

import numpy as np

UNIT = 2.0 ** -24


def bound(k, s, extra=4):
    """(k + extra) 2^-24 S per element, k per row"""
    return (np.asarray(k, np.float64)[:, None] + extra) * UNIT * np.asarray(s, np.float64)


# ---------------------------------------------------------------- bitmaps (uint32 words; bit i = word i >> 5, bit i & 31)
def words_for(n_bits):
    return (int(n_bits) + 31) // 32


def pack_bits(ids, n_bits):
    w = np.zeros(words_for(n_bits), np.uint32)
    for i in np.asarray(ids, np.int64).reshape(-1):
        w[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return w


def unpack_bits(words, n_bits):
    w = np.asarray(words, np.uint32)
    i = np.arange(int(n_bits))
    return ((w[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def get_bit(words, i):
    return bool((int(words[i >> 5]) >> (i & 31)) & 1)


def mark_rows_and_neighbours(a, rows, words):
    """bits |= every listed row and every column of a listed row's stored entries; negative list entries are skipped"""
    out = np.array(words, np.uint32, copy=True)
    for r in np.asarray(rows, np.int64):
        if r < 0:
            continue
        out[r >> 5] |= np.uint32(1) << np.uint32(r & 31)
        for e in range(a.indptr[r], a.indptr[r + 1]):
            c = int(a.indices[e])
            out[c >> 5] |= np.uint32(1) << np.uint32(c & 31)
    return out


def batch_bits(ids, words, set_):
    """set: bits |= ids.  clear: the WORDS of the ids := 0 (contract: every set bit of such a word belongs to ids).  Negative ids skipped"""
    out = np.array(words, np.uint32, copy=True)
    for i in np.asarray(ids, np.int64):
        if i < 0:
            continue
        if set_:
            out[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
        else:
            out[i >> 5] = 0
    return out


def bits_fill(words, first, last):
    """bits [first, last) := 1, every other bit untouched"""
    out = np.array(words, np.uint32, copy=True)
    for i in range(int(first), int(last)):
        out[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return out


# ---------------------------------------------------------------- the modes
def elu_grad(p):
    p = np.asarray(p)
    return np.where(p > 0, p.dtype.type(1), np.exp(np.minimum(p, 0)))


Bwd1 = namedtuple("Bwd1", "u t s_u s_t k nz written")
Bwd2 = namedtuple("Bwd2", "dp gx s_dp s_gx k")
Fwd = namedtuple("Fwd", "y m s_y s_m k written")


def bwd1_sparse(a, g_am_b, g_ax_b, pos, pos_row, x_in, ax, posbits=None, live_rows=None, skip_zero_rows=False, dtype=np.float64):
    """SPMM_BWD1S.  a: scipy CSR [n_rows][n_cols] (fp32 values); g_am_b, g_ax_b: compact [B][d]; pos[c] = compact row of column c or
    -1; pos_row[r] = compact row of output row r or -1; x_in, ax: [n_rows][d].
        dm[r] = sum over the stored entries (r, c) with pos[c] >= 0 (and bit c of posbits, when given) of A[r, c] g_am_b[pos[c]]
        u[r]  = dm[r] (.) x_in[r]  (+ g_ax_b[pos_row[r]] where pos_row[r] >= 0)
        t[r]  = dm[r] (.) ax[r]
    live_rows (a bitmap, optional): a row whose bit is clear is not walked: dm[r] = 0.
    nz[r] (the bit of nzbits_out) = r is a batch row (pos_row[r] >= 0) or dm[r] has a non-zero element -- decided per ROW.
    written[r] = every row, or under skip_zero_rows the rows with nz[r] only; a written row is written in full, zeros included."""
    n_rows = a.shape[0]
    d = g_am_b.shape[1]
    val = a.data.astype(dtype)
    g_am = g_am_b.astype(dtype)
    dm = np.zeros((n_rows, d), dtype)
    s_dm = np.zeros((n_rows, d), np.float64)
    k = np.zeros(n_rows, np.int64)
    for r in range(n_rows):
        if live_rows is not None and not get_bit(live_rows, r):
            continue
        for e in range(a.indptr[r], a.indptr[r + 1]):
            c = int(a.indices[e])
            if posbits is not None and not get_bit(posbits, c):
                continue
            if pos[c] < 0:
                continue
            dm[r] = dm[r] + val[e] * g_am[pos[c]]
            s_dm[r] += abs(float(a.data[e])) * np.abs(g_am_b[pos[c]].astype(np.float64))
            k[r] += 1
    u = dm * x_in.astype(dtype)
    t = dm * ax.astype(dtype)
    s_u = s_dm * np.abs(x_in.astype(np.float64))
    s_t = s_dm * np.abs(ax.astype(np.float64))
    member = np.asarray(pos_row[:n_rows]) >= 0
    for r in np.flatnonzero(member):
        u[r] = u[r] + g_ax_b[pos_row[r]].astype(dtype)
        s_u[r] += np.abs(g_ax_b[pos_row[r]].astype(np.float64))
    nz = member | (dm != 0).any(1)
    written = nz.copy() if skip_zero_rows else np.ones(n_rows, bool)
    return Bwd1(u, t, s_u, s_t, k, nz, written)


def bwd2_sparse_res(a, u, t, p, c, res_b, pos_row, nzbits=None, y_in=None, pos_row_limit=0, dtype=np.float64):
    """SPMM_BWD2S.  u: [n_cols][d]; t, pos_row: [n_rows][d] / [n_rows] -- or pos_row_limit rows of them when that is > 0; p: [n_rows][d];
    res_b: compact [B][d].
        gx[r] = t[r] + (y_in[r]) + sum over the stored entries (r, c) (with bit c of nzbits, when given) of A[r, c] u[c]
        dp[r] = c gx[r] (.) elu'(p[r])  (+ res_b[pos_row[r]] where pos_row[r] >= 0)
    Rows at or behind pos_row_limit have neither t nor a residual.  nzbits' contract: a clear bit c says rows c of u AND of t are zero,
    so the filter changes no sum; here the filtered entries are simply left out.  Every row is written."""
    n_rows = a.shape[0]
    d = u.shape[1]
    val = a.data.astype(dtype)
    uu = u.astype(dtype)
    acc = np.zeros((n_rows, d), dtype)
    s = np.zeros((n_rows, d), np.float64)
    k = np.zeros(n_rows, np.int64)
    for r in range(n_rows):
        for e in range(a.indptr[r], a.indptr[r + 1]):
            col = int(a.indices[e])
            if nzbits is not None and not get_bit(nzbits, col):
                continue
            acc[r] = acc[r] + val[e] * uu[col]
            s[r] += abs(float(a.data[e])) * np.abs(u[col].astype(np.float64))
            k[r] += 1
    if y_in is not None:
        acc = y_in.astype(dtype) + acc
        s = s + np.abs(y_in.astype(np.float64))
        k = k + 1
    own = n_rows if pos_row_limit <= 0 else min(n_rows, int(pos_row_limit))
    gx = acc.copy()
    gx[:own] = t[:own].astype(dtype) + acc[:own]
    s_gx = s.copy()
    s_gx[:own] += np.abs(t[:own].astype(np.float64))
    eg = elu_grad(p.astype(dtype))
    dp = dtype(c) * (gx * eg)
    s_dp = abs(float(c)) * s_gx * eg.astype(np.float64)
    for r in range(own):
        if pos_row[r] >= 0:
            dp[r] = dp[r] + res_b[pos_row[r]].astype(dtype)
            s_dp[r] += np.abs(res_b[pos_row[r]].astype(np.float64))
    return Bwd2(dp, gx, s_dp, s_gx, k)


def spmm_filtered(a, x, h=None, row_pos=None, row_bits=None, y_in=None, gather_bits=None, dtype=np.float64):
    """SPMM_PLAIN / SPMM_FWD1 under filters.
        y[r] = (y_in[r]) + sum over the stored entries (r, c) (with bit c of gather_bits, when given) of A[r, c] x[c];  m[r] = y[r] (.) h[r]
    written[r] = (row_pos is None or row_pos[r] >= 0) and (row_bits is None or bit r of row_bits); other rows keep what they held."""
    n_rows = a.shape[0]
    d = x.shape[1]
    val = a.data.astype(dtype)
    xx = x.astype(dtype)
    written = np.ones(n_rows, bool)
    if row_pos is not None:
        written &= np.asarray(row_pos[:n_rows]) >= 0
    if row_bits is not None:
        written &= unpack_bits(row_bits, n_rows)
    y = np.zeros((n_rows, d), dtype)
    s = np.zeros((n_rows, d), np.float64)
    k = np.zeros(n_rows, np.int64)
    for r in np.flatnonzero(written):
        for e in range(a.indptr[r], a.indptr[r + 1]):
            col = int(a.indices[e])
            if gather_bits is not None and not get_bit(gather_bits, col):
                continue
            y[r] = y[r] + val[e] * xx[col]
            s[r] += abs(float(a.data[e])) * np.abs(x[col].astype(np.float64))
            k[r] += 1
    if y_in is not None:
        y = np.where(written[:, None], y_in.astype(dtype) + y, y)
        s = s + np.where(written[:, None], np.abs(y_in.astype(np.float64)), 0.0)
        k = k + 1
    m = s_m = None
    if h is not None:
        m = y * h.astype(dtype)
        s_m = s * np.abs(h.astype(np.float64))
    return Fwd(y, m, s, s_m, k, written)


# ---------------------------------------------------------------- the dense backward modes (SPMM_BWD1, SPMM_BWD2)
def _dense_sum(a, x, y_in, dtype):
    """acc[r] = (y_in[r] +) sum over the stored entries (r, c) of A[r, c] x[c], entry by entry in entry order; its magnitude; its k"""
    n_rows = a.shape[0]
    d = x.shape[1]
    val = a.data.astype(dtype)
    xx = x.astype(dtype)
    acc = np.zeros((n_rows, d), dtype)
    s = np.zeros((n_rows, d), np.float64)
    k = np.zeros(n_rows, np.int64)
    for r in range(n_rows):
        for e in range(a.indptr[r], a.indptr[r + 1]):
            col = int(a.indices[e])
            acc[r] = acc[r] + val[e] * xx[col]
            s[r] += abs(float(a.data[e])) * np.abs(x[col].astype(np.float64))
            k[r] += 1
    if y_in is not None:
        acc = y_in.astype(dtype) + acc
        s = s + np.abs(y_in.astype(np.float64))
        k = k + 1
    return acc, s, k


def bwd1_dense(a, g_am, g_ax, x_in, ax, y_in=None, dtype=np.float64):
    """SPMM_BWD1.  a: scipy CSR [n_rows][n_cols]; g_am: [n_cols][d]; g_ax, x_in, ax: [n_rows][d]; y_in (the first pass's sums): [n_rows][d].
        dm[r] = (y_in[r] +) sum over the stored entries (r, c) of A[r, c] g_am[c]
        u[r]  = g_ax[r] + dm[r] (.) x_in[r]
        t[r]  = dm[r] (.) ax[r]
    Every row is written (nz and written are all rows); an empty row gets u = g_ax and t = 0.  k counts the row's stored entries, + 1
    with y_in.  Epilogue roundings inside the 4 of bound(): the Hadamard product and g_ax's addition for u (one when the two contract
    into a multiply-add), the Hadamard product for t."""
    n_rows = a.shape[0]
    dm, s_dm, k = _dense_sum(a, g_am, y_in, dtype)
    u = g_ax.astype(dtype) + dm * x_in.astype(dtype)
    t = dm * ax.astype(dtype)
    s_u = np.abs(g_ax.astype(np.float64)) + s_dm * np.abs(x_in.astype(np.float64))
    s_t = s_dm * np.abs(ax.astype(np.float64))
    every = np.ones(n_rows, bool)
    return Bwd1(u, t, s_u, s_t, k, every, every.copy())


def bwd2_dense(a, u, t, p, c, res=None, y_in=None, own_row_limit=0, dtype=np.float64):
    """SPMM_BWD2.  u: [n_cols][d]; p: [n_rows][d]; t, res: [n_rows][d] -- or own_row_limit rows of them when that is > 0.
        gx[r] = t[r] + ((y_in[r] +) sum over the stored entries (r, c) of A[r, c] u[c])
        dp[r] = c gx[r] (.) elu'(p[r])  (+ res[r])
    Rows at or behind own_row_limit have neither t nor a residual: gx = A u (+ y_in), dp = c gx (.) elu'(p).  Every row is written; an
    empty row gets gx = t.  k counts the row's stored entries, + 1 with y_in.  Epilogue roundings inside the 4 of bound(): t's
    addition, the Hadamard product with elu'(p), the scale by c, the residual's addition."""
    n_rows = a.shape[0]
    acc, s, k = _dense_sum(a, u, y_in, dtype)
    own = n_rows if own_row_limit <= 0 else min(n_rows, int(own_row_limit))
    gx = acc.copy()
    gx[:own] = t[:own].astype(dtype) + acc[:own]
    s_gx = s.copy()
    s_gx[:own] += np.abs(t[:own].astype(np.float64))
    eg = elu_grad(p.astype(dtype))
    dp = dtype(c) * (gx * eg)
    s_dp = abs(float(c)) * s_gx * eg.astype(np.float64)
    if res is not None:
        dp[:own] = dp[:own] + res[:own].astype(dtype)
        s_dp[:own] += np.abs(res[:own].astype(np.float64))
    return Bwd2(dp, gx, s_dp, s_gx, k)
