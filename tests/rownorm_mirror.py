"""The backward of the row normalisation fused with ELU' on the batch rows (rownorm_elu_bwd_kernel, csrc/elementwise.hip; autograd of
modules/model.py:173,201-205), restated in numpy -- TEST INFRASTRUCTURE.  tests/test_rownorm_mirror.py checks this file on the CPU,
tests/test_gpu_rownorm.py holds gss_rownorm_elu_bwd / gss_rownorm_elu_bwd_ex to it.

    dot[r] = sum_j de[r][j] e[idx[r]][j]
    dx[r]  = (de[r] - e[idx[r]] dot[r]) inv_den[idx[r]]
    dp[r]  = c dx[r] (.) elu'(p[idx[r]]),   elu'(p) = 1 for p > 0, exp(p) otherwise
    pos_set[idx[r]] = r                       (the side write: the key of the batch-sparse backward hop)

e and inv_den are INPUTS, taken as given in float32 (the forward pass's results): the contract is the exact value of these formulas on
them, evaluated here in float64.

The derived bound, per element, u = 2^-24.  A row of d floats lies on LPR = min(64, pow2ceil(d / 4)) lanes of VPL float4 each
(row_geometry).  A lane sums its 4 VPL products sequentially, the lanes are then summed by an xor tree of log2(LPR) levels: every
product passes at most m = 4 VPL + log2(LPR) roundings (its own, at most 4 VPL - 1 additions in the lane, log2(LPR) in the tree; fewer
where the compiler contracts a product and an addition into an fma), so |dot^ - dot| <= m u S_dot, S_dot = sum_j |de| |e| (gamma_m
= m u (1 + o(1)), m <= 22).
  dx adds three roundings: the product e dot^, the subtraction, the product with inv_den.  With S_dx = |inv_den| (|de| + |e| S_dot)
     |dx^ - dx| <= |inv_den| (m u |e| S_dot  +  u |e| S_dot  +  2 u (|de| + |e| S_dot))  <=  (m + 3) u S_dx
  dp adds two roundings (the Hadamard product, the scale by c; one where c = 1) and expf's own error, which the device library states
     as 1 ulp = 2 u relative at most (the same expf whose error the users of sparse_hop_mirror.elu_grad carry inside their four
     epilogue roundings).  With S_dp = |c| S_dx elu'(p):
     |dp^ - dp| <= (m + 3 + 2 + 2) u S_dp = (m + 7) u S_dp
One float4 of a row missing from the dot moves dx by |e| |inv_den| times four products of the row: tens to thousands of bounds away on
the seeded cases (tests/test_rownorm_mirror.py prints the smallest distance per width)."""
from collections import namedtuple

import numpy as np

from sparse_hop_mirror import UNIT, elu_grad

DX_EXTRA = 3        # roundings of dx behind the dot
DP_EXTRA = 7        # ... of dp: dx's 3, two more, and 2 u for expf (1 ulp)
EPS = 1e-12

Bwd = namedtuple("Bwd", "dx dp s_dx s_dp")


def row_geometry(d):
    """(d4, lpr_log2, vpl) as csrc/elementwise.hip row_geometry"""
    d4 = d // 4
    lg = 2
    while (1 << lg) < d4 and lg < 6:
        lg += 1
    return d4, lg, (1 if d4 <= 64 else 2 if d4 <= 128 else 4)


def depth(d):
    """m: the roundings a product of the dot passes at most"""
    _, lg, vpl = row_geometry(d)
    return 4 * vpl + lg


def rows_per_block(d):
    return 4 * (64 >> row_geometry(d)[1])


def bound_dx(d, s_dx):
    return (depth(d) + DX_EXTRA) * UNIT * np.asarray(s_dx, np.float64)


def bound_dp(d, s_dp):
    return (depth(d) + DP_EXTRA) * UNIT * np.asarray(s_dp, np.float64)


def backward(de, idx, e, inv_den, p, c):
    """the contract in float64 on the float32 inputs as given -> Bwd(dx, dp, S_dx, S_dp), all [b][d]"""
    idx = np.asarray(idx, np.int64)
    g, ev, inv = de.astype(np.float64), e[idx].astype(np.float64), inv_den[idx].astype(np.float64)[:, None]
    dot = (g * ev).sum(1, keepdims=True)
    s_dot = (np.abs(g) * np.abs(ev)).sum(1, keepdims=True)
    dx = (g - ev * dot) * inv
    s_dx = np.abs(inv) * (np.abs(g) + np.abs(ev) * s_dot)
    eg = elu_grad(p[idx].astype(np.float64))
    return Bwd(dx, float(c) * (dx * eg), s_dx, abs(float(c)) * s_dx * eg)


def pos_set(idx, n, free):
    """the batch-position map after the launch: pos_set[idx[r]] = r, `free` everywhere else"""
    out = np.full(n, free, np.int32)
    out[np.asarray(idx, np.int64)] = np.arange(len(idx), dtype=np.int32)
    return out


def backward_fp32(de, idx, e, inv_den, p, c, drop=None):
    """the same formulas in float32 in the kernel's order: lane li of a row's LPR lanes holds the float4 li + 64 k, k < VPL; it adds
    their products element by element (x, y, z, w), the lanes are summed by the xor tree (offsets 1, 2, ..., LPR / 2); no fma.
    drop = (r, f4): the dot of batch row r misses that float4 (a kernel that skipped it).  -> dx, dp in float32"""
    b, d = de.shape
    d4, lg, vpl = row_geometry(d)
    lpr = 1 << lg
    idx = np.asarray(idx, np.int64)
    g, ev = de.astype(np.float32), e[idx].astype(np.float32)
    prod = np.zeros((b, vpl * 64 * 4), np.float32)        # float4 slots beyond d4 hold zeros, as in the kernel
    prod[:, :d] = g * ev
    if drop is not None:
        prod[drop[0], 4 * drop[1]:4 * drop[1] + 4] = 0
    prod = prod.reshape(b, vpl, 64, 4)[:, :, :lpr, :]     # [row][k][lane][element]; lanes >= lpr hold nothing (f4 = li + 64 k, li < lpr)
    assert vpl == 1 or lpr == 64
    lane = np.zeros((b, lpr), np.float32)
    for k in range(vpl):
        q = prod[:, k]
        lane = lane + (((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3])
    o = 1
    while o < lpr:
        lane = lane + lane[:, np.arange(lpr) ^ o]
        o <<= 1
    assert (lane == lane[:, :1]).all() and lane.dtype == np.float32
    dot = lane[:, :1]
    inv = inv_den[idx].astype(np.float32)[:, None]
    dx = (g - ev * dot) * inv
    eg = elu_grad(p[idx].astype(np.float32))
    dp = np.float32(c) * (dx * eg)
    assert dx.dtype == np.float32 and dp.dtype == np.float32
    return dx, dp
