"""Seeded inputs of the row-norm tests (tests/test_rownorm_mirror.py on the CPU, tests/test_gpu_rownorm.py on the GPU) -- TEST
INFRASTRUCTURE.  One table of N = 400 node rows per width; the widths are one per (lane group, VPL) class of row_geometry
(csrc/elementwise.hip) and the ones that fill their lane group only partly: 48 (12 of 16 lanes), 192 (48 of 64), 320 (VPL 2, the second
float4 on 16 of 64 lanes), 576 (VPL 4, the third on 16 of 64, the fourth on none).  The batch sizes are the tails of
rows_per_block = 4 (64 >> lpr_log2) = 64, 32, 16, 8, 4: one row, one block less one, a block, a block and one, many blocks and a tail.

e and inv_den are the fp64 normalisation of a seeded x rounded to float32 and are passed as given; row 0 of x is all zero (e = 0,
inv_den = 1e12) and is a batch member.  p carries dense_hop_cases.P_PLANT (+0, -0, the smallest normal, -20) in a member row, an
all-positive and an all-negative member row."""
import functools

import numpy as np

import dense_step_mirror as DM
from dense_hop_cases import P_PLANT

N = 400
WIDTHS = (16, 32, 48, 64, 128, 192, 256, 320, 512, 576, 1024)
BATCHES = (1, 3, 4, 5, 63, 64, 65, 333)
CS = (1.0, 0.3)
FWD_N = (1, 63, 64, 65, 333)
ZERO_ROW, P_ROW, POS_ROW, NEG_ROW = 0, 20, 21, 22
MUST = (ZERO_ROW, P_ROW, POS_ROW, NEG_ROW)       # members of every batch they fit in, in front of row N - 1
POS_FREE = -7                                    # a batch-position map entry nobody wrote
GUARD_ROWS = 64                                  # pre-filled rows behind the rows a launch covers


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def table(d):
    """x, e, inv_den, p over N node rows of d features (e, inv_den: float32 roundings of the fp64 normalisation of x)"""
    rng = np.random.RandomState(4000 + d)
    x = rng.randn(N, d).astype(np.float32)
    x[ZERO_ROW] = 0.0
    e, inv = DM.normalize(x)
    p = rng.randn(N, d).astype(np.float32)
    p[P_ROW, :4] = P_PLANT
    p[POS_ROW] = np.abs(p[POS_ROW]) + np.float32(0.01)
    p[NEG_ROW] = -np.abs(p[NEG_ROW]) - np.float32(0.01)
    c = dict(x=x, e=e.astype(np.float32), inv_den=inv.astype(np.float32), p=p)
    assert not c["e"][ZERO_ROW].any() and c["inv_den"][ZERO_ROW] == np.float32(1e12)
    return _freeze(c)


@functools.lru_cache(maxsize=None)
def batch(d, b):
    """idx [b]: unique rows of [0, N), a permutation prefix that holds row N - 1 (last) and as many of MUST as fit (row 0 first, the
    others at seeded positions); de [b][d] ~ N(0, 1) with one exactly-zero row where b >= 5"""
    rng = np.random.RandomState(100 * d + b)
    must = ([N - 1] if b == 1 else list(MUST[:b - 1]) + [N - 1])
    rest = [r for r in rng.permutation(N) if r not in must][:b - len(must)]
    mid = must[1:-1] + rest
    mid = [mid[i] for i in rng.permutation(len(mid))]
    idx = np.array((must[:1] if b > 1 else []) + mid + must[-1:], np.int32)
    assert len(idx) == b == len(set(idx.tolist())) and idx.min() >= 0 and idx.max() == N - 1 and (b == 1 or idx[0] == 0)
    de = rng.randn(b, d).astype(np.float32)
    if b >= 5:
        de[b // 2] = 0.0
    return _freeze(dict(idx=idx, de=de))


def bwd_cases():
    return [(d, b, c) for d in WIDTHS for b in BATCHES for c in CS]


@functools.lru_cache(maxsize=None)
def fwd_list(d, n):
    """a row list for gss_rownorm_fwd_rows over the first n rows: unique valid rows, rows 0 and n - 1 among them, unsorted"""
    rng = np.random.RandomState(7 * d + n)
    length = max(1, min(n, 17))
    lst = [r for r in rng.permutation(n) if r not in (0, n - 1)][:max(0, length - 2)]
    lst = ([n - 1] if n > 1 else []) + lst + [0]
    return np.array(lst, np.int32)
