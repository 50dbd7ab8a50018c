"""Seeded inputs of the dense-step tests (tests/test_gpu_dense_step.py; checked on the CPU by tests/test_dense_step_mirror.py) -- TEST
INFRASTRUCTURE.  Shapes are the smallest at which each path of csrc/dense.hip can break; the two long row lists are the smallest that
leave launch_gemm's short-list branch (ceil(n / 64) * J / (16 nt) >= 256).

Regimes of the forward projection:
  unit   ax, am, p_prev ~ N(0, 1), weights I + 0.1 randn (as test_dense_fwd), biases 0.1 randn: P straddles 0, both ELU branches taken
  zero   the same, but b2 = -b1 exactly and some node rows have AX, AM and P_prev all zero: in the kernels P = 0 bit for bit there
         (every product is 0, b1 + b2 = 0), X = 0, E = 0, inv_den = 1e12.  The zero rows are the first and the last node row (first in
         a tile, last in a partial tile) and node row 16 where there is one; a row list has node rows 0 and n - 1 as its first and last
         entry; the batch of a position map holds them all
Regime of the weight gradient:
  int    dP, AX, AM take integer values in [-3, 3], n <= 4096: every partial and every sum is below 2^24 and exact in fp32 in any order
  unit   N(0, 1), as test_dense_bwd_weight"""
import functools

import numpy as np

import dense_step_mirror as M

DECAY = 0.3
SKIP_ONE_IN = 8                      # about one list entry in eight is -1

# ---- forward without the norm (gss_dense_fwd_rows)
ROWS_N = 300
ROWS_LENS = (1, 15, 16, 17, 100)
ROWS_SPLIT_D = (64, 128, 256)        # gemm_rows_split_kernel
ROWS_WAVE_D = (16, 32, 48, 192)      # gemm_nt_lds_kernel<NT, 1, EPI, 1>
LONG_ROWS = ((2048, 1024, 2048), (16400, 128, 16321))      # (N, d, listed rows)
SPLIT_D = (64, 128, 256)
SPLIT_N = (1, 129, 300)
# ---- fused norm (gss_dense_fwd_norm)
NORM_D = (16, 32, 64, 128, 256)
NORM_N = (1, 17, 300)
NORM_LENS = (1, 17, 100)
NORM_LONG = ((16400, 128, 16321), (16400, 256, 16321))
NORM_MEMBERS = 100                   # b = min(n, 100) members of the position map
# ---- gss_rownorm_fwd_rows
ROWNORM_N = 400
ROWNORM_D = (48, 192, 512, 1024)
ROWNORM_LENS = (1, 17, 333)
# ---- weight gradient
REDUCE_K = (1, 3, 4, 5, 12, 13, 16, 17, 28, 29, 32, 33, 60, 61, 64, 65, 100, 128)     # slices: every tail of the reduce's loops
REDUCE_K_SIMPLE = (1, 5, 33, 65)
REDUCE_D_SIMPLE = (16, 48)
PAIR_D = (64, 128, 256)
PAIR_NA, PAIR_NB = 300, 100
# (n, d) of every weight-gradient launch of the GPU tests, against the n_max its buffer is sized for
SLICE_BOUND_CASES = ([(32 * k, 64, 32 * k) for k in REDUCE_K] + [(32 * k, d, 32 * k) for k in REDUCE_K_SIMPLE for d in REDUCE_D_SIMPLE]
                     + [(n, d, n) for d in PAIR_D + (48,) for n in (PAIR_NA, PAIR_NB)] + [(1008, 128, 1034), (1034, 128, 1034)])
# ---- Adam
ADAM_D = (16, 48, 64, 128)
ADAM_STEPS = 5
ADAM_LR = 3e-4
POS_N = 5000
ADAM_B = {16: 2500, 48: 1, 64: 100, 128: 100}      # b = 2500 at d = 16 exceeds the 256 x 9 threads of the reduce proper
TRANSPOSE_DIMS = (16, 48, 64, 100, 128)


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def row_list(rng, n, length, must=()):
    """a permutation prefix of the n node rows with about one entry in eight set to -1; `must` (node rows) sit at the list's ends"""
    lst = rng.permutation(n)[:length].astype(np.int32)
    ends = np.array(([0, length - 1] if length > 1 else [0])[:len(must)], np.int64)
    for pos, row in zip(ends, must):
        where = np.nonzero(lst == row)[0]
        if len(where):
            lst[where[0]] = lst[pos]
        lst[pos] = row
    skip = rng.rand(length) < 1.0 / SKIP_ONE_IN
    skip[ends] = False
    skip[0] = False                       # (a list of one entry lists a row)
    if length >= 15:
        skip[length // 2] = True          # at least one
    lst[skip] = -1
    return lst


@functools.lru_cache(maxsize=None)
def forward(regime, n, d, length=None):
    """the operands of a projection over n node rows of d features; length: also a row list of that many entries.  Read only"""
    rng = np.random.RandomState((n * 7919 + d * 31 + (length or 0) * 1009 + (regime == "zero")) % (2 ** 31))
    ax, am, p_prev = (rng.randn(n, d).astype(np.float32) for _ in range(3))
    w1, w2 = (np.eye(d, dtype=np.float32) + 0.1 * rng.randn(d, d).astype(np.float32) for _ in range(2))
    b1, b2 = (0.1 * rng.randn(d).astype(np.float32) for _ in range(2))
    zero = []
    if regime == "zero":
        b2 = -b1
        zero = sorted({0, n - 1} | ({16} if n > 16 else set()))
    c = dict(regime=regime, n=n, d=d, w1=w1, b1=b1, w2=w2, b2=b2)
    if length is not None:      # the list's first and last entry are zero rows (node rows 0 and n - 1)
        c["list"] = row_list(rng, n, length, ([0] if length == 1 else [0, n - 1]) if zero else [])
    for r in zero:
        ax[r] = am[r] = p_prev[r] = 0.0
    c.update(ax=ax, am=am, p_prev=p_prev, zero=np.array(zero, np.int64))
    # the batch of a full pass: b members (the zero rows among them) at permuted positions, -1 for every other node
    b = min(n, NORM_MEMBERS)
    others = np.setdiff1d(rng.permutation(n), zero, assume_unique=False)
    members = np.concatenate([np.array(zero, np.int64), rng.permutation(others)])[:b]
    pos = np.full(n, -1, np.int32)
    pos[members] = rng.permutation(b).astype(np.int32)
    c.update(b=b, pos=pos)
    return _freeze(c)


@functools.lru_cache(maxsize=64)
def forward_reference(regime, n, d, length=None, prev=True):
    """the fp64 mirror on forward(...): dict(p, x, e, inv_den)"""
    c = forward(regime, n, d, length)
    p, x = M.projection(c["ax"], c["am"], c["w1"], c["b1"], c["w2"], c["b2"], c["p_prev"] if prev else None, DECAY)
    e, inv = M.normalize(x)
    return _freeze(dict(p=p, x=x, e=e, inv_den=inv))


def plain_cases():
    """every (regime, n, d, length) gss_dense_fwd_rows / gss_dense_fwd_first run on"""
    out = [(regime, ROWS_N, d, length) for regime in ("unit", "zero") for d in ROWS_SPLIT_D + ROWS_WAVE_D for length in ROWS_LENS]
    out += [(regime, n, d, None) for regime in ("unit", "zero") for d in SPLIT_D for n in SPLIT_N]
    return out + [("unit", n, d, length) for n, d, length in LONG_ROWS]


def norm_cases():
    """every (regime, n, d, length) gss_dense_fwd_norm runs on"""
    out = [(regime, n, d, None) for regime in ("unit", "zero") for d in NORM_D for n in NORM_N]
    out += [(regime, n, d, None) for regime in ("unit", "zero") for d in SPLIT_D for n in SPLIT_N if n not in NORM_N]     # (in two launches)
    out += [(regime, ROWS_N, d, length) for regime in ("unit", "zero") for d in NORM_D for length in NORM_LENS]
    return out + [("unit", n, d, length) for n, d, length in NORM_LONG]


@functools.lru_cache(maxsize=None)
def rownorm(n, d, length):
    rng = np.random.RandomState(n + 13 * d + 101 * length)
    x = rng.randn(n, d).astype(np.float32)
    x[0] = x[n - 1] = 0.0
    lst = row_list(rng, n, length, [0] if length == 1 else [0, n - 1])
    return _freeze(dict(x=x, list=lst, zero=np.array([0, n - 1], np.int64)))


def rownorm_cases():
    return [(ROWNORM_N, d, length) for d in ROWNORM_D for length in ROWNORM_LENS]


@functools.lru_cache(maxsize=None)
def wgrad(regime, n_nodes, n, d, gathered, seed=0):
    """one weight-gradient problem: dP [n][d] compact; AX, AM [n_nodes][d]; rows (gathered: a permutation prefix of the nodes) or None"""
    rng = np.random.RandomState((seed * 1000003 + n_nodes * 131 + n * 17 + d + (regime == "int")) % (2 ** 31))
    if regime == "int":
        assert n <= 4096
        dp, ax, am = rng.randint(-3, 4, (n, d)), rng.randint(-3, 4, (n_nodes, d)), rng.randint(-3, 4, (n_nodes, d))
    else:
        dp, ax, am = rng.randn(n, d), rng.randn(n_nodes, d), rng.randn(n_nodes, d)
    rows = rng.permutation(n_nodes)[:n].astype(np.int32) if gathered else None
    return _freeze(dict(n=n, d=d, dp=dp.astype(np.float32), ax=ax.astype(np.float32), am=am.astype(np.float32), rows=rows))


def problem(c):
    return c["dp"], c["ax"], c["am"], c["rows"]


def exact(problems):
    """the int64 sums of integer-regime problems, as float32 (every value is below 2^24: exact)"""
    out = M.wgrad(problems, np.int64)
    assert all(np.abs(v).max() < 2 ** 24 for v in out)
    return tuple(v.astype(np.float32) for v in out)


def adam_start(d):
    """parameters and a non-zero optimizer state at step 0"""
    rng = np.random.RandomState(d)
    shapes = (("W1", (d, d)), ("b1", (d,)), ("W2", (d, d)), ("b2", (d,)))
    params = {k: rng.randn(*s).astype(np.float32) for k, s in shapes}
    state = {"t": 0}
    for k, s in shapes:
        state["m_" + k] = (1e-2 * rng.randn(*s)).astype(np.float32)
        state["v_" + k] = (1e-4 * rng.rand(*s)).astype(np.float32)
    return params, state


def adam_step_problems(d, step):
    """the gradient of one step: two problems of mixed magnitude (as test_adam_matches_torch_semantics: 10^U(-6, 0) per step)"""
    rng = np.random.RandomState(1000 * d + step)
    scale = 10.0 ** rng.uniform(-6, 0)
    a, b = wgrad("unit", 300, 300, d, False, seed=step), wgrad("unit", 300, 100, d, True, seed=step)
    return [dict(a, dp=(a["dp"] * scale).astype(np.float32)), dict(b, dp=(b["dp"] * scale).astype(np.float32))]


def adam_idx(d):
    """the batch ids of the position-map reset: b distinct ids of POS_N, about one in eight of them -1"""
    rng = np.random.RandomState(77 + d)
    b = ADAM_B[d]
    idx = rng.permutation(POS_N)[:b].astype(np.int32)
    if b > 1:
        idx[rng.rand(b) < 1.0 / SKIP_ONE_IN] = -1
        idx[b // 2] = -1
    return idx
