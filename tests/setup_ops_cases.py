"""Inputs of the op-by-op tests of the setup ops (tests/test_setup_ops_mirror.py on the CPU, tests/test_gpu_setup_ops.py on the GPU):
named, small, deterministic, each with the property it exists for.  tests/test_setup_ops_mirror.py asserts those properties on the
mirror alone -- a seed that loses one fails there, not on the GPU.  Mirror results are computed once and shared; treat every array as
read-only.

Percentile (pct_case(name) -> e fp32 [n][d]; pct_qs(name) -> the percentiles asked of it):
  lat_<n>_<d>   entries in {-1, -1/2, 0, 1/2, 1}: every partial sum of an inner product is a multiple of 1/4 no larger than d, exact in fp32
                in any order.  Tens of levels of both signs, tie groups of up to thousands of entries.
  special_65    rows 0..63 equal, row 64 of its own: three levels -- the 64 x 64 diagonal tile, the 2 x 64 entries of the one off-diagonal
                tile (held as 64 entries of weight 2) and the single entry of the last tile.
  all_equal     every row the same: one level, one bin in every pass.
  adjacent      n = 40, E[i][0] = 1 + i 2^-11: 820 distinct products 1 + (i + j) 2^-11 + i j 2^-22 that share the first radix digit and
                differ in the second and third.
  unit_<n>      random unit rows (the generator of test_percentile_exact): not exact, held to the project's 2e-6 and to a rank condition.
  nan, inf, overflow   lat_65_16 with one NaN entry, one +inf entry, two entries of 2e19 (finite in fp32, their product is not).
For an exact case the percentiles are placed at level boundaries: with c the number of entries up to and including level A, pos = c - 1
(lo the last of A, hi the first of B, frac 0), c - 1/2, c - 1/4 and c, at about six boundaries of which one has A < 0 <= B wherever the
case has a negative similarity; then q = 0, q = 100 and one q inside the largest tie group.

kNN (knn_case(name) -> x fp64 [n][d], k): integer descriptors in {-2..2} (similarities exact in fp64), names int_<n>_<d>_<k>;
`equal_130` (all rows equal: every similarity ties); gauss_<n>_<d>_<k> tie-free.  KNN_WINDOWS are the row windows of gss_knn_topk_rows.

Normalisation (norm_case(name) -> n, rowptr, col, val of A + I in CSR, columns ascending, A with random positive weights and no
diagonal): n in {1, 3, 4, 5, 257, 320}; rows of forced length 1, 63, 64, 65, 129 (and 300 at n = 320, the only size with room for it).
Structure and weights are not symmetric.  SHARD_CUTS are the (row0, rows) windows of the n = 257 matrix and of its transpose.
Row-sum checks (check_case(name) -> fp64 vector): bad rows planted at 0, 63, 64, 255, 256, n - 1, or in every row."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import setup_ops_mirror as M

SEED = 20251


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- percentile -----------------------------------------------------------------------------------------------------------------------

LATTICE_N = (1, 2, 3, 63, 64, 65, 129, 200)
LATTICE_D = (16, 48, 64, 1024)
LATTICE_CASES = [f"lat_{n}_{d}" for n in LATTICE_N for d in LATTICE_D]
EXACT_CASES = LATTICE_CASES + ["special_65", "all_equal", "adjacent"]
UNIT_CASES = ["unit_129", "unit_1000"]
UNIT_D = {"unit_129": 16, "unit_1000": 128}
UNIT_QS = (0.0, 37.5, 50.0, 98.0, 99.9, 100.0)
NON_FINITE_CASES = ["nan", "inf", "overflow"]
NON_FINITE_QS = (0.0, 50.0, 98.0, 100.0)
N_BOUNDARIES = 6


def _lattice(n, d, seed):
    return (np.random.RandomState(seed).randint(-2, 3, (n, d)) * 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pct_case(name):
    if name.startswith("lat_"):
        n, d = (int(t) for t in name.split("_")[1:])
        e = _lattice(n, d, SEED + 7 * n + d)
    elif name == "special_65":
        two = _lattice(2, 16, SEED + 1)
        e = np.repeat(two[:1], 65, 0)
        e[64] = two[1]
    elif name == "all_equal":
        e = np.repeat(_lattice(1, 16, SEED + 2), 65, 0)
    elif name == "adjacent":
        e = np.zeros((40, 16), np.float32)
        e[:, 0] = 1.0 + np.arange(40) * 2.0 ** -11
    elif name.startswith("unit_"):
        n = int(name.split("_")[1])
        x = np.random.RandomState(n).randn(n, UNIT_D[name])
        e = (x / np.sqrt((x ** 2).sum(1, keepdims=True))).astype(np.float32)
    elif name in NON_FINITE_CASES:
        e = pct_case("lat_65_16").copy()
        if name == "nan":
            e[10, 3] = np.nan
        elif name == "inf":
            e[10, 3] = np.inf
        else:
            e[5, 0] = e[7, 0] = np.float32(2e19)
    else:
        raise KeyError(name)
    return _frozen(e)


@functools.lru_cache(maxsize=None)
def pct_sim(name):
    with np.errstate(invalid="ignore", over="ignore"):
        return _frozen(M.similarities(pct_case(name)))


@functools.lru_cache(maxsize=None)
def pct_sorted(name):
    return _frozen(np.sort(pct_sim(name), axis=None))


def q_for(n, target, lo):
    """the q whose pos = q / 100 * (n^2 - 1) lands at `target` with int(pos) == lo, nudged by single ulps where the division rounds across"""
    m = n * n
    if m == 1:
        return 0.0
    q = min(100.0, max(0.0, 100.0 * target / (m - 1)))
    for _ in range(8):
        got = M.position(n, q)[0]
        if got == lo:
            return q
        q = float(np.nextafter(q, 100.0 if got < lo else 0.0))
    raise AssertionError((n, target, lo, q))


@functools.lru_cache(maxsize=None)
def pct_boundaries(name):
    """indices b into the levels: the boundary between level b and level b + 1.  The sign boundary first, then both ends and an even spread"""
    val, cum = M.levels(pct_sim(name))
    nb = len(val) - 1
    if nb <= 0:
        return ()
    picks = []
    neg = np.flatnonzero(val < 0)
    if len(neg):
        picks.append(int(neg[-1]))                                    # A = the largest negative level, B >= 0 (the diagonal is never negative)
    picks += [int(round(t)) for t in np.linspace(0, nb - 1, N_BOUNDARIES - 1)]
    out = []
    for b in picks:
        if b not in out:
            out.append(b)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pct_plan(name):
    """-> list of (q, intended lo, what): the percentiles of an exact case"""
    s = pct_sim(name)
    n = s.shape[0]
    m = n * n
    val, cum = M.levels(s)
    plan = []
    for b in pct_boundaries(name):
        c = int(cum[b])
        for target, lo, what in ((c - 1, c - 1, "last_of_A"), (c - 0.5, c - 1, "midpoint"), (c - 0.25, c - 1, "inside_straddle"), (c, c, "in_B")):
            plan.append((q_for(n, target, lo), lo, f"{what}@{b}"))
    cnt = np.diff(np.concatenate([[0], cum]))
    big = int(np.argmax(cnt))
    inside = int(cum[big] - cnt[big] + cnt[big] // 2)                 # the middle entry of the largest tie group
    plan += [(0.0, 0, "q0"), (100.0, m - 1, "q100"), (q_for(n, inside, inside), inside, "largest_group")]
    return plan


def pct_qs(name):
    if name in UNIT_CASES:
        return list(UNIT_QS)
    if name in NON_FINITE_CASES:
        return list(NON_FINITE_QS)
    return [q for q, _lo, _what in pct_plan(name)]


@functools.lru_cache(maxsize=None)
def pct_mirror(name):
    """float32 results of the mirror for pct_qs(name)"""
    e, s = pct_case(name), pct_sim(name)
    return _frozen(np.array([M.percentile(e, q, s) for q in pct_qs(name)], np.float32))


# ---- kNN top-k ------------------------------------------------------------------------------------------------------------------------

KNN_N = (1, 2, 63, 64, 65, 130)
KNN_D = (8, 24, 64)


def _ks(n):
    return sorted({k for k in (1, 5, min(n, 64)) if k <= n})


INT_CASES = [f"int_{n}_{d}_{k}" for n in KNN_N for d in KNN_D for k in _ks(n)]
GAUSS_CASES = ["gauss_130_24_5", "gauss_65_8_64", "gauss_64_64_1"]
KNN_CASES = INT_CASES + ["equal_130"] + GAUSS_CASES
# d = 8, more than one column left out: at least a quarter of the rows tie across the k-th place (tests/test_setup_ops_mirror.py)
TIE_CASES = [c for c in INT_CASES if c.split("_")[2] == "8" and int(c.split("_")[1]) >= 63 and 1 < int(c.split("_")[3]) < int(c.split("_")[1]) - 1]
KNN_WINDOWS = ((0, 1), (1, 64), (63, 66), (64, 65), (65, 130), (17, 17))
WINDOW_CASES = ["int_130_8_5", "int_130_24_64", "equal_130"]


@functools.lru_cache(maxsize=None)
def knn_case(name):
    """-> (x fp64 [n][d], k)"""
    if name == "equal_130":
        x = np.repeat(np.random.RandomState(SEED + 3).randint(-2, 3, (1, 8)).astype(np.float64), 130, 0)
        return _frozen(x), 5
    kind, n, d, k = name.split("_")
    n, d, k = int(n), int(d), int(k)
    rng = np.random.RandomState(SEED + 13 * n + d)                   # one table per (n, d), whatever k
    x = rng.randint(-2, 3, (n, d)).astype(np.float64) if kind == "int" else rng.randn(n, d)
    return _frozen(x), k


@functools.lru_cache(maxsize=None)
def knn_sim(name):
    return _frozen(M.knn_sim(knn_case(name)[0]))


# ---- normalisation --------------------------------------------------------------------------------------------------------------------

NORM_CASES = ["n1", "n3", "n4", "n5", "n257", "n320"]
FORCED = {"n257": {0: 1, 3: 63, 4: 64, 7: 65, 128: 129, 256: 64, 255: 1}, "n320": {0: 300, 1: 1, 2: 63, 5: 64, 6: 65, 200: 129, 319: 300, 318: 65}}
ASYMMETRIC = "n257"
SHARD_ROW0 = lambda n: (0, 1, n // 2, n - 1)  # noqa: E731
SHARD_SIZES = (1, 4, 5, None)                 # None: the remainder


@functools.lru_cache(maxsize=None)
def norm_case(name):
    """-> namespace(n, adj (scipy CSR of A, no diagonal), rowptr int32, col int32, val fp64) -- the arrays are A + I"""
    n = int(name[1:])
    rng = np.random.RandomState(SEED + n)
    rows, cols = [], []
    for r in range(n):
        length = FORCED.get(name, {}).get(r)
        if length is None:
            length = 1 + int(rng.randint(0, min(n, 12)))
        others = np.setdiff1d(np.arange(n), [r])
        pick = rng.choice(others, length - 1, replace=False)
        rows += [r] * (length - 1)
        cols += pick.tolist()
    w = rng.uniform(0.05, 3.0, len(rows))
    adj = sp.csr_matrix((w, (np.array(rows, np.int64), np.array(cols, np.int64))), shape=(n, n), dtype=np.float64)
    a = sp.csr_matrix(adj + sp.eye(n, dtype=np.float64, format="csr"))
    a.sort_indices()
    return types.SimpleNamespace(n=n, adj=adj, rowptr=_frozen(a.indptr.astype(np.int32)), col=_frozen(a.indices.astype(np.int32)),
                                 val=_frozen(a.data.astype(np.float64)))


def csr_of(c):
    return sp.csr_matrix((c.val, c.col, c.rowptr), shape=(c.n, c.n))


@functools.lru_cache(maxsize=None)
def transpose_case(name):
    """the same matrix transposed, as a CSR of its own"""
    c = norm_case(name)
    t = sp.csr_matrix(csr_of(c).T)
    t.sort_indices()
    return types.SimpleNamespace(n=c.n, rowptr=_frozen(t.indptr.astype(np.int32)), col=_frozen(t.indices.astype(np.int32)),
                                 val=_frozen(t.data.astype(np.float64)))


def shard_cuts(n):
    out = []
    for row0 in SHARD_ROW0(n):
        for size in SHARD_SIZES:
            rows = n - row0 if size is None else size
            if row0 + rows <= n and (row0, rows) not in out:
                out.append((row0, rows))
    return out


def cut(c, row0, rows):
    """rows [row0, row0 + rows) of a CSR as a shard: rowptr from 0, global column ids -> (rowptr, col, val, first entry)"""
    e0, e1 = int(c.rowptr[row0]), int(c.rowptr[row0 + rows])
    return (c.rowptr[row0:row0 + rows + 1] - e0).astype(np.int32), c.col[e0:e1].copy(), c.val[e0:e1].copy(), e0


CHECK_N = (1, 63, 64, 65, 257, 1000)
BAD_VALUES = (0.0, -0.0, -1.5, float("nan"))
BAD_AT = (0, 63, 64, 255, 256)
CHECK_CASES = [f"{kind}_{n}" for n in CHECK_N for kind in ("planted", "every", "good")] + ["late_1000"]


@functools.lru_cache(maxsize=None)
def check_case(name):
    kind, n = name.split("_")
    n = int(n)
    v = np.random.RandomState(SEED + n).uniform(0.5, 9.0, n)
    v[n // 3] = np.inf                                                # good: +inf > 0
    v[n // 2] = 5e-324                                                # good: the smallest subnormal > 0
    if kind == "planted":
        at = sorted({p for p in BAD_AT + (n - 1,) if p < n})
        for t, p in enumerate(at):
            v[p] = BAD_VALUES[t % 4]
    elif kind == "every":
        v = np.array([BAD_VALUES[i % 4] for i in range(n)], np.float64)
    elif kind == "late":                                              # the first bad row in the last wave of the last block, three in it
        v[[997, 998, 999]] = (np.nan, -0.0, -2.0)
    return _frozen(v)
