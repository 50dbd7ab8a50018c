"""Seeded inputs and references of the input-gradient GEMM (gss_dense_bwd_input -> dense_bwd_input -> launch_gemm<EPI_SPLIT> in
csrc/dense.hip): g_ax = dP W1, g_am = dP W2, the weights given transposed ([in][out]) -- TEST INFRASTRUCTURE shared by
tests/test_input_grad_cases.py (CPU) and tests/test_gpu_input_grad.py (GPU).

launch_gemm picks one of 14 instantiations of gemm_nt_lds_kernel for EPI_SPLIT: the whole-line epilogue (no row list) with nt in {2, 4,
8} feature blocks per tile and mt in {1, 2} 16-node tiles per wave, or the MFMA-layout epilogue ("plain": a row list, or nt = 1) with nt
in {1, 2, 4, 8} and mt in {1, 2}.  tile_class() replays that decision; the shapes below are the smallest that reach every class, on both
sides of every threshold and of a tile edge (a tile is 64 mt nodes).

Regimes:
  int    dP, W1^T, W2^T take integer values in [-3, 3]: every partial sum is at most 9 * 1024 < 2^24, so every output is exact in fp32 in
         ANY order and must equal the integer product bit for bit.  A K chunk dropped or doubled, a column tile fed from the wrong weight
         half, a row read from the clamp row, a tile written twice over another's place: each is an exact mismatch.
  unit   N(0, 1), some rows of dP scaled by 2^-20 and some by 2^10 (exact scalings).  Bound, per element:
             |got - ref| <= 1.01 d 2^-24 (|dP| @ |W|)
         the standard forward bound of a length-d dot product in fp32 -- gamma_d = d u / (1 - d u) with u = 2^-24, in any order, with or
         without FMA; 1.01 covers 1 / (1 - d u) and the fp64 reference's own error (d 2^-53) with room.  Derived, not measured.  Per
         element, so the rows scaled down are held as tightly as the others, which a max-norm over the matrix cannot do."""
import functools

import numpy as np

UNIT = 2.0 ** -24
GUARD_ROWS = 128                     # pre-filled rows behind row n of an output without a list: one whole tile of 64 x 2 nodes
VARIANTS = (2, 3, 5)                 # gemm_variant: the default, "3" (forces mt = 2), "5" (no effect on EPI_SPLIT: the 8-wave tiles are forward only)
TILED_ROWS = 4096                    # the 262k-row cases repeat this many distinct rows of dP
BIG_N = (262143, 262144)             # d = 32: both sides of the row threshold of mt (<2, 1> and <2, 2>); no list, int regime


def tile_class(n, d, has_list, gemm_variant=2):
    """(nt, mt, lines) of the gemm_nt_lds_kernel<nt, mt, EPI_SPLIT, 4, lines> that launch_gemm<EPI_SPLIT> launches for n > 0 rows.
    Mirrors csrc/dense.hip, launch_gemm:
      `int nt = (d % 128 == 0) ? 8 : (d % 64 == 0) ? 4 : (d % 32 == 0) ? 2 : 1;`
      `if (EPI == EPI_SPLIT) while (nt > 2 && ceil_div(g.n, 64) * (g.J / (16 * nt)) < 256) nt >>= 1;`           (J = 2 d)
      `const int mt = K().gemm_variant == 3 ? 2 : ((d >= 256 || g.n >= 262144) ? 2 : 1);`
      `if (!g.rows && nt >= 2)` -> the whole-line kernels (GSS_GEMM_LINES), else the MFMA-layout kernels (GSS_GEMM_CASE).
    The row-list branches in between (`short_list`, gemm_rows_split_kernel, the one-wave tiles), the weight-stationary kernel and the
    eight-wave tiles all carry `EPI != EPI_SPLIT`: the input gradient never takes them, whatever gemm_variant says."""
    assert n > 0 and d % 16 == 0 and 16 <= d <= 1024
    nt = 8 if d % 128 == 0 else 4 if d % 64 == 0 else 2 if d % 32 == 0 else 1
    while nt > 2 and -(-n // 64) * (2 * d // (16 * nt)) < 256:
        nt >>= 1
    mt = 2 if gemm_variant == 3 else (2 if (d >= 256 or n >= 262144) else 1)
    return nt, mt, (not has_list) and nt >= 2


def node_tiles(n, d, gemm_variant=2):
    """gridDim.x of the launch: xcd_ids takes one branch for fewer than 8 node tiles, one for a multiple of 8, both with a remainder"""
    return -(-n // (64 * tile_class(n, d, False, gemm_variant)[1]))


ALL_CLASSES = tuple([(nt, mt, True) for nt in (2, 4, 8) for mt in (1, 2)] + [(nt, mt, False) for nt in (1, 2, 4, 8) for mt in (1, 2)])

SMALL_N = (1, 15, 16, 17, 63, 64, 65, 129)
# (d, n): every case runs without and with a row list of n rows, under every gemm_variant of VARIANTS, in both regimes
CASES = (
    [(16, n) for n in SMALL_N] + [(48, 65), (48, 129)]                                  # nt = 1
    + [(272, n) for n in SMALL_N + (127, 128)]                                            # nt = 1, mt = 2
    + [(32, n) for n in SMALL_N + (447, 511, 513, 1025)]                                  # nt = 2; 1, 7, 8, 9 and 17 node tiles
    + [(96, 65), (96, 129)]
    + [(288, n) for n in SMALL_N + (127, 128, 895, 1023, 1025, 2049)]                     # nt = 2, mt = 2; 1, 7, 8, 9 and 17 node tiles
    + [(64, n) for n in (8128, 8129, 8191, 8192)]                                         # nt = 4 from 8129 = 127 * 64 + 1 on
    + [(192, n) for n in (2688, 2689, 2751, 2752)]                                        # nt = 4 from 2689
    + [(320, n) for n in (1600, 1601, 1663, 1664, 1665)]                                  # nt = 4, mt = 2 from 1601; 1664 = 13 * 128
    + [(128, n) for n in (129, 4032, 4033, 4095, 4096, 8128, 8129, 8191, 8192)]           # nt = 4 from 4033, nt = 8 from 8129
    + [(256, n) for n in (129, 1984, 1985, 2047, 2048, 4032, 4033, 4095, 4096)]           # mt = 2: nt = 4 from 1985, nt = 8 from 4033
    + [(384, n) for n in (1344, 1345, 1407, 1408, 2688, 2689, 2751, 2752)]                # nt = 4 from 1345, nt = 8 from 2689
    + [(512, n) for n in (960, 961, 1023, 1024, 1984, 1985, 2047, 2048)]                  # nt = 4 from 961, nt = 8 from 1985
    + [(1024, n) for n in (448, 449, 511, 512, 960, 961, 1023, 1024)]                     # nt = 4 from 449, nt = 8 from 961
)
XCD_TILES = (1, 7, 8, 9, 17)         # node-tile counts the cases at d = 32 and d = 288 must show


def reached():
    """class -> the (d, n, has_list, gemm_variant) launches of the GPU tests that run it"""
    out = {c: [] for c in ALL_CLASSES}
    for d, n in CASES:
        for has_list in (False, True):
            for v in VARIANTS:
                out[tile_class(n, d, has_list, v)].append((d, n, has_list, v))
    for n in BIG_N:
        out[tile_class(n, 32, False)].append((32, n, False, 2))
    return out


def _freeze(c):
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def row_list(rng, n):
    """n unique rows of [0, 3 n): a permutation prefix that holds row 0 (first) and row 3 n - 1 (last; the only entry when n = 1)"""
    big = 3 * n
    lst = rng.permutation(big)[:n]
    must = [big - 1] if n == 1 else [0, big - 1]
    rest = [r for r in lst if r not in must][:n - len(must)]
    lst = np.array(must[:1] + rest + must[1:], np.int32)
    assert len(lst) == n and len(set(lst.tolist())) == n and lst.min() >= 0 and lst.max() == big - 1
    return lst


def scales(n):
    """the exact row scalings of the unit regime: 2^-20 on rows 3 mod 7, 2^10 on rows 5 mod 11 (both from n = 6 on), 1 elsewhere"""
    s = np.ones(n, np.float32)
    r = np.arange(n)
    s[r % 7 == 3] = np.float32(2.0 ** -20)
    s[r % 11 == 5] = np.float32(2.0 ** 10)
    return s


@functools.lru_cache(maxsize=4)
def case(regime, d, n):
    """dp [n][d], w1t, w2t [d][d] ([in][out]: g_ax = dp @ w1t.T), rows [n] -- read only"""
    rng = np.random.RandomState((n * 7919 + d * 31 + (regime == "int")) % (2 ** 31))
    if regime == "int":
        dp, w1t, w2t = (rng.randint(-3, 4, s).astype(np.float32) for s in ((n, d), (d, d), (d, d)))
    else:
        dp, w1t, w2t = (rng.randn(*s).astype(np.float32) for s in ((n, d), (d, d), (d, d)))
        dp *= scales(n)[:, None]
    return _freeze(dict(regime=regime, n=n, d=d, dp=dp, w1t=w1t, w2t=w2t, rows=row_list(rng, n)))


def exact(dp, w1t, w2t):
    """int regime: the integer products as float32.  Evaluated in float64, where every partial sum (below 2^24) is exact in any order, and
    taken through int64; tests/test_input_grad_cases.py holds this to numpy's own int64 matmul"""
    out = []
    for wt in (w1t, w2t):
        p = dp.astype(np.float64) @ wt.astype(np.float64).T
        q = p.astype(np.int64)
        assert (q == p).all() and np.abs(q).max() < 2 ** 24
        out.append(q.astype(np.float32))
    return tuple(out)


def reference(dp, w1t, w2t):
    """unit regime: (g_ax, g_am) in float64 and the per-element bounds 1.01 d 2^-24 (|dP| @ |W|)"""
    d = dp.shape[1]
    a = dp.astype(np.float64)
    ref, lim = [], []
    for wt in (w1t, w2t):
        w = wt.astype(np.float64).T
        ref.append(a @ w)
        lim.append(1.01 * d * UNIT * (np.abs(a) @ np.abs(w)))
    return tuple(ref), tuple(lim)


@functools.lru_cache(maxsize=2)
def big_case(n):
    """d = 32, int regime, n rows that repeat TILED_ROWS distinct ones: dp, weights, and the exact outputs (one small product, indexed)"""
    d = 32
    rng = np.random.RandomState(n % (2 ** 31))
    base, w1t, w2t = (rng.randint(-3, 4, s).astype(np.float32) for s in ((TILED_ROWS, d), (d, d), (d, d)))
    which = np.arange(n) % TILED_ROWS
    gax, gam = exact(base, w1t, w2t)
    return _freeze(dict(n=n, d=d, dp=base[which], w1t=w1t, w2t=w2t, gax=gax[which], gam=gam[which]))


# ---------------------------------------------------------------- seeded mutations (what the checks must reject)
def drop_k_chunk(dp, chunk):
    """dP without the 16 input features of one K chunk: what a kernel computes that skips that chunk"""
    out = dp.copy()
    out[:, 16 * chunk:16 * (chunk + 1)] = 0
    return out


def swap_halves(w1t, w2t, nt, tile):
    """the weights as a kernel sees them that feeds column tile `tile` (16 nt output features) of BOTH halves from the other half"""
    a, b = w1t.copy(), w2t.copy()
    s = slice(16 * nt * tile, 16 * nt * (tile + 1))
    a[s], b[s] = w2t[s], w1t[s]
    return a, b
