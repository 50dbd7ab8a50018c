"""Shared by test_profile_rank.py (CPU) and the GPU tests of gss_profile_rank: csrc/profile_rank.hip's arithmetic in numpy (the
order-preserving keys with -0.0 folded into +0.0, the column sorted in chunks padded to a power of two with the all-ones key, two searches per
chunk and key, (acc + 1) / 2, NaN propagation) and the seeded inputs the tests rank."""
import numpy as np

CHUNK = 16384                      # kRkChunk
PANEL = 512                        # kKeyPanel (profile_front.h)
STATUS_BYTES = 256                 # kStatusBytes (profile_front.h)
BEHIND = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = (1, 2, 63, 64, 65, 1000, 16383, 16384, 16385, 32768, 32769, 40000)
KINDS = ("uniform", "small_integers", "zeros_and_tails", "all_equal")


def keys(v):
    """rk_key: uint64 keys that order as IEEE comparison orders the doubles; +-0.0 one value, NaN -> the all-ones key"""
    v = np.asarray(v, dtype=np.float64)
    b = np.where(v == 0.0, 0.0, v).view(np.uint64)
    k = np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(v), BEHIND, k)


def pow2_at_least(c):
    p = 64
    while p < c:
        p <<= 1
    return p


def mirror_rank(v, chunk=CHUNK):
    """one column as rk_rank_kernel and rk_write_kernel rank it"""
    k = keys(v)
    n = len(k)
    acc = np.zeros(n, dtype=np.int32)
    for c0 in range(0, n, chunk):
        part = k[c0:c0 + chunk]
        srt = np.sort(np.concatenate([part, np.full(pow2_at_least(len(part)) - len(part), BEHIND, dtype=np.uint64)]))[:len(part)]
        acc += (np.searchsorted(srt, k, "left") + np.searchsorted(srt, k, "right")).astype(np.int32)
    if np.any(k == BEHIND):
        return np.full(n, np.nan)
    return (acc + 1).astype(np.float64) * 0.5


def workspace_bytes(n, nc):
    """gss_profile_rank_workspace_bytes, the formula of include/gssgcn.h"""
    if n < 1 or nc < 0:
        return 0
    p = min(nc, PANEL)
    up8 = lambda b: (b + 7) // 8 * 8   # noqa: E731
    return STATUS_BYTES + p * n * 8 + up8(p * n * 4) + up8(p * 4)


def column(kind, n, seed):
    """one seeded input column of n fp64 values"""
    rng = np.random.RandomState(seed)
    if kind == "uniform":
        return rng.rand(n)
    if kind == "small_integers":
        return rng.randint(0, 5, size=n).astype(np.float64)
    if kind == "all_equal":
        return np.full(n, 0.25)
    if kind != "zeros_and_tails":
        raise ValueError(kind)
    v = rng.lognormal(-8.0, 4.0, size=n)                      # the heavy tail of a profile, many orders of magnitude
    u = rng.rand(n)
    v[u < 0.6] = np.where(rng.rand(int((u < 0.6).sum())) < 0.5, 0.0, -0.0)
    special = np.array([np.inf, -np.inf, 5e-324, -5e-324, np.inf, 5e-324])
    at = rng.permutation(n)[:min(n, len(special))]
    v[at] = special[:len(at)]
    return v


def columns(n, count, seed):
    """count columns [count][n], the four kinds in turn"""
    return np.stack([column(KINDS[j % len(KINDS)], n, seed + 31 * j) for j in range(count)])
