"""Shared by test_profile_topk.py (CPU) and the GPU tests of gss_profile_topk / gss_topk_overlap: csrc/profile_topk.hip's algorithm in numpy
(the order-preserving keys, the radix select by 8-bit digits from the top with its early stop on a bucket taken whole, the index digits
among the keys tied at the k-th place, the collection and the final sort by (key descending, index ascending)), the statement both are held
to (np.argsort(-col[members], kind="stable")[:k]), the workspace formula and the seeded inputs."""
import numpy as np

from profile_rank_mirror import BEHIND, KINDS, column, keys  # noqa: F401  (the key and the input kinds are gss_profile_rank's)

PANEL = 512                        # kKeyPanel (profile_front.h)
THREADS = 512                      # kTkThreads
STATUS_BYTES = 256                 # kStatusBytes (profile_front.h)
MAX_K, MAX_GROUPS, MAX_ROWS = 1024, 8, 1 << 24
# the issue's sizes; 511 / 512 / 513: one sweep of the select kernel's 512 threads and the next; 255 / 256 / 257 and 65535 / 65536 / 65537:
# a node index gains its second and its third 8-bit digit (the tie-break among equal keys runs over those digits)
SIZES = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 16383, 16384, 16385, 65535, 65536, 65537)
NAN_BITS = np.float64(np.nan).view(np.int64)


def workspace_bytes(n, nc, G, k):
    """gss_profile_topk_workspace_bytes, the formula of include/gssgcn.h"""
    if n < 1 or n > MAX_ROWS or nc < 0 or not 1 <= G <= MAX_GROUPS or not 1 <= k <= MAX_K:
        return 0
    return STATUS_BYTES + min(nc, PANEL) * n * 8


def columns(n, count, seed):
    """count columns [count][n]: profile_rank_mirror's four kinds in turn (uniform; small integers = heavy ties; zeros of both signs with a
    lognormal tail, +-inf and +-5e-324; all equal)"""
    return np.stack([column(KINDS[j % len(KINDS)], n, seed + 31 * j) for j in range(count)])


def groups(n, G, seed, empty=None):
    """a seeded group array [n] int32 over [-1, G): about a fifth of the nodes in no group; group `empty` has no node"""
    g = np.random.RandomState(seed).randint(-1, G, size=n).astype(np.int32)
    if n > 4:
        g[np.random.RandomState(seed + 1).rand(n) < 0.2] = -1
    if empty is not None:
        g[g == empty] = -1
    return g


def members_of(group, n, g):
    return np.arange(n) if group is None else np.flatnonzero(np.asarray(group) == g)


def expected(v, group, G, k):
    """the statement: -> (idx [G][k] int32, val bits [G][k] int64, cnt [G] int32)"""
    v = np.asarray(v, dtype=np.float64)
    idx = np.full((G, k), -1, np.int32)
    val = np.full((G, k), NAN_BITS, np.int64)
    cnt = np.zeros(G, np.int32)
    for g in range(G):
        m = members_of(group, len(v), g)
        col = v[m]
        if np.isnan(col).any():
            cnt[g] = -1
            continue
        top = m[np.argsort(-col, kind="stable")[:k]]
        cnt[g] = len(top)
        idx[g, :len(top)] = top
        val[g, :len(top)] = v[top].view(np.int64)
    return idx, val, cnt


def _select_digit(hist, need, from_top):
    """the bin that holds the need-th entry counted from the top (from the bottom) -> (digit, entries ahead of it)"""
    order = range(255, -1, -1) if from_top else range(256)
    ahead = 0
    for d in order:
        if ahead < need <= ahead + hist[d]:
            return d, ahead
        ahead += int(hist[d])
    raise AssertionError("need is outside the histogram")


def mirror_select(key, m, k):
    """tk_select_kernel's threshold for one group with more than k members m: -> (T, I, sweeps): admitted = key > T, or key == T and index <= I"""
    T, I, need, sweeps = 0, None, k, 0
    active = m
    for ph in range(8):
        shift = 56 - 8 * ph
        digit = ((key[active] >> np.uint64(shift)) & np.uint64(255)).astype(np.int64)
        hist = np.bincount(digit, minlength=256)
        d, ahead = _select_digit(hist, need, True)
        sweeps += 1
        T |= d << shift
        need -= ahead
        active = active[digit == d]
        if hist[d] == need:
            return T, None, sweeps
    I = 0
    for q in range(3):
        shift = 16 - 8 * q
        digit = (active >> shift) & 255
        hist = np.bincount(digit, minlength=256)
        d, ahead = _select_digit(hist, need, False)
        sweeps += 1
        I |= d << shift
        need -= ahead
        active = active[digit == d]
        if hist[d] == need:
            return T, I | ((1 << shift) - 1), sweeps
    raise AssertionError("three index digits did not separate the ties")


def mirror_topk(v, group, G, k):
    """one column as tk_select_kernel selects it -> (idx [G][k], val bits [G][k], cnt [G])"""
    v = np.asarray(v, dtype=np.float64)
    key = keys(v)
    idx = np.full((G, k), -1, np.int32)
    val = np.full((G, k), NAN_BITS, np.int64)
    cnt = np.zeros(G, np.int32)
    for g in range(G):
        m = members_of(group, len(v), g)
        if np.any(key[m] == BEHIND):
            cnt[g] = -1
            continue
        if len(m) <= k:
            take = m
        else:
            T, I, _ = mirror_select(key, m, k)
            km = key[m]
            take = m[(km > np.uint64(T)) | ((km == np.uint64(T)) & ((I is None) | (m <= (I if I is not None else 0))))]
            assert len(take) == k
        take = take[np.lexsort((take, ~key[take]))]          # key descending, index ascending
        cnt[g] = len(take)
        idx[g, :len(take)] = take
        val[g, :len(take)] = v[take].view(np.int64)
    return idx, val, cnt


def expected_overlap(idx, cnt, a, b):
    """np.intersect1d per (pair, group) -> [T][G] int32; -1 where either side is flagged"""
    G = cnt.shape[1]
    out = np.zeros((len(a), G), np.int32)
    for t, (i, j) in enumerate(zip(a, b)):
        for g in range(G):
            if cnt[i, g] < 0 or cnt[j, g] < 0:
                out[t, g] = -1
            else:
                out[t, g] = len(np.intersect1d(idx[i, g, :cnt[i, g]], idx[j, g, :cnt[j, g]]))
    return out
