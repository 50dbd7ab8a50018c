"""Cases for the shard-vs-one-GPU bit identity of the balanced SpMM where the automatic feature-slice policy (csrc/spmm.hip
launch_balanced) would decide differently on a shard than on the whole graph.

The policy cuts the features into slices when the gathered operand is beyond 8 MiB.  The slice count sets the lane-group width, that
sets the lane groups per wave (GPW), and a row's segment sums (segments of 32 entries, csrc/segments.h) are combined by an xor tree inside
a wave and then in wave order: with four segments one GPW gives ((s0+s1)+s2)+s3, another (s0+s1)+(s2+s3).  A shard's own operand is its
rows plus the boundary rows it reads -- far fewer rows than N --, so a graph just above the threshold is sliced on one GPU and unsliced on
every shard, unless the shard's handle is told the job's operand rows (gss_csr_set_job_cols).

One case per width, at the smallest N (a multiple of 128 per node range) above the threshold:

    d      N       ranges   GPW unsliced -> sliced   rows regroup above
    1024   2,304   2        1 -> 2                   64 entries
    256    8,448   3        1 -> 4                   64 entries
    128    16,640  2        2 -> 4                   128 entries  (3-4 segments: (s0+s1)+(s2+s3) under both)

The graph is block-local: a band of +-32 around the diagonal with about 8 entries per row, so a node range reads at most 32 foreign
columns on either side.  Every node range carries planted rows whose lengths sit either side of p = 2 / 4 / 8 lane groups per row, of
the 512-entry cap of a GPW-1 workgroup (16 waves x 32 entries; above 512 * GPW entries the cap on p moves the segment boundaries too),
and far beyond it, plus one empty row.  Planted rows draw their columns from their own range, so the halo stays the band's.

Nothing here needs a GPU; tests/test_shard_grouping_cases.py checks that the builder plants what it says and that shard_of is the
sharded trainer's renumbering (dist.sharded_plan_engine's shard_of)."""
import functools
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

SIZES = {1024: (2304, 2), 256: (8448, 3), 128: (16640, 2)}      # d -> (N, node ranges)
PLANTED = (33, 64, 65, 128, 129, 257, 512, 513, 1025, 2000)      # the last: min(2000, range size)
REGROUP_ABOVE = {1024: 64, 256: 64, 128: 128}                    # rows with more entries are grouped differently by the two GPWs
BAND = 32

Case = namedtuple("Case", "d n ranges a x planted empty")         # planted: {range index: [(row, length), ...]}; empty: {range index: row}
Shard = namedtuple("Shard", "lo hi a halo x n_cols")             # a: [hi - lo] x [n_cols] with own-first-then-halo column ids


def ranges_of(n, parts):
    return [(k * n // parts, (k + 1) * n // parts) for k in range(parts)]


def planted_lengths(size):
    return [min(k, size) for k in PLANTED]


@functools.lru_cache(maxsize=None)
def case(d):
    n, parts = SIZES[d]
    rng = np.random.RandomState(1000 + d)
    ranges = ranges_of(n, parts)
    rows = [None] * n
    for i in range(n):
        w0, w1 = max(0, i - BAND), min(n, i + BAND + 1)
        rows[i] = np.sort(rng.choice(np.arange(w0, w1), int(rng.randint(4, 13)), replace=False))
    planted, empty = {}, {}
    for k, (lo, hi) in enumerate(ranges):
        size = hi - lo
        lens = planted_lengths(size)
        # spread inside the range, clear of its ends (a sharded plan's nnz-balanced boundaries sit near, not at, these ranges' ends)
        at = lo + size // 8 + (np.arange(len(lens) + 1) * (3 * size // 4)) // (len(lens) + 1)
        planted[k] = []
        for r, ln in zip(at[:-1], lens):
            rows[r] = np.sort(rng.choice(np.arange(lo, hi), ln, replace=False))
            planted[k].append((int(r), int(ln)))
        empty[k] = int(at[-1])
        rows[empty[k]] = np.zeros(0, np.int64)
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    data = (0.1 + 0.9 * rng.rand(len(indices))).astype(np.float32)
    a = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    x = rng.randn(n, d).astype(np.float32)
    return Case(d, n, ranges, a, x, planted, empty)


def shard_of(a, lo, hi, x=None):
    """rows [lo, hi) of `a` as a shard holds them: the entries stay in ascending GLOBAL column order, the ids become operand rows -- the
    shard's own rows first (column c in [lo, hi) -> c - lo), then the foreign columns it references in ascending order (the halo) --
    and the operand is [x[lo:hi]; x[halo]]"""
    sub = sp.csr_matrix(a[lo:hi])
    sub.sort_indices()
    cols = sub.indices.astype(np.int64)
    uniq = np.unique(cols)
    halo = uniq[(uniq < lo) | (uniq >= hi)]
    gid2op = np.full(a.shape[1], -1, np.int64)
    gid2op[lo:hi] = np.arange(hi - lo)
    gid2op[halo] = (hi - lo) + np.arange(len(halo))
    n_cols = (hi - lo) + len(halo)
    local = sp.csr_matrix((sub.data.astype(np.float32), gid2op[cols].astype(np.int32), sub.indptr.astype(np.int32)), shape=(hi - lo, n_cols))
    x_local = None if x is None else np.concatenate([x[lo:hi], x[halo]]).astype(np.float32)
    return Shard(lo, hi, local, halo, x_local, n_cols)


def map_back(sh):
    """the global column id of every stored entry of a shard, in storage order"""
    op2gid = np.concatenate([np.arange(sh.lo, sh.hi), sh.halo])
    return op2gid[sh.a.indices]


def adjacency(c):
    """the case's pattern as a symmetric 0/1 adjacency without a diagonal: what a trainer is given.  A planted row keeps its length or
    gains the few entries its column mirrors add."""
    m = sp.csr_matrix((np.ones(c.a.nnz, np.float64), c.a.indices, c.a.indptr), shape=c.a.shape)
    m = ((m + m.T) > 0).astype(np.float64).tolil()
    m.setdiag(0)
    m = sp.csr_matrix(m)
    m.eliminate_zeros()
    m.sort_indices()
    return m
