"""Seeded inputs shared by tests/test_sparse_hop_mirror.py (CPU) and tests/test_gpu_sparse_ops.py (GPU): the graphs, batches and operands
at which the row-sparse SpMM modes are held to tests/sparse_hop_mirror.py.  What a plan's step never feeds them on purpose is fed here
on purpose: batch members on the bitmaps' word edges (0, 31, 32, 63, 64, n - 1), a hub row, an empty row and a hub's neighbour as
members, members whose gradient row is exactly zero, a non-member row all of whose member neighbours have a zero gradient, and 16-byte
pieces that are zero in every member (a live row with zero pieces)."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

WIDTHS = (16, 48, 128, 512)     # narrow lane groups, a d/4 that is no power of two, the common case, more than one float4 per lane
BATCHES = (1, 17, 300)
EDGE_IDS = (0, 31, 32, 63, 64)  # + n - 1: the first and last bit of a bitmap word
# (graph, d, b) per mode: every width, batch size and graph with every mode at least once, no cross product
BWD1_CASES = [("hub", 16, 17), ("hub", 48, 1), ("hub", 128, 300), ("hub", 512, 17), ("rect", 128, 17), ("rect", 48, 300), ("rect", 512, 1),
              ("giant", 128, 17), ("giant", 16, 300)]
BWD2_CASES = [("hub", 16, 300), ("hub", 48, 17), ("hub", 128, 1), ("hub", 512, 300), ("rect", 128, 17), ("rect", 16, 1), ("giant", 48, 17),
              ("giant", 128, 300)]
FWD_CASES = [("hub", 16, 1), ("hub", 128, 17), ("hub", 512, 300), ("rect", 48, 17), ("rect", 128, 300), ("giant", 128, 300), ("giant", 16, 17),
             ("giant", 48, 1)]
LIMIT_CASES = [("rect", 16, 17, 600), ("rect", 128, 300, 600), ("rect", 512, 1, 577)]    # pos_row_limit < n_rows = 900


def random_graph(rng, n, avg_deg, hub_rows=(), hub_deg=0, empty_rows=()):
    m = n * avg_deg
    r = rng.randint(0, n, m)
    c = rng.randint(0, n, m)
    for h in hub_rows:
        r = np.concatenate([r, np.full(hub_deg, h)])
        c = np.concatenate([c, rng.choice(n, hub_deg, replace=False)])
    keep = ~np.isin(r, list(empty_rows))
    r, c = r[keep], c[keep]
    a = sp.csr_matrix((rng.uniform(0.1, 1.0, len(r)), (r, c)), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a


def _fp32(a):
    a = sp.csr_matrix(a)
    a.sort_indices()
    return sp.csr_matrix((a.data.astype(np.float32), a.indices.astype(np.int32), a.indptr.astype(np.int32)), shape=a.shape)


@functools.lru_cache(maxsize=None)
def graph(kind):
    """hub:   1500 x 1500, average degree 7, two hub rows of 1200 entries (rows that span several waves), empty rows 0, 11, n - 1
    rect:  900 x 1400 -- a shard's operand: halo columns behind the own ones -- one hub row, empty rows 0, 11, 899
    giant: 2100 x 2100, three hub rows and row 40 holding every column (a giant row under spmm_giant = 64)"""
    if kind == "hub":
        a = random_graph(np.random.RandomState(7001), 1500, 7, hub_rows=(3, 700), hub_deg=1200, empty_rows=(0, 11, 1499))
        g = SimpleNamespace(a=_fp32(a), hubs=(3, 700), empty=(0, 11, 1499))
    elif kind == "rect":
        a = random_graph(np.random.RandomState(7002), 1400, 7, hub_rows=(5,), hub_deg=1200, empty_rows=(0, 11, 899))
        g = SimpleNamespace(a=_fp32(a[:900, :]), hubs=(5,), empty=(0, 11, 899))
    elif kind == "giant":
        rng = np.random.RandomState(7003)
        a = sp.lil_matrix(random_graph(rng, 2100, 7, hub_rows=(5, 900, 1500), hub_deg=1300, empty_rows=(2, 2099)))
        a[40, :] = rng.uniform(0.1, 1.0, 2100)
        g = SimpleNamespace(a=_fp32(a), hubs=(40, 5), empty=(2, 2099))
    else:
        raise KeyError(kind)
    g.kind = kind
    g.n_rows, g.n_cols = g.a.shape
    g.lens = np.diff(g.a.indptr)
    assert all(g.lens[r] == 0 for r in g.empty) and all(g.lens[h] >= 1200 for h in g.hubs)
    return g


def batch_for(g, b, seed, giant_row_inside=True):
    """b distinct column ids (the batch) in compact order, and the witness row of the zero-sum branch (-1 when b is too small for one).
    From 17 members on the batch holds: the word-edge ids 0, 31, 32, 63, 64, n_cols - 1 (and n_rows - 1), a hub row, empty rows, a column of
    the hub's row, and `zcol`: a member whose gradient the operands set to zero and which is the ONLY member among the columns of the
    non-member row `zrow`."""
    rng = np.random.RandomState(seed)
    a, n_rows, n_cols = g.a, g.n_rows, g.n_cols
    hub = g.hubs[0]
    if b == 1:
        # one member: a different kind of row per seed
        pick = [hub, n_cols - 1, 32, 0, int(a.indices[a.indptr[hub]]), 63][seed % 6]
        if not giant_row_inside and pick == hub:
            pick = 31
        return np.array([pick], np.int32), -1, -1
    hub_nb = int(a.indices[a.indptr[hub] + 7])
    must = list(dict.fromkeys(list(EDGE_IDS) + [n_cols - 1, n_rows - 1, hub, hub_nb] + list(g.empty)))
    if not giant_row_inside:
        must.remove(hub)
    # the zero-sum witness: a short non-member row none of whose columns is a member except zcol
    zrow = zcol = -1
    for r in range(100, n_rows):
        cols = a.indices[a.indptr[r]:a.indptr[r + 1]]
        if 2 <= len(cols) <= 8 and r not in must and not set(cols.tolist()) & set(must) and r not in cols:
            zrow, zcol = r, int(cols[0])
            break
    assert zrow >= 0
    banned = set(a.indices[a.indptr[zrow]:a.indptr[zrow + 1]].tolist()) | {zrow}
    if not giant_row_inside:
        banned.add(hub)
    must.append(zcol)
    assert len(must) <= b
    rest = [i for i in rng.permutation(n_cols).tolist() if i not in banned and i not in must][:b - len(must)]
    ids = np.array(must + rest, np.int32)
    ids = ids[rng.permutation(len(ids))]
    assert len(set(ids.tolist())) == b
    return ids, zrow, zcol


def position_maps(g, ids):
    pos = np.full(g.n_cols, -1, np.int32)
    pos[ids] = np.arange(len(ids), dtype=np.int32)
    return pos, pos[:g.n_rows].copy()


@functools.lru_cache(maxsize=None)
def bwd1_case(kind, d, b, giant_row_inside=True):
    """operands of SPMM_BWD1S.  Every member's g_am is zero in the 16-byte piece 1 (floats 4..7); a third of the members have a g_am row
    that is exactly zero (zcol among them), another third are zero in the last piece as well"""
    g = graph(kind)
    seed = 1000 * d + b
    rng = np.random.RandomState(seed)
    ids, zrow, zcol = batch_for(g, b, seed, giant_row_inside)
    pos, pos_row = position_maps(g, ids)
    g_am_b = rng.randn(b, d).astype(np.float32)
    g_ax_b = rng.randn(b, d).astype(np.float32)
    g_am_b[:, 4:8] = 0
    if b > 1:
        g_am_b[0::3] = 0
        g_am_b[1::3, d - 4:] = 0
        g_am_b[pos[zcol]] = 0
    x_in = rng.randn(g.n_rows, d).astype(np.float32)
    ax = rng.randn(g.n_rows, d).astype(np.float32)
    return SimpleNamespace(g=g, d=d, b=b, ids=ids, zrow=zrow, zcol=zcol, pos=pos, pos_row=pos_row, g_am_b=g_am_b, g_ax_b=g_ax_b,
                           x_in=x_in, ax=ax)


def live_rows_of(case, extra=()):
    """the row bitmap a lazy step's forward marks: the member rows and every row with an entry in a member column (+ `extra` rows,
    which the contract allows: the set is an upper estimate)"""
    g = case.g
    member_col = case.pos >= 0
    hit = np.array([member_col[g.a.indices[g.a.indptr[r]:g.a.indptr[r + 1]]].any() for r in range(g.n_rows)])
    live = hit | (case.pos_row >= 0)
    live[list(extra)] = True
    return live


@functools.lru_cache(maxsize=None)
def bwd2_case(kind, d, b, limit=0):
    """operands of SPMM_BWD2S.  u is non-zero on a set Z of rows that straddles the word edges (0, 32, 63, n_cols - 1 inside; 31, 64
    outside); t is zero outside Z, as nzbits' contract demands, and on a few rows of Z too.  limit > 0: t and pos_row have `limit` rows"""
    g = graph(kind)
    seed = 2000 * d + b + limit
    rng = np.random.RandomState(seed)
    ids, _, _ = batch_for(g, b, seed)
    pos, pos_row = position_maps(g, ids)
    inside = rng.rand(g.n_cols) < 0.3
    inside[[0, 32, 63, g.n_cols - 1, g.hubs[0]]] = True
    inside[[31, 64]] = False
    u = rng.randn(g.n_cols, d).astype(np.float32) * inside[:, None]
    own = limit if limit > 0 else g.n_rows
    t = rng.randn(own, d).astype(np.float32) * inside[:own, None]
    t[np.flatnonzero(inside[:own])[::5]] = 0
    p = rng.randn(g.n_rows, d).astype(np.float32)
    res_b = rng.randn(b, d).astype(np.float32)
    return SimpleNamespace(g=g, d=d, b=b, ids=ids, pos_row=pos_row[:own].copy(), u=u, t=t, p=p, c=0.3, res_b=res_b, inside=inside,
                           limit=limit)


@functools.lru_cache(maxsize=None)
def fwd_case(kind, d, b):
    """operands of the filtered forward products: x is zero outside the rows of gather set Z (gather_bits' contract)"""
    g = graph(kind)
    seed = 3000 * d + b
    rng = np.random.RandomState(seed)
    ids, _, _ = batch_for(g, b, seed)
    rows = ids[ids < g.n_rows]
    row_pos = np.full(g.n_rows, -1, np.int32)
    row_pos[rows] = np.arange(len(rows), dtype=np.int32)
    inside = rng.rand(g.n_cols) < 0.4
    inside[[0, 32, 63, g.n_cols - 1]] = True
    inside[[31, 64]] = False
    x = rng.randn(g.n_cols, d).astype(np.float32)
    h = rng.randn(g.n_rows, d).astype(np.float32)
    return SimpleNamespace(g=g, d=d, b=b, ids=ids, rows=rows, row_pos=row_pos, x=x, xz=x * inside[:, None], h=h, inside=inside)


def split_by_column(a, c0):
    """the entries of every row split over two CSRs of the same shape: columns < c0, columns >= c0"""
    coo = a.tocoo()
    halves = []
    for mask in (coo.col < c0, coo.col >= c0):
        halves.append(_fp32(sp.csr_matrix((coo.data[mask], (coo.row[mask], coo.col[mask])), shape=a.shape)))
    return halves
