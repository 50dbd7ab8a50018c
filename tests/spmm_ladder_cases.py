"""Seeded inputs shared by tests/test_spmm_ladder_cases.py (CPU) and tests/test_gpu_spmm_ladder.py (GPU): two graphs whose rows reach every
block class of the balanced SpMM's schedule (csrc/segments.h) at every lane-group width, operands that make every sum EXACT in fp32, the
integer references, and a Python restatement of the schedule's placement rule.

The ladder graph.  n_rows x 8320, rectangular as a shard's operand is (halo columns behind the own ones).  Every length of
LADDER_LENGTHS twice -- one below, on and above every power of two of segments from 1 to 256, and a full row --, the lengths of
EXTRA_LENGTHS once (48: it makes the number of two-group blocks odd, so that at four groups per wave one wave holds a two-group block
beside one-group blocks; 80 and 81: five chunks exactly and five chunks + 1 entry under spmm_giant = 64), N_FILLER rows of 0..9 entries,
all in a seeded permuted order, between an empty first row, a run of three empty rows and an empty last row.  Columns distinct and sorted.

The packed graph.  256 rows of exactly 32 entries over 1000 columns: one descriptor per row and a descriptor count that every workgroup
size divides, so the list ends without a `row = -1` padding descriptor at every width (the ladder's last workgroup is padded at every width).

Exactness.  Values of A are 1, 2, 3; every operand is an integer in [-4, 4] held as float32 (the pre-activation p: an integer in [1, 4],
so that elu' = 1; c = 0.5).  Every partial sum of every mode, in any order, contracted or not, is an integer of magnitude at most
8320 * 3 * 4 * 4 + 8 < 2^24 (dp: a multiple of 0.5 below 2^23), hence exact in fp32: a kernel that sums every stored entry once -- in ANY
order -- returns the reference to the last bit, and one that drops or doubles a single partial sum does not.  The one exception is
planted: on the rows plant_rows(g) p starts with dense_hop_cases.P_PLANT (+0, -0, the smallest normal, -20); expf(-20) is not exact, so dp
on those rows is held to sparse_hop_mirror.bound, as the other hop suites do.  (Signed zeros: a sum that is zero is +0, a product with a
negative factor may be -0; the comparisons are on values, -0 == +0, and NaN -- the pre-fill -- equals nothing.)

The references are scipy products over int64 copies of the operands (dp in fp64: halves), independent of any project code.

schedule() restates the placement rule of csrc/segments.h (build_segments_items, giant_items) so that the cases can assert what they
claim about themselves -- which block classes they reach, where a block holds an empty segment, which wave mixes block sizes -- and so
that a failing comparison can name the block class of its rows.  It checks nothing about the C++: tests/native/segments_check.cpp
(run by tests/test_native_host.py) is what checks the descriptors themselves."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

from dense_hop_cases import P_PLANT

N_COLS = 8320
LADDER_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049,
                  4095, 4096, 4097, 8191, 8192, 8193, 8320)
EXTRA_LENGTHS = (48, 80, 81)
N_FILLER = 300
PACKED_ROWS, PACKED_COLS, PACKED_LEN = 256, 1000, 32
WIDTHS = (16, 32, 48, 64, 128, 256, 512, 1024)    # 16, 8, 4, 4, 2 groups per wave; one group of 64 lanes x 1, 2, 4 float4
SEG_EDGES, WAVES = 32, 16                         # gss_csr::seg_edges, kBalWaves
C = 0.5
CLASS_LENGTHS = (1, 33, 65, 129, 257, 513, 1025, 2049, 4097, 8193, 8320)   # one length per uncapped log2 p = 0 .. 8, and the two longest
GIANT = 64                                        # spmm_giant of the chunked runs: chunks of 16 entries
KINDS = ("ladder", "packed")


# ---------------------------------------------------------------- the graphs
def _csr(lens, n_cols, rng):
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([np.sort(rng.choice(n_cols, int(k), replace=False)) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    data = rng.choice(np.array([1.0, 2.0, 3.0], np.float32), len(indices)).astype(np.float32)
    return sp.csr_matrix((data, indices, indptr), shape=(len(lens), n_cols))


@functools.lru_cache(maxsize=None)
def graph(kind):
    if kind == "ladder":
        rng = np.random.RandomState(8101)
        lens = np.array([k for k in LADDER_LENGTHS for _ in range(2)] + list(EXTRA_LENGTHS) + list(rng.randint(0, 10, N_FILLER)))
        lens = lens[rng.permutation(len(lens))]
        half = len(lens) // 2
        lens = np.concatenate([[0], lens[:half], [0, 0, 0], lens[half:], [0]])
        g = SimpleNamespace(a=_csr(lens, N_COLS, rng), empty_run=(half + 1, half + 2, half + 3))
    elif kind == "packed":
        rng = np.random.RandomState(8102)
        g = SimpleNamespace(a=_csr(np.full(PACKED_ROWS, PACKED_LEN), PACKED_COLS, rng), empty_run=())
    else:
        raise KeyError(kind)
    g.kind = kind
    g.n_rows, g.n_cols = g.a.shape
    g.lens = np.diff(g.a.indptr)
    # rank of a row among the rows of its own length: the row filters keep the even ranks -- of two copies of a length the first
    g.rank = np.zeros(g.n_rows, np.int64)
    for k in np.unique(g.lens):
        rows = np.flatnonzero(g.lens == k)
        g.rank[rows] = np.arange(len(rows))
    g.keep = g.rank % 2 == 0
    return g


def rows_of_length(g, k):
    """the rows of that length, in row order (a ladder length: two of them, or more where the filler rows have it too)"""
    return np.flatnonzero(g.lens == k)


def a_int(a):
    return sp.csr_matrix((a.data.astype(np.int64), a.indices, a.indptr), shape=a.shape)


@functools.lru_cache(maxsize=None)
def halves(kind):
    """the entries of every row split over two CSRs of the same shape: columns < n_cols // 3, columns >= n_cols // 3"""
    g = graph(kind)
    coo = g.a.tocoo()
    out = []
    for mask in (coo.col < g.n_cols // 3, coo.col >= g.n_cols // 3):
        h = sp.csr_matrix((coo.data[mask], (coo.row[mask], coo.col[mask])), shape=g.a.shape)
        h.sort_indices()
        out.append(sp.csr_matrix((h.data.astype(np.float32), h.indices.astype(np.int32), h.indptr.astype(np.int32)), shape=g.a.shape))
    assert out[0].nnz + out[1].nnz == g.a.nnz
    return tuple(out)


def part(kind, which):
    return graph(kind).a if which == "all" else halves(kind)[("first", "second").index(which)]


# ---------------------------------------------------------------- the operands: integers in [-4, 4] as float32
_GATHERED = ("x0", "x1")                               # [n_cols][d]: the operand a mode gathers from
_BY_ROW = ("h", "g_ax", "x_in", "ax", "t", "res", "h1")      # [n_rows][d]: the epilogues' operands
PLANT_LENGTHS = (2, 129, 4097)


def plant_rows(g):
    """the rows whose p starts with P_PLANT: a short row, a row of several segments, a row of many waves (ladder); rows 7 and 200 (packed)"""
    if g.kind == "packed":
        return (7, 200)
    return tuple(int(rows_of_length(g, k)[0]) for k in PLANT_LENGTHS)


@functools.lru_cache(maxsize=None)
def operand(kind, d, name):
    g = graph(kind)
    names = _GATHERED + _BY_ROW + ("p",)
    rng = np.random.RandomState(8200 + 1000 * KINDS.index(kind) + 17 * d + names.index(name))
    if name == "p":
        p = rng.randint(1, 5, (g.n_rows, d)).astype(np.float32)
        for r in plant_rows(g):
            p[r, :4] = P_PLANT
        return p
    return rng.randint(-4, 5, (g.n_cols if name in _GATHERED else g.n_rows, d)).astype(np.float32)


def _i(x):
    return np.asarray(x).astype(np.int64)


@functools.lru_cache(maxsize=None)
def product(kind, d, name, which="all"):
    """A x over int64, by scipy: [n_rows][d].  name: a gathered operand, or one of the masked ones of the sparse cases below"""
    x = operand(kind, d, name) if name in _GATHERED else masked_operand(kind, d, name)
    return np.asarray(a_int(part(kind, which)) @ _i(x))


def elu_grad64(p):
    p = p.astype(np.float64)
    return np.where(p > 0, 1.0, np.exp(np.minimum(p, 0.0)))


Ref = SimpleNamespace


@functools.lru_cache(maxsize=None)
def fwd_ref(kind, d, x="x0", h="h"):
    """SPMM_PLAIN / SPMM_FWD1: y = A x, m = y (.) h"""
    y = product(kind, d, x)
    return Ref(y=y, m=y * _i(operand(kind, d, h)))


@functools.lru_cache(maxsize=None)
def bwd1_ref(kind, d):
    """SPMM_BWD1 gathering x1: dm = A g_am, u = g_ax + dm (.) x_in, t = dm (.) ax"""
    dm = product(kind, d, "x1")
    return Ref(u=_i(operand(kind, d, "g_ax")) + dm * _i(operand(kind, d, "x_in")), t=dm * _i(operand(kind, d, "ax")))


def _dp(kind, d, gx, res, s_sum, k):
    """dp = c gx (.) elu'(p) + res in fp64 (exact: halves), the magnitude S of the same expression and the row's term count k"""
    eg = elu_grad64(operand(kind, d, "p"))
    dp = C * gx * eg + res
    s = C * s_sum * eg + np.abs(res)
    return dp, s, k


@functools.lru_cache(maxsize=None)
def bwd2_ref(kind, d, res=True, two_pass=False):
    """SPMM_BWD2 gathering x0: gx = t + A u, dp = c gx (.) elu'(p) (+ res).  s_dp, k: what sparse_hop_mirror.bound takes on the planted
    rows -- the expression over absolute values (two_pass: the first pass's sum enters as ONE term, |y_in|, as in the mirror)"""
    g = graph(kind)
    t = _i(operand(kind, d, "t"))
    gx = t + product(kind, d, "x0")
    r = _i(operand(kind, d, "res")).astype(np.float64) if res else np.zeros((g.n_rows, d))
    ax = np.abs(_i(operand(kind, d, "x0")))
    if two_pass:
        s_sum = np.abs(product(kind, d, "x0", "first")) + np.asarray(a_int(part(kind, "second")) @ ax)
        k = np.diff(part(kind, "second").indptr) + 1
    else:
        s_sum = np.asarray(a_int(g.a) @ ax)
        k = g.lens
    dp, s_dp, k = _dp(kind, d, gx.astype(np.float64), r, (np.abs(t) + s_sum).astype(np.float64), k)
    return Ref(gx=gx, dp=dp, s_dp=s_dp, k=k)


# ---------------------------------------------------------------- the sparse cases: a batch of about 40 ids
@functools.lru_cache(maxsize=None)
def batch(kind):
    """distinct column ids in compact order.  Ladder: as MEMBERS (ids below n_rows are output rows too) one row of every length of
    CLASS_LENGTHS -- a row of every block class at every width --, the empty rows 0 and n_rows - 1, the bitmap word edges 31, 32, 63, 64;
    as COLUMNS the first and last entry of each of those rows and the middle entry of the other row of the same length, so that rows of
    every block class meet a member in their first and in their last segment (the longest rows meet nearly all of them)"""
    g = graph(kind)
    a = g.a
    rng = np.random.RandomState(8300 + KINDS.index(kind))
    ids = [0, g.n_rows - 1, 31, 32, 63, 64]
    if kind == "ladder":
        for k in CLASS_LENGTHS:
            r0, r1 = rows_of_length(g, k)[:2]
            ids += [int(r0), int(a.indices[a.indptr[r0]]), int(a.indices[a.indptr[r0 + 1] - 1]), int(a.indices[a.indptr[r1] + k // 2])]
    else:
        ids += [int(a.indices[a.indptr[r] + 5]) for r in (1, 100, 255)] + [int(c) for c in rng.permutation(g.n_cols)[:30]]
    ids = np.array(list(dict.fromkeys(ids)), np.int32)
    return ids[rng.permutation(len(ids))]


@functools.lru_cache(maxsize=None)
def inside(kind):
    """the set Z of SPMM_BWD2S's non-zero-row bitmap and of the gather filter: a third of the columns, straddling the word edges"""
    g = graph(kind)
    z = np.random.RandomState(8400 + KINDS.index(kind)).rand(g.n_cols) < 0.33
    z[[0, 32, 63, g.n_cols - 1]] = True
    z[[31, 64]] = False
    return z


@functools.lru_cache(maxsize=None)
def masked_operand(kind, d, name):
    """x0z: x0 with the rows outside Z zeroed (nzbits' / gather_bits' contract); tz: t likewise, over the rows.
    g_am_full: the compact g_am_b of the batch scattered over [n_cols][d]"""
    g = graph(kind)
    if name == "x0z":
        return operand(kind, d, "x0") * inside(kind)[:, None]
    if name == "tz":
        return operand(kind, d, "t") * inside(kind)[:g.n_rows, None]
    if name == "g_am_full":
        cs = bwd1s_case(kind, d)
        full = np.zeros((g.n_cols, d), np.float32)
        full[cs.ids] = cs.g_am_b
        return full
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def bwd1s_case(kind, d):
    """operands of SPMM_BWD1S: compact g_am_b (every fifth member's row exactly zero), g_ax_b; pos over the columns, pos_row over the
    rows; live: the bitmap a lazy step's forward marks -- members, rows with an entry in a member column -- and two rows more"""
    g = graph(kind)
    ids = batch(kind)
    rng = np.random.RandomState(8500 + d)
    g_am_b = rng.randint(-4, 5, (len(ids), d)).astype(np.float32)
    g_am_b[0::5] = 0
    g_ax_b = rng.randint(-4, 5, (len(ids), d)).astype(np.float32)
    pos = np.full(g.n_cols, -1, np.int32)
    pos[ids] = np.arange(len(ids), dtype=np.int32)
    pos_row = pos[:g.n_rows].copy()
    hit = np.asarray(a_int(g.a)[:, np.sort(ids)].getnnz(axis=1)) > 0
    live = hit | (pos_row >= 0)
    live[[1, g.n_rows - 2]] = True
    return SimpleNamespace(g=g, d=d, ids=ids, g_am_b=g_am_b, g_ax_b=g_ax_b, pos=pos, pos_row=pos_row, live=live)


@functools.lru_cache(maxsize=None)
def bwd1s_ref(kind, d):
    """dm = the sum over the entries in member columns; u = dm (.) x_in (+ g_ax_b on member rows); t = dm (.) ax;
    nz = member rows and rows with a non-zero dm: the bits of nzbits_out and, under skip_zero_rows, the write set"""
    cs = bwd1s_case(kind, d)
    dm = product(kind, d, "g_am_full")
    u = dm * _i(operand(kind, d, "x_in"))
    member = cs.pos_row >= 0
    u[member] += _i(cs.g_ax_b)[cs.pos_row[member]]
    return Ref(u=u, t=dm * _i(operand(kind, d, "ax")), nz=member | (dm != 0).any(1))


@functools.lru_cache(maxsize=None)
def bwd2s_ref(kind, d, two_pass=False):
    """SPMM_BWD2S gathering x0z with t = tz and the residual held compactly on the member rows"""
    g = graph(kind)
    ids = batch(kind)
    res_b = np.random.RandomState(8600 + d).randint(-4, 5, (len(ids), d)).astype(np.float32)
    pos_row = np.full(g.n_cols, -1, np.int32)
    pos_row[ids] = np.arange(len(ids), dtype=np.int32)
    pos_row = pos_row[:g.n_rows].copy()
    t = _i(masked_operand(kind, d, "tz"))
    gx = t + product(kind, d, "x0z")
    res = np.zeros((g.n_rows, d))
    res[pos_row >= 0] = res_b[pos_row[pos_row >= 0]]
    ax = np.abs(_i(masked_operand(kind, d, "x0z")))
    if two_pass:
        s_sum = np.abs(product(kind, d, "x0z", "first")) + np.asarray(a_int(part(kind, "second")) @ ax)
        k = np.diff(part(kind, "second").indptr) + 1
    else:
        s_sum = np.asarray(a_int(g.a) @ ax)
        k = g.lens
    dp, s_dp, k = _dp(kind, d, gx.astype(np.float64), res, (np.abs(t) + s_sum).astype(np.float64), k)
    return Ref(gx=gx, dp=dp, s_dp=s_dp, k=k, res_b=res_b, pos_row=pos_row)


def all_references(kind, d):
    """every reference array of (kind, d), by name: what the exactness premise is asserted over"""
    out = {}
    for name, ref, fields in (("fwd", fwd_ref(kind, d), ("y", "m")), ("fwd x1", fwd_ref(kind, d, "x1", "h1"), ("y", "m")),
                              ("bwd1", bwd1_ref(kind, d), ("u", "t")), ("bwd2", bwd2_ref(kind, d), ("gx", "dp")),
                              ("bwd2 no res", bwd2_ref(kind, d, res=False), ("dp",)), ("bwd1s", bwd1s_ref(kind, d), ("u", "t")),
                              ("bwd2s", bwd2s_ref(kind, d), ("gx", "dp")), ("gather", Ref(y=product(kind, d, "x0z")), ("y",))):
        for f in fields:
            out[f"{name} {f}"] = getattr(ref, f)
    return out


# ---------------------------------------------------------------- the placement rule of csrc/segments.h, restated
def gpw_log2_of(d, slices=1):
    """log2 of the lane groups per wave launch_balanced gives a product of width d cut into `slices` feature slices"""
    ds = d // 4 // slices
    return 4 if ds <= 4 else 3 if ds <= 8 else 2 if ds <= 16 else 1 if ds <= 32 else 0


def schedule(lens, gpw_log2):
    """build_segments_items over items of these lengths (item i = row i).  Per item, indexed by ROW: plog; p = 2^plog lane groups;
    waves = waves per block (1 when the block fits a wave); group0 = its first lane group, counted over the whole list; wg, wave = the
    workgroup and the list-wide wave of group0; per = entries per segment; n_empty = segments of the block without an entry (0 for an
    empty row: its one segment IS the row); whole = the row takes the whole workgroup with segments longer than SEG_EDGES.
    n_groups, n_blocks, padding: descriptors in use, workgroups, `row = -1` descriptors behind the last block.
    multi[wg]: the workgroup carries the 0x100 flag (some block of it spans more than one wave)."""
    lens = np.asarray(lens, np.int64)
    gpw = 1 << gpw_log2
    ngb = WAVES * gpw
    ngb_log2 = 4 + gpw_log2
    sgm = np.where(lens <= SEG_EDGES, 1, -(-lens // SEG_EDGES))
    plog = np.minimum(np.ceil(np.log2(sgm)).astype(np.int64), ngb_log2)
    assert ((1 << plog) >= np.minimum(sgm, ngb)).all() and ((plog == 0) | ((1 << (plog - 1)) < sgm)).all()
    order = np.lexsort((-lens, -plog))            # stable: by non-increasing plog, then non-increasing length, then row order
    p_sorted = 1 << plog[order]
    group0 = np.zeros(len(lens), np.int64)
    group0[order] = np.cumsum(p_sorted) - p_sorted
    p = 1 << plog
    assert (group0 % p == 0).all()                # aligned blocks
    per = -(-lens // p)
    n_empty = np.where(lens > 0, p - -(-lens // np.maximum(per, 1)), 0)
    n_groups = int(p.sum())
    n_blocks = -(-n_groups // ngb)
    wg = group0 // ngb
    assert ((group0 + p - 1) // ngb == wg).all()  # a block never straddles two workgroups
    multi = np.zeros(max(n_blocks, 1), bool)
    multi[wg[p > gpw]] = True
    return SimpleNamespace(gpw_log2=gpw_log2, gpw=gpw, ngb=ngb, ngb_log2=ngb_log2, lens=lens, plog=plog, p=p, waves=np.maximum(1, p // gpw),
                           group0=group0, wg=wg, wave=group0 // gpw, per=per, n_empty=n_empty, whole=sgm > ngb, n_groups=n_groups,
                           n_blocks=n_blocks, padding=n_blocks * ngb - n_groups, multi=multi)


def mixed_waves(s):
    """the list-wide waves that hold blocks of two different sizes (blocks smaller than a wave: the others fill their waves)"""
    small = np.flatnonzero(s.p < s.gpw)
    sizes = {}
    for i in small:
        sizes.setdefault(int(s.wave[i]), set()).add(int(s.p[i]))
    return sorted(w for w, ps in sizes.items() if len(ps) > 1)


def mixed_workgroups(s):
    """the workgroups that hold a block of several waves beside a block inside one wave"""
    return sorted(set(s.wg[s.p > s.gpw].tolist()) & set(s.wg[s.p <= s.gpw].tolist()))


def giant_items(lens, thr):
    """giant_items of csrc/segments.h: rows above thr entries are cut into chunks of thr / 4.  -> the lengths of the short pass's items
    (every other row), of the chunk pass's items (the chunks) and of the finish pass's items (chunks per giant row), and the giant rows"""
    lens = np.asarray(lens, np.int64)
    chunk = max(thr // 4, 1)
    giant = np.flatnonzero(lens > thr)
    chunks = np.concatenate([np.minimum(chunk, k - np.arange(0, k, chunk)) for k in lens[giant]] + [np.zeros(0, np.int64)])
    finish = -(-lens[giant] // chunk)
    assert chunks.sum() == lens[giant].sum() and len(chunks) == finish.sum()
    return SimpleNamespace(short=lens[lens <= thr], chunks=chunks, finish=finish, rows=giant)


def describe(lens, rows, gpw_log2, limit=6):
    """for an assertion's message: the listed rows' lengths and block class at this width"""
    s = schedule(lens, gpw_log2)
    rows = np.asarray(rows).reshape(-1)
    txt = [f"row {r}: {int(s.lens[r])} entries, plog {int(s.plog[r])}, {int(s.waves[r])} wave(s) per block, {int(s.n_empty[r])} empty segment(s)"
           + (", whole workgroup" if s.whole[r] else "") for r in rows[:limit]]
    return f"{len(rows)} row(s) at {s.gpw} group(s) per wave -- " + "; ".join(txt) + (" ..." if len(rows) > limit else "")
