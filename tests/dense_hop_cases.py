"""Seeded inputs shared by tests/test_dense_hop_mirror.py (CPU) and tests/test_gpu_dense_hops.py (GPU): the graphs and DENSE operands
at which the dense backward modes of csrc/spmm.hip (SPMM_BWD1, SPMM_BWD2) are held to tests/sparse_hop_mirror.py.  The graphs are
those of sparse_hop_cases.py and one more, "rect_tail": the rectangular operand with a second long row behind every own-row limit the
tests use.  The operands are randn everywhere (a hub row of 1200 entries sums 1200 terms), with these planted: the graphs' empty rows,
a block of exactly-zero rows in the gathered operand, and in the pre-activation p the values at which elu' changes branch."""
import functools
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import sparse_hop_cases as K

WIDTHS = (16, 32, 48, 128, 256, 512, 1024)   # one per lane-group class of launch_balanced: 4, 8, 16, 32 lanes, 64 lanes x 1, 2, 4 float4
TAIL_ROW, TAIL_LEN = 850, 600                # rect_tail's second long row: behind the limits 577 and 600, several waves at every width
ZERO_BLOCK = slice(96, 160)                  # rows of the gathered operand (g_am / u) that are exactly zero
P_ROW, POS_ROW, NEG_ROW = 20, 21, 22         # rows of p with the planted values / all positive / all negative (and the hub row, and row 860)
P_PLANT = np.array([0.0, -0.0, np.finfo(np.float32).tiny, -20.0], np.float32)
KINDS = ("hub", "rect", "giant", "rect_tail")


def _one_pass_cases():
    """(mode, kind, d): every width with every graph kind once, the mode alternating so that every width meets both modes and every
    mode every kind; d = 1024 on hub and rect only"""
    out = []
    for wi, d in enumerate(WIDTHS):
        for ki, kind in enumerate(KINDS):
            if d == 1024 and kind not in ("hub", "rect"):
                continue
            out.append((("bwd1", "bwd2")[(wi + ki) % 2], kind, d))
    return out


ONE_PASS = _one_pass_cases()
BWD1_CASES = [(kind, d) for mode, kind, d in ONE_PASS if mode == "bwd1"]
# (kind, d, c): c alternates along the list
BWD2_CASES = [(kind, d, (1.0, 0.3)[i % 2]) for i, (kind, d) in enumerate((kind, d) for mode, kind, d in ONE_PASS if mode == "bwd2")]
# the second pass in place: (mode, kind, d); giant runs under spmm_giant = 64
TWO_PASS_CASES = [("bwd1", "hub", 16), ("bwd1", "rect", 128), ("bwd1", "giant", 48), ("bwd1", "hub", 256), ("bwd1", "rect", 1024),
                  ("bwd1", "giant", 512), ("bwd1", "rect", 32),
                  ("bwd2", "hub", 128), ("bwd2", "rect", 32), ("bwd2", "giant", 16), ("bwd2", "rect", 256), ("bwd2", "hub", 1024),
                  ("bwd2", "giant", 128), ("bwd2", "hub", 48), ("bwd2", "rect", 512)]
# own_row_limit < n_rows = 900: (kind, d, c, limit)
LIMIT_CASES = [("rect", 16, 0.3, 600), ("rect_tail", 128, 1.0, 600), ("rect_tail", 32, 0.3, 577), ("rect", 512, 1.0, 577),
               ("rect_tail", 256, 0.3, 600), ("rect_tail", 48, 1.0, 577)]
# feature slices: (d, spmm_slices, spmm_pin); bwd1 on hub, bwd2 on rect_tail under the limit 600, both with y_in in place
SLICE_CASES = [(48, 2, 1), (128, 2, 0), (128, 4, 1), (512, 4, 1), (512, 8, 0), (1024, 8, 1)]
SLICE_LIMIT = 600
SLICE_C = 0.3


def all_bwd1():
    """every (kind, d) whose SPMM_BWD1 operands a GPU test uses"""
    s = set(BWD1_CASES) | {(kind, d) for mode, kind, d in TWO_PASS_CASES if mode == "bwd1"} | {("hub", d) for d, _, _ in SLICE_CASES}
    return sorted(s)


def all_bwd2():
    """every (kind, d, c, limit) whose SPMM_BWD2 operands a GPU test uses"""
    s = {(kind, d, c, 0) for kind, d, c in BWD2_CASES} | set(LIMIT_CASES) | {("rect_tail", d, SLICE_C, SLICE_LIMIT) for d, _, _ in SLICE_CASES}
    s |= {(kind, d, two_pass_c(d), 0) for mode, kind, d in TWO_PASS_CASES if mode == "bwd2"}
    return sorted(s)


def two_pass_c(d):
    return 1.0 if d in (32, 128, 512) else 0.3


@functools.lru_cache(maxsize=None)
def graph(kind):
    """hub, rect, giant: sparse_hop_cases.graph.  rect_tail: rect + row TAIL_ROW holding TAIL_LEN entries -- with a limit of 600 or 577 a
    long row (and under spmm_giant = 64 a giant row) lies on each side of the limit: row 5 in front of it, row 850 behind"""
    if kind != "rect_tail":
        return K.graph(kind)
    base = K.graph("rect")
    rng = np.random.RandomState(7004)
    a = sp.lil_matrix(base.a.astype(np.float64))
    cols = np.sort(rng.choice(base.n_cols, TAIL_LEN, replace=False))
    a[TAIL_ROW, :] = 0
    a[TAIL_ROW, cols] = rng.uniform(0.1, 1.0, TAIL_LEN)
    g = SimpleNamespace(a=K._fp32(sp.csr_matrix(a)), hubs=base.hubs + (TAIL_ROW,), empty=base.empty, kind=kind)
    g.a.eliminate_zeros()
    g.a.sort_indices()
    g.n_rows, g.n_cols = g.a.shape
    g.lens = np.diff(g.a.indptr)
    assert g.lens[TAIL_ROW] == TAIL_LEN >= 200 and all(g.lens[r] == 0 for r in g.empty) and g.lens[base.hubs[0]] >= 1200
    return g


def _seed(kind, d, salt):
    return 100000 * salt + 10 * d + KINDS.index(kind)


@functools.lru_cache(maxsize=None)
def bwd1_case(kind, d):
    """dense operands of SPMM_BWD1: g_am [n_cols][d] with the rows ZERO_BLOCK exactly zero; g_ax, x_in, ax [n_rows][d]"""
    g = graph(kind)
    rng = np.random.RandomState(_seed(kind, d, 1))
    g_am = rng.randn(g.n_cols, d).astype(np.float32)
    g_am[ZERO_BLOCK] = 0
    g_ax = rng.randn(g.n_rows, d).astype(np.float32)
    x_in = rng.randn(g.n_rows, d).astype(np.float32)
    ax = rng.randn(g.n_rows, d).astype(np.float32)
    return SimpleNamespace(g=g, d=d, g_am=g_am, g_ax=g_ax, x_in=x_in, ax=ax)


def p_rows(g):
    """the rows of p that carry P_PLANT in their first four elements: a short row, the first hub row, a row behind every limit"""
    return (P_ROW, g.hubs[0], 860)


@functools.lru_cache(maxsize=None)
def bwd2_case(kind, d, limit=0):
    """dense operands of SPMM_BWD2: u [n_cols][d] with the rows ZERO_BLOCK exactly zero; p [n_rows][d] with +0.0, -0.0, the smallest
    positive normal and -20 planted in rows p_rows(g), row POS_ROW all positive, row NEG_ROW (and 861) all negative; t and res
    [n_rows][d], or exactly `limit` rows of them when limit > 0"""
    g = graph(kind)
    rng = np.random.RandomState(_seed(kind, d, 2) + limit)
    u = rng.randn(g.n_cols, d).astype(np.float32)
    u[ZERO_BLOCK] = 0
    own = limit if limit > 0 else g.n_rows
    t = rng.randn(own, d).astype(np.float32)
    res = rng.randn(own, d).astype(np.float32)
    p = rng.randn(g.n_rows, d).astype(np.float32)
    for r in p_rows(g):
        p[r, :4] = P_PLANT
    p[POS_ROW] = np.abs(p[POS_ROW]) + np.float32(0.01)
    for r in (NEG_ROW, 861):
        p[r] = -np.abs(p[r]) - np.float32(0.01)
    return SimpleNamespace(g=g, d=d, u=u, t=t, p=p, res=res, limit=limit)
