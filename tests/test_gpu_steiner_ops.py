"""-m gpu: gss_steiner_trees (csrc/steiner.hip) through the C entry point on the cases of tests/steiner_cases.py, against the mirror
(tests/steiner_mirror.py; tests/test_steiner_mirror.py holds the mirror to scipy, networkx and enumeration and shows what every case is
for).  Every output is an integer and both orders of the definition are total, so every comparison is an equality: the five counts,
the Steiner nodes with their parents and the bridges.  All outputs lie between guard rows that must come back untouched, list entries
past the counts keep the caller's value, and every call is made twice and must give the same bits.

No test provokes a fault: the refusals are host-side argument checks that launch nothing, or units the kernel flags before it walks a
row of theirs (a size outside the row, a seed that is no node, seeds out of order, a row longer than the bound given)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import steiner_cases as K  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, EINVAL, SENT = 2, -22, -77
COUNTS = ("n_comp", "length", "n_steiner", "n_edges", "max_w")
LISTS = ("steiner", "parent", "bridge")
OUT = COUNTS + LISTS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _error():
    return _lib.load().gss_last_error().decode()


_graphs = {}


def graph(c):
    key = id(c.rowptr)                                     # steiner_cases keeps one array per graph
    if key not in _graphs:
        _graphs[key] = (_dev(c.rowptr), _dev(c.col if len(c.col) else np.zeros(1, np.int32)))
    return _graphs[key]


def trees(c, seeds=None, sizes=None, null=(), **over):
    """-> (rc, {field: array}) of one call on case c; `over` replaces scalar arguments, `null` names the pointers passed as NULL.  The
    list buffers are exactly [U][max_add] and [U][max_size - 1][2] inside their guards (a dummy row where that is empty)"""
    lib = _lib.load()
    if seeds is None:
        seeds, sizes = K.seed_table(c)
    U, ms = seeds.shape
    max_add = over.get("max_add", c.max_add)
    rowptr, col = graph(c)
    ds, dz = _dev(seeds), _dev(sizes)
    width = {"steiner": max(max_add, 0), "parent": max(max_add, 0), "bridge": 2 * (ms - 1)}
    bufs = {f: torch.full((U + 2 * GUARD,), SENT, dtype=torch.int32, device="cuda") for f in COUNTS}
    bufs.update({f: torch.full(((U + 2 * GUARD) * max(width[f], 1),), SENT, dtype=torch.int32, device="cuda") for f in LISTS})
    ptrs = dict(rowptr=_lib.ptr(rowptr), col=_lib.ptr(col), seeds=_lib.ptr(ds), sizes=_lib.ptr(dz))
    ptrs.update({f: _lib.ptr(bufs[f][GUARD:]) for f in COUNTS})
    ptrs.update({f: _lib.ptr(bufs[f][GUARD * width[f]:]) if width[f] else None for f in LISTS})
    for k in null:
        ptrs[k] = None
    rc = lib.gss_steiner_trees(over.get("n", c.n), ptrs["rowptr"], ptrs["col"], over.get("max_deg", K.max_degree(c)), over.get("n_units", U),
                               over.get("max_size", ms), ptrs["seeds"], ptrs["sizes"], max_add, *(ptrs[f] for f in OUT), _lib.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(ds.cpu().numpy(), seeds) and np.array_equal(dz.cpu().numpy(), sizes)            # inputs left alone
    out = {}
    for f in OUT:
        h = bufs[f].cpu().numpy()
        per = 1 if f in COUNTS else max(width[f], 1)
        h = h.reshape(U + 2 * GUARD, per)
        assert (h[:GUARD] == SENT).all() and (h[GUARD + U:] == SENT).all(), f"a guard row of {f} was written"
        out[f] = h[GUARD:GUARD + U] if f in LISTS else h[GUARD:GUARD + U, 0]
    return rc, out


def same_bits(a, b):
    return all(a[f].dtype == b[f].dtype == np.int32 and np.array_equal(a[f], b[f]) for f in OUT)


def check(c, got, want, what, max_add=None):
    max_add = c.max_add if max_add is None else max_add
    for f in COUNTS:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5])
    for u in range(len(c.units)):
        k = min(len(want["steiner"][u]), max_add)
        for f in ("steiner", "parent"):
            assert np.array_equal(got[f][u, :k], want[f][u][:k]), (what, f, u)
            assert (got[f][u, k:] == SENT).all(), (what, f + " past the count", u)
        b = want["bridge"][u].ravel()
        assert np.array_equal(got["bridge"][u, :len(b)], b), (what, "bridge", u)
        assert (got["bridge"][u, len(b):] == SENT).all(), (what, "bridge past the count", u)


@pytest.mark.parametrize("name", K.CASES)
def test_trees_equal_the_mirror(name):
    c = K.case(name)
    want = K.mirror(name)
    rc, got = trees(c)
    assert rc == 0, _error()
    check(c, got, want, name)
    rc, again = trees(c)
    assert rc == 0 and same_bits(got, again), name
    rc, bare = trees(c, null=LISTS)                                             # the lists are optional: the null of random sets passes none
    assert rc == 0 and all(np.array_equal(bare[f], got[f]) for f in COUNTS) and all((bare[f] == SENT).all() for f in LISTS), name
    if len(c.units) <= 8 and max(len(u) for u in c.units) <= 1025:              # rows 7 longer, junk past every size
        seeds, sizes = K.seed_table(c, max(1, max(len(u) for u in c.units)) + 7, pad=0x7FFFFFFF)
        rc, wide = trees(c, seeds, sizes)
        assert rc == 0, _error()
        check(c, wide, want, name + " (wide)")
        rc, half = trees(c, null=("bridge",))                                   # one list without the other
        assert rc == 0 and all(np.array_equal(half[f], got[f]) for f in COUNTS + ("steiner", "parent")) and (half["bridge"] == SENT).all()
        rc, other = trees(c, null=("steiner", "parent"))
        assert rc == 0 and np.array_equal(other["bridge"], got["bridge"]) and (other["steiner"] == SENT).all()


def test_counts_stay_exact_past_max_add():
    c = K.case("capped")
    want = K.mirror("capped")
    for max_add in (0, 1, 2):
        rc, got = trees(c, max_add=max_add)
        assert rc == 0, _error()
        check(c, got, want, f"max_add={max_add}", max_add)
    assert (want["n_steiner"] > 2).all()


def test_one_call_and_three_calls_give_the_same_bits():
    c = K.case("n300")
    lib = _lib.load()
    seeds, sizes = K.seed_table(c)
    rc, whole = trees(c, seeds, sizes)
    assert rc == 0, _error()
    U, ms = seeds.shape
    rowptr, col = graph(c)
    ds, dz = _dev(seeds), _dev(sizes)
    bufs = {f: torch.full((U,), SENT, dtype=torch.int32, device="cuda") for f in COUNTS}
    bufs.update(steiner=torch.full((U, c.max_add), SENT, dtype=torch.int32, device="cuda"), parent=torch.full((U, c.max_add), SENT, dtype=torch.int32, device="cuda"),
                bridge=torch.full((U, 2 * (ms - 1)), SENT, dtype=torch.int32, device="cuda"))
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        rc = lib.gss_steiner_trees(c.n, _lib.ptr(rowptr), _lib.ptr(col), K.max_degree(c), hi - lo, ms, _lib.ptr(ds[lo:]), _lib.ptr(dz[lo:]),
                                   c.max_add, *(_lib.ptr(bufs[f][lo:]) for f in OUT), _lib.current_stream())
        assert rc == 0, _error()
    torch.cuda.synchronize()
    assert same_bits(whole, {f: bufs[f].cpu().numpy() for f in OUT})


def test_refusals_by_name_leave_nothing_behind():
    c = K.case("n40")
    seeds, sizes = K.seed_table(c)                         # five units in rows of six
    assert seeds.shape == (5, 6) and sizes.min() >= 2
    rc, kept = trees(c)
    assert rc == 0, _error()

    def with_unit(u, members=None, size=None, of=None):
        """the table (or the table `of` an earlier with_unit) with unit u replaced"""
        s2, z2 = (seeds.copy(), sizes.copy()) if of is None else (x.copy() for x in of.table)
        if members is not None:
            s2[u, :len(members)] = members
            z2[u] = len(members)
        if size is not None:
            z2[u] = size
        call = lambda: trees(c, s2, z2)[0]  # noqa: E731
        call.table = (s2, z2)
        return call

    md = K.max_degree(c)
    over = (K.LDS_BUDGET - 4 * c.n) // 16 + 1              # the first max_size whose 4 n + 16 max_size is over the budget at this n
    refusals = [(lambda k=k: trees(c, null=(k,))[0], "steiner_trees: null pointer") for k in ("rowptr", "col", "seeds", "sizes") + COUNTS]
    refusals += [
        (lambda: trees(c, null=("steiner",))[0], "steiner_trees: steiner and parent must both be given or both be NULL"),
        (lambda: trees(c, null=("parent",))[0], "steiner_trees: steiner and parent must both be given or both be NULL"),
        (lambda: trees(c, n=0)[0], "steiner_trees: n=0 n_units=5 must be >= 1"),
        (lambda: trees(c, n_units=0)[0], "steiner_trees: n=40 n_units=0 must be >= 1"),
        (lambda: trees(c, n=K.MAX_NODES + 1)[0], f"steiner_trees: n={K.MAX_NODES + 1} is over the limit of {K.MAX_NODES} nodes"),
        (lambda: trees(c, max_size=0)[0], "steiner_trees: max_size=0 must be in [1, 4096]"),
        (lambda: trees(c, max_size=K.MAX_SEEDS + 1)[0], "steiner_trees: max_size=4097 must be in [1, 4096]"),
        (lambda: trees(c, max_add=-1)[0], "steiner_trees: max_add=-1 must be >= 0"),
        (lambda: trees(c, max_deg=-1)[0], f"steiner_trees: max_deg=-1 must be in [0, {K.MAX_DEG}]"),
        (lambda: trees(c, max_deg=K.MAX_DEG + 1)[0], f"steiner_trees: max_deg={K.MAX_DEG + 1} must be in [0, {K.MAX_DEG}]"),
        (lambda: trees(c, n=K.MAX_NODES, max_size=2529)[0], "steiner_trees: 4 n + 16 max_size = 163344 bytes of LDS for n=30720, max_size=2529 is over the budget of 163328"),
        (lambda: trees(c, n=K.MAX_NODES, max_size=K.MAX_SEEDS)[0], "bytes of LDS for n=30720, max_size=4096 is over the budget"),
        (lambda: trees(c, n_units=1 << 38)[0], "steiner_trees: the tables are too large"),
        (lambda: trees(c, max_deg=md - 1)[0], f"steiner_trees: a row of the CSR is longer than max_deg={md - 1}"),
        (with_unit(1, size=7), "steiner_trees: a unit's size is outside [0, max_size=6]"),
        (with_unit(2, size=-1), "steiner_trees: a unit's size is outside [0, max_size=6]"),
        (with_unit(0, members=[0, 10, c.n]), f"steiner_trees: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[-1, 20, 30]), f"steiner_trees: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[10, 20, 20]), "steiner_trees: a unit's seeds are not strictly ascending"),
        (with_unit(2, members=[30, 20]), "steiner_trees: a unit's seeds are not strictly ascending"),
        # several bad units in one call: the refusal is the lowest bit's, whichever unit set it
        (with_unit(2, members=[0, 10, c.n], of=with_unit(0, members=[30, 20])), f"steiner_trees: a seed is not a node index in [0, {c.n})"),
        (with_unit(2, size=7, of=with_unit(1, members=[30, 20], of=with_unit(0, members=[0, 10, c.n]))),
         "steiner_trees: a unit's size is outside [0, max_size=6]"),
    ]
    assert 4 * c.n + 16 * over > K.LDS_BUDGET >= 4 * c.n + 16 * (over - 1) and over > K.MAX_SEEDS     # at n = 40 the bound on max_size comes first
    for call, words in refusals:
        assert call() == EINVAL, words
        assert words in _error(), (words, _error())
        rc, again = trees(c)
        assert rc == 0 and same_bits(kept, again), words
