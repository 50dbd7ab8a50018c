"""-m gpu: gss_seed_connectors (csrc/seed_connect.hip) through the C entry point on the cases of tests/connectors_cases.py, against the
mirror (tests/connectors_mirror.py; tests/test_connectors_mirror.py holds the mirror to a brute-force scipy oracle and to networkx and
shows what every case is for).  Every output is an integer and the key of the choice is a total order, so every comparison is an
equality: the step outputs, the per-unit summaries and the labels.  All ten outputs lie between guard rows that must come back
untouched, label entries past size + steps keep the caller's value, and every call is made twice and must give the same bits.

No test provokes a fault: the refusals are host-side argument checks that launch nothing, or units the kernel flags before it walks a
row of theirs (a size outside the row, a seed that is no node, seeds out of order, a row longer than the bound given)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import connectors_cases as K  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, EINVAL, SENT = 2, -22, -77
STEP = ("node", "lcc", "merged", "deg")
UNIT = ("steps", "first_lcc", "final_lcc", "seeds_in", "added_in")
OUT = STEP + UNIT + ("label",)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _error():
    return _lib.load().gss_last_error().decode()


_graphs = {}


def graph(c):
    key = (c.n, len(c.col))
    if key not in _graphs:
        _graphs[key] = (_dev(c.rowptr), _dev(c.col if len(c.col) else np.zeros(1, np.int32)))
    return _graphs[key]


def grow(c, seeds=None, sizes=None, null=None, **over):
    """-> (rc, {field: array}) of one call on case c; `over` replaces scalar arguments, `null` names a pointer passed as NULL"""
    lib = _lib.load()
    if seeds is None:
        seeds, sizes = K.seed_table(c)
    U, ms = seeds.shape
    n_add = over.get("n_add", c.n_add)
    rows = max(n_add, 1)
    rowptr, col = graph(c)
    ds, dz = _dev(seeds), _dev(sizes)
    shape = {f: (U + 2 * GUARD, rows) for f in STEP}
    shape.update({f: (U + 2 * GUARD,) for f in UNIT})
    shape["label"] = (U + 2 * GUARD, ms + rows)
    bufs = {f: torch.full(shape[f], SENT, dtype=torch.int32, device="cuda") for f in OUT}
    ptrs = dict(rowptr=_lib.ptr(rowptr), col=_lib.ptr(col), seeds=_lib.ptr(ds), sizes=_lib.ptr(dz))
    ptrs.update({f: _lib.ptr(bufs[f][GUARD:]) for f in OUT})
    if null:
        ptrs[null] = None
    rc = lib.gss_seed_connectors(over.get("n", c.n), ptrs["rowptr"], ptrs["col"], over.get("max_deg", K.max_degree(c)), over.get("n_units", U),
                                 over.get("max_size", ms), ptrs["seeds"], ptrs["sizes"], n_add, *(ptrs[f] for f in OUT), _lib.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(ds.cpu().numpy(), seeds) and np.array_equal(dz.cpu().numpy(), sizes)            # inputs left alone
    out = {}
    for f in OUT:
        h = bufs[f].cpu().numpy()
        assert (h[:GUARD] == SENT).all() and (h[GUARD + U:] == SENT).all(), f"a guard row of {f} was written"
        out[f] = h[GUARD:GUARD + U]
    return rc, out


def same_bits(a, b):
    return all(a[f].dtype == b[f].dtype == np.int32 and np.array_equal(a[f], b[f]) for f in OUT)


def check(got, want, what):
    for f in STEP + UNIT:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5])
    for u, label in enumerate(want["label"]):
        assert np.array_equal(got["label"][u, :len(label)], label), (what, "label", u)
        assert (got["label"][u, len(label):] == SENT).all(), (what, "label past size + steps", u)


@pytest.mark.parametrize("name", K.CASES)
def test_growth_equals_the_mirror(name):
    c = K.case(name)
    want = K.mirror(name)
    rc, got = grow(c)
    assert rc == 0, _error()
    check(got, want, name)
    rc, again = grow(c)
    assert rc == 0 and same_bits(got, again), name
    if len(c.units) <= 8:                                                      # rows 7 longer, junk past every size
        seeds, sizes = K.seed_table(c, max(1, max(len(u) for u in c.units)) + 7, pad=0x7FFFFFFF)
        rc, wide = grow(c, seeds, sizes)
        assert rc == 0, _error()
        check(wide, want, name + " (wide)")
        rc, bare = grow(c, null="label")                                       # the labels are optional
        assert rc == 0 and all(np.array_equal(bare[f], got[f]) for f in STEP + UNIT) and (bare["label"] == SENT).all()


def test_the_fill_after_the_stop_is_exact():
    rc, got = grow(K.case("odd"))
    assert rc == 0, _error()
    assert got["node"][0].tolist() == [2] + [-1] * 9 and got["lcc"][0].tolist() == [3] + [0] * 9
    for u, first in ((0, 1), (1, 0), (4, 0), (5, 0), (6, 0)):
        assert (got["node"][u, first:] == -1).all() and all((got[f][u, first:] == 0).all() for f in ("lcc", "merged", "deg"))
    assert got["steps"].tolist() == [1, 0, 1, 0, 0, 0, 0] and got["final_lcc"].tolist() == [3, 1, 3, 1, 0, 6, 10]


def test_one_call_and_three_calls_give_the_same_bits():
    c = K.case("n300")
    lib = _lib.load()
    seeds, sizes = K.seed_table(c)
    rc, whole = grow(c, seeds, sizes)
    assert rc == 0, _error()
    U, ms = seeds.shape
    rowptr, col = graph(c)
    ds, dz = _dev(seeds), _dev(sizes)
    bufs = {f: torch.full((U, c.n_add), SENT, dtype=torch.int32, device="cuda") for f in STEP}
    bufs.update({f: torch.full((U,), SENT, dtype=torch.int32, device="cuda") for f in UNIT})
    bufs["label"] = torch.full((U, ms + c.n_add), SENT, dtype=torch.int32, device="cuda")
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        rc = lib.gss_seed_connectors(c.n, _lib.ptr(rowptr), _lib.ptr(col), K.max_degree(c), hi - lo, ms, _lib.ptr(ds[lo:]), _lib.ptr(dz[lo:]),
                                     c.n_add, *(_lib.ptr(bufs[f][lo:]) for f in OUT), _lib.current_stream())
        assert rc == 0, _error()
    torch.cuda.synchronize()
    assert same_bits(whole, {f: bufs[f].cpu().numpy() for f in OUT})


def test_refusals_by_name_leave_nothing_behind():
    c = K.case("n40")
    seeds, sizes = K.seed_table(c)                         # five units in rows of six
    assert seeds.shape == (5, 6) and sizes.min() >= 2
    rc, kept = grow(c)
    assert rc == 0, _error()

    def with_unit(u, members=None, size=None, of=None):
        """the table (or the table `of` an earlier with_unit) with unit u replaced"""
        s2, z2 = (seeds.copy(), sizes.copy()) if of is None else (x.copy() for x in of.table)
        if members is not None:
            s2[u, :len(members)] = members
            z2[u] = len(members)
        if size is not None:
            z2[u] = size
        call = lambda: grow(c, s2, z2)[0]  # noqa: E731
        call.table = (s2, z2)
        return call

    md = K.max_degree(c)
    refusals = [(lambda k=k: grow(c, null=k)[0], "seed_connectors: null pointer") for k in ("rowptr", "col", "seeds", "sizes") + STEP + UNIT]
    refusals += [
        (lambda: grow(c, n_add=0)[0], "seed_connectors: n_add=0 must be >= 1"),
        (lambda: grow(c, n=0)[0], "seed_connectors: n=0 n_units=5 must be >= 1"),
        (lambda: grow(c, n_units=0)[0], "seed_connectors: n=40 n_units=0 must be >= 1"),
        (lambda: grow(c, n=K.MAX_NODES + 1)[0], f"seed_connectors: n={K.MAX_NODES + 1} is over the limit of {K.MAX_NODES} nodes"),
        (lambda: grow(c, max_size=0)[0], "seed_connectors: max_size=0 must be in [1, 4096]"),
        (lambda: grow(c, max_size=K.MAX_SEEDS + 1)[0], "seed_connectors: max_size=4097 must be in [1, 4096]"),
        (lambda: grow(c, max_size=K.MAX_SEEDS, n_add=K.MAX_MEMBERS - K.MAX_SEEDS + 1)[0], "seed_connectors: max_size=4096 + n_add=4097 is over 8192"),
        (lambda: grow(c, max_deg=-1)[0], f"seed_connectors: max_deg=-1 must be in [0, {K.MAX_DEG}]"),
        (lambda: grow(c, max_deg=K.MAX_DEG + 1)[0], f"seed_connectors: max_deg={K.MAX_DEG + 1} must be in [0, {K.MAX_DEG}]"),
        (lambda: grow(c, n_units=1 << 38)[0], "seed_connectors: the tables are too large"),
        (lambda: grow(c, max_deg=md - 1)[0], f"seed_connectors: a row of the CSR is longer than max_deg={md - 1}"),
        (with_unit(1, size=7), "seed_connectors: a unit's size is outside [0, max_size=6]"),
        (with_unit(2, size=-1), "seed_connectors: a unit's size is outside [0, max_size=6]"),
        (with_unit(0, members=[0, 10, c.n]), f"seed_connectors: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[-1, 20, 30]), f"seed_connectors: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[10, 20, 20]), "seed_connectors: a unit's seeds are not strictly ascending"),
        (with_unit(2, members=[30, 20]), "seed_connectors: a unit's seeds are not strictly ascending"),
        # several bad units in one call: the refusal is the lowest bit's, whichever unit set it
        (with_unit(2, members=[0, 10, c.n], of=with_unit(0, members=[30, 20])), f"seed_connectors: a seed is not a node index in [0, {c.n})"),
        (with_unit(2, size=7, of=with_unit(1, members=[30, 20], of=with_unit(0, members=[0, 10, c.n]))),
         "seed_connectors: a unit's size is outside [0, max_size=6]"),
    ]
    for call, words in refusals:
        assert call() == EINVAL, words
        assert words in _error(), (words, _error())
        rc, again = grow(c)
        assert rc == 0 and same_bits(kept, again), words
