"""-m gpu: gss_diamond_grow (csrc/diamond.hip) through the C entry point on the cases of tests/diamond_cases.py, against the mirror
(tests/diamond_mirror.py; tests/test_diamond_mirror.py holds the mirror to scipy and shows what every case is for).

node, k', kb' are compared exactly, lt0 and S bit for bit (both sides do the same IEEE additions, one division and one multiplication per
term, in the same order), logp to within 4 ulp of the mirror's lt0 + log(S): the device's log is the only operation that is not
correctly rounded on both sides.  Every case keeps the runner-up's logp more than MIN_GAP relative away from the winner's at every
step (asserted here again, on the CPU): below that the winner is reproducible but implementation-defined, and the mirror could not be
the judge.  All six outputs lie between guard rows that must come back untouched; every call is made twice and must give the same bits.

No test provokes a fault: the refusals are host-side argument checks that launch nothing, or units the kernel flags before it walks a
row of theirs (a size outside the row, a seed that is no node, seeds out of order, a row longer than the bound given)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import diamond_cases as K  # noqa: E402
import diamond_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, EINVAL = 2, -22
SENT_I, SENT_F = -77, -7.75
INTS, REALS = ("node", "k", "kb"), ("lt0", "S", "logp")
OUT = ("node", "k", "kb", "lt0", "S", "logp")


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


_tables = {}


def lg_table(n_lg):
    if n_lg not in _tables:
        _tables[n_lg] = _dev(M.lgamma_table(n_lg))
    return _tables[n_lg]


def grow(c, seeds=None, sizes=None, null=None, **over):
    """-> (rc, {field: [U, n_add]}) of one call on case c; `over` replaces scalar arguments, `null` names a pointer passed as NULL"""
    lib = _lib.load()
    if seeds is None:
        seeds, sizes = K.seed_table(c)
    U, ms = seeds.shape
    n_add, alpha = over.get("n_add", c.n_add), over.get("alpha", c.alpha)
    rows = max(n_add, 1)
    rowptr, col = graph(c)
    lg = lg_table(c.n + (max(alpha, 1) - 1) * ms + 2)
    ds, dz = _dev(seeds), _dev(sizes)
    bufs = {f: torch.full((U + 2 * GUARD, rows), SENT_I, dtype=torch.int32, device="cuda") for f in INTS}
    bufs.update({f: torch.full((U + 2 * GUARD, rows), SENT_F, dtype=torch.float64, device="cuda") for f in REALS})
    ptrs = dict(rowptr=_lib.ptr(rowptr), col=_lib.ptr(col), lg=_lib.ptr(lg), seeds=_lib.ptr(ds), sizes=_lib.ptr(dz))
    ptrs.update({f: _lib.ptr(bufs[f][GUARD:]) for f in OUT})
    if null:
        ptrs[null] = None
    rc = lib.gss_diamond_grow(over.get("n", c.n), ptrs["rowptr"], ptrs["col"], over.get("max_deg", K.max_degree(c)), ptrs["lg"],
                              over.get("n_lg", len(lg)), over.get("n_units", U), over.get("max_size", ms), ptrs["seeds"], ptrs["sizes"], n_add,
                              alpha, *(ptrs[f] for f in OUT), _lib.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(ds.cpu().numpy(), seeds) and np.array_equal(dz.cpu().numpy(), sizes)            # inputs left alone
    out = {}
    for f in OUT:
        h = bufs[f].cpu().numpy()
        sent = SENT_I if f in INTS else SENT_F
        assert (h[:GUARD] == sent).all() and (h[GUARD + U:] == sent).all(), f"a guard row of {f} was written"
        out[f] = h[GUARD:GUARD + U]
    return rc, out


def same_bits(a, b):
    return all(a[f].dtype == b[f].dtype and np.array_equal(a[f].view(np.int64 if f in REALS else np.int32),
                                                           b[f].view(np.int64 if f in REALS else np.int32)) for f in OUT)


def check(got, want, what):
    """the comparison of the module's docstring; prints the logp figure before it asserts"""
    for f in INTS:
        assert got[f].dtype == np.int32 and np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:5])
    for f in ("lt0", "S"):
        assert np.array_equal(got[f].view(np.int64), want[f].view(np.int64)), (what, f, np.argwhere(got[f] != want[f])[:5])
    ulps = np.abs(got["logp"] - want["logp"]) / np.spacing(np.abs(want["logp"]))
    print(f"{what}: logp within {ulps.max():.3g} ulp of the mirror's lt0 + log(S), {int((ulps > 0).sum())} of {ulps.size} differ")
    assert ulps.max() <= 4, (what, np.argwhere(ulps > 4)[:5], ulps.max())


@pytest.mark.parametrize("name", K.CASES)
def test_growth_equals_the_mirror(name):
    c = K.case(name)
    want = K.mirror(name)
    assert np.where(want["node"] >= 0, want["gap"], np.inf).min() > K.MIN_GAP
    rc, got = grow(c)
    assert rc == 0, _error()
    check(got, want, name)
    rc, again = grow(c)
    assert rc == 0 and same_bits(got, again), name
    if len(c.units) <= 8:                                                      # rows 7 longer, junk past every size
        seeds, sizes = K.seed_table(c, max(1, max(len(u) for u in c.units)) + 7, pad=0x7FFFFFFF)
        rc, wide = grow(c, seeds, sizes)
        assert rc == 0 and same_bits(got, wide), name


def test_the_fill_after_the_last_candidate_is_exact():
    rc, got = grow(K.case("odd"))
    assert rc == 0, _error()
    assert sorted(got["node"][0, :4].tolist()) == [0, 2, 4, 5]
    for u, first in ((0, 4), (1, 0), (4, 0), (5, 0)):
        assert (got["node"][u, first:] == -1).all() and (got["k"][u, first:] == 0).all() and (got["kb"][u, first:] == 0).all()
        for f in REALS:
            assert (got[f][u, first:].view(np.int64) == 0).all(), (u, f)      # +0.0, bit for bit


def test_one_call_and_three_calls_give_the_same_bits():
    c = K.case("n300_a1")
    lib = _lib.load()
    seeds, sizes = K.seed_table(c)
    rc, whole = grow(c, seeds, sizes)
    assert rc == 0, _error()
    U, ms = seeds.shape
    rowptr, col = graph(c)
    lg = lg_table(c.n + 2)
    ds, dz = _dev(seeds), _dev(sizes)
    bufs = {f: torch.full((U, c.n_add), SENT_I, dtype=torch.int32, device="cuda") for f in INTS}
    bufs.update({f: torch.full((U, c.n_add), SENT_F, dtype=torch.float64, device="cuda") for f in REALS})
    for lo, hi in ((0, 2), (2, 3), (3, 6)):
        rc = lib.gss_diamond_grow(c.n, _lib.ptr(rowptr), _lib.ptr(col), K.max_degree(c), _lib.ptr(lg), len(lg), hi - lo, ms, _lib.ptr(ds[lo:]),
                                  _lib.ptr(dz[lo:]), c.n_add, c.alpha, *(_lib.ptr(bufs[f][lo:]) for f in OUT), _lib.current_stream())
        assert rc == 0, _error()
    torch.cuda.synchronize()
    assert same_bits(whole, {f: bufs[f].cpu().numpy() for f in OUT})


def test_refusals_by_name_leave_nothing_behind():
    c = K.case("n40_a1")
    seeds, sizes = K.seed_table(c)                         # three units of five seeds
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
    refusals = [(lambda k=k: grow(c, null=k)[0], "diamond_grow: null pointer") for k in ("rowptr", "col", "lg", "seeds", "sizes") + OUT]
    refusals += [
        (lambda: grow(c, alpha=0)[0], "diamond_grow: alpha=0 must be >= 1"),
        (lambda: grow(c, n_add=0)[0], "diamond_grow: n_add=0 must be >= 1"),
        (lambda: grow(c, n=0)[0], "diamond_grow: n=0 n_units=3 must be >= 1"),
        (lambda: grow(c, n_units=0)[0], "diamond_grow: n=40 n_units=0 must be >= 1"),
        (lambda: grow(c, n=K.MAX_NODES + 1)[0], f"diamond_grow: n={K.MAX_NODES + 1} is over the limit of {K.MAX_NODES} nodes"),
        (lambda: grow(c, max_size=0)[0], "diamond_grow: max_size=0 must be in [1, 4096]"),
        (lambda: grow(c, max_size=4097)[0], "diamond_grow: max_size=4097 must be in [1, 4096]"),
        (lambda: grow(c, max_deg=65536)[0], "diamond_grow: alpha=1 x max_deg=65536 is over 65535"),
        (lambda: grow(c, alpha=3, max_deg=21846)[0], "diamond_grow: alpha=3 x max_deg=21846 is over 65535"),
        (lambda: grow(c, max_deg=5000, max_size=4090)[0], "diamond_grow: a node can have 4119 weighted links into the module"),
        (lambda: grow(c, n_lg=41)[0], "diamond_grow: n_lg=41, the lgamma table needs 42 entries"),
        (lambda: grow(c, max_deg=md - 1)[0], f"diamond_grow: a row of the CSR is longer than max_deg={md - 1}"),
        (with_unit(1, size=6), "diamond_grow: a unit's size is outside [0, max_size=5]"),
        (with_unit(2, size=-1), "diamond_grow: a unit's size is outside [0, max_size=5]"),
        (with_unit(0, members=[0, 10, c.n]), f"diamond_grow: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[-1, 20, 30]), f"diamond_grow: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[10, 20, 20]), "diamond_grow: a unit's seeds are not strictly ascending"),
        (with_unit(2, members=[30, 20]), "diamond_grow: a unit's seeds are not strictly ascending"),
        # several bad units in one call: the refusal is the lowest bit's, whichever unit set it
        (with_unit(2, members=[0, 10, c.n], of=with_unit(0, members=[30, 20])), f"diamond_grow: a seed is not a node index in [0, {c.n})"),
        (with_unit(2, size=6, of=with_unit(1, members=[30, 20], of=with_unit(0, members=[0, 10, c.n]))),
         "diamond_grow: a unit's size is outside [0, max_size=5]"),
    ]
    for call, words in refusals:
        assert call() == EINVAL, words
        assert words in _error(), (words, _error())
        rc, again = grow(c)
        assert rc == 0 and same_bits(kept, again), words
