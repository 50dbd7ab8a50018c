"""-m gpu: gss_set_components (csrc/set_modules.hip) and gss_random_sets (csrc/proximity.hip) through the C entry points, on the inputs of
tests/set_modules_cases.py and the random-set inputs of tests/proximity_cases.py.  What those inputs are for, and that a wrong rule
cannot hide behind the comparisons used here, is established on the CPU in tests/test_set_modules_mirror.py.

Everything is an integer and compared bit for bit (np.array_equal): lcc, n_comp, n_edges and the labels against the mirror, between guard
rows that must come back untouched, the labels' entries past every size still the sentinel.  Every call is made twice and must give the
same bits.  Every small case runs with the table's rows exactly as long as the set (64 and below: one wave per workgroup; above: four)
and again with rows 7 longer.

No test provokes a fault: the refusals are host-side argument checks that launch nothing, or units the kernel flags before it reads a
row of theirs (a size outside the row, a member that is no node, members out of order)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import proximity_cases as PK  # noqa: E402
import set_modules_cases as K  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, SENT, EINVAL = 3, -77, -22
MAX_SET = 4096


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _error():
    return _lib.load().gss_last_error().decode()


def guarded(rows, shape):
    return torch.full((rows + 2 * GUARD,) + tuple(shape), SENT, dtype=torch.int32, device="cuda")


def inside(buf, rows):
    h = buf.cpu().numpy()
    assert (h[:GUARD] == SENT).all() and (h[GUARD + rows:] == SENT).all(), "a guard row was written"
    return h[GUARD:GUARD + rows]


_graphs = {}


def graph(c):
    if c.name not in _graphs:
        _graphs[c.name] = (_dev(c.rowptr), _dev(c.col if len(c.col) else np.zeros(1, np.int32)))
    return _graphs[c.name]


def components(c, nodes, sizes, labels=True, n=None, n_units=None, max_size=None, null=None):
    """nodes [U, max_size], sizes [U] host int32 -> (rc, lcc, n_comp, n_edges [U], label [U, max_size] with SENT where unwritten)"""
    lib = _lib.load()
    rowptr, col = graph(c)
    U, ms = nodes.shape
    dn, ds = _dev(nodes), _dev(sizes)
    out = [guarded(U, ()) for _ in range(3)]
    lab = guarded(U, (ms,))
    ptrs = dict(rowptr=_lib.ptr(rowptr), col=_lib.ptr(col), nodes=_lib.ptr(dn), sizes=_lib.ptr(ds), lcc=_lib.ptr(out[0][GUARD:]),
                n_comp=_lib.ptr(out[1][GUARD:]), n_edges=_lib.ptr(out[2][GUARD:]), label=_lib.ptr(lab[GUARD:]) if labels else None)
    if null:
        ptrs[null] = None
    rc = lib.gss_set_components(c.n if n is None else n, ptrs["rowptr"], ptrs["col"], U if n_units is None else n_units,
                                ms if max_size is None else max_size, ptrs["nodes"], ptrs["sizes"], ptrs["lcc"], ptrs["n_comp"],
                                ptrs["n_edges"], ptrs["label"], _lib.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy(), nodes) and np.array_equal(ds.cpu().numpy(), sizes)            # inputs left alone
    return (rc,) + tuple(inside(o, U) for o in out) + (inside(lab, U),)


def want(name, max_size=None):
    """the mirror's four outputs as the device writes them: int32, the labels SENT past every size and widened to max_size"""
    lcc, n_comp, n_edges, lab = K.mirror(name)
    wide = np.full((lab.shape[0], max_size or lab.shape[1]), SENT, np.int32)
    wide[:, :lab.shape[1]] = np.where(lab < 0, SENT, lab)
    return lcc.astype(np.int32), n_comp.astype(np.int32), n_edges.astype(np.int32), wide


def check(got, expected, what):
    assert got[0] == 0, _error()
    for g, w, field in zip(got[1:], expected, ("lcc", "n_comp", "n_edges", "label")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, field, np.argwhere(g != w)[:5])


@pytest.mark.parametrize("name", K.SMALL_CASES)
def test_components_equal_the_mirror_bit_for_bit(name):
    c = K.case(name)
    for ms in sorted({c.max_size, min(c.max_size + 7, MAX_SET)}):
        nodes, sizes = K.table_arrays(c, ms)
        got = components(c, nodes, sizes)
        check(got, want(name, ms), (name, ms))
        again = components(c, nodes, sizes)
        assert all(np.array_equal(a, b) for a, b in zip(got[1:], again[1:])), (name, ms)
        bare = components(c, nodes, sizes, labels=False)                          # label = NULL: the same triples, no label written
        assert bare[0] == 0 and all(np.array_equal(a, b) for a, b in zip(got[1:4], bare[1:4])) and (bare[4] == SENT).all()
    if c.want is not None:
        assert [tuple(int(x[k]) for x in got[1:4]) for k in range(len(c.units))] == [tuple(w) for w in c.want]


def test_3000_units_in_one_launch_and_each_alone():
    c = K.case("many_3000")
    lib = _lib.load()
    nodes, sizes = K.table_arrays(c)
    got = components(c, nodes, sizes)
    check(got, want("many_3000"), "many_3000")
    again = components(c, nodes, sizes)
    assert all(np.array_equal(a, b) for a, b in zip(got[1:], again[1:]))
    # every unit in a call of its own, reading its row of the same table and writing its row of fresh outputs
    rowptr, col = graph(c)
    U, ms = nodes.shape
    dn, ds = _dev(nodes), _dev(sizes)
    out = [guarded(U, ()) for _ in range(3)]
    lab = guarded(U, (ms,))
    st = _lib.current_stream()
    for u in range(U):
        rc = lib.gss_set_components(c.n, _lib.ptr(rowptr), _lib.ptr(col), 1, ms, _lib.ptr(dn[u:]), _lib.ptr(ds[u:]), _lib.ptr(out[0][GUARD + u:]),
                                    _lib.ptr(out[1][GUARD + u:]), _lib.ptr(out[2][GUARD + u:]), _lib.ptr(lab[GUARD + u:]), st)
        assert rc == 0, (u, _error())
    torch.cuda.synchronize()
    alone = tuple(inside(o, U) for o in out) + (inside(lab, U),)
    assert all(np.array_equal(a, b) for a, b in zip(got[1:], alone))


def test_70000_units_in_one_launch():
    c = K.case("grid_70000")
    nodes, sizes = K.table_arrays(c)
    got = components(c, nodes, sizes)
    check(got, want("grid_70000"), "grid_70000")
    again = components(c, nodes, sizes)
    assert all(np.array_equal(a, b) for a, b in zip(got[1:], again[1:]))
    assert got[1][-1] == K.mirror("grid_70000")[0][-1] and len(got[1]) == 70000


def _valid_refused_valid(valid, *refused):
    kept = valid()
    for call, words in refused:
        assert call() == EINVAL, words
        assert words in _error(), (words, _error())
        again = valid()
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(again, kept)), words


def test_components_refusals_by_name_leave_nothing_behind():
    c = K.case("bounds")
    nodes, sizes = K.table_arrays(c)                      # max_size 5, units of 3, 3 and 2 members

    def valid():
        got = components(c, nodes, sizes)
        check(got, want("bounds"), "bounds")
        return got[1:]

    def with_unit(u, members=None, size=None, of=None):
        """the table (or the table `of` an earlier with_unit) with unit u replaced"""
        n2, s2 = (nodes.copy(), sizes.copy()) if of is None else (x.copy() for x in of.table)
        if members is not None:
            n2[u, :len(members)] = members
            s2[u] = len(members)
        if size is not None:
            s2[u] = size
        call = lambda: components(c, n2, s2)[0]  # noqa: E731
        call.table = (n2, s2)
        return call

    refusals = [(lambda k=k: components(c, nodes, sizes, null=k)[0], "set_components: null pointer")
                for k in ("rowptr", "col", "nodes", "sizes", "lcc", "n_comp", "n_edges")]
    refusals += [
        (lambda: components(c, nodes, sizes, n=0)[0], "set_components: n=0 n_units=3 must be >= 1"),
        (lambda: components(c, nodes, sizes, n_units=0)[0], "set_components: n=5000 n_units=0 must be >= 1"),
        (lambda: components(c, nodes, sizes, max_size=0)[0], "set_components: max_size=0 must be in [1, 4096]"),
        (lambda: components(c, nodes, sizes, max_size=4097)[0], "set_components: max_size=4097 must be in [1, 4096]"),
        (lambda: components(c, nodes, sizes, n_units=(1 << 40) // 5 + 1)[0], "set_components: the set table is too large"),
        (with_unit(1, size=6), "set_components: a unit's size is outside [0, max_size=5]"),
        (with_unit(2, size=-1), "set_components: a unit's size is outside [0, max_size=5]"),
        (with_unit(0, members=[0, 100, c.n]), f"set_components: a member is not a node index in [0, {c.n})"),
        (with_unit(1, members=[-1, 20, 30]), f"set_components: a member is not a node index in [0, {c.n})"),
        (with_unit(1, members=[10, 20, 20]), "set_components: a unit's members are not strictly ascending"),
        (with_unit(2, members=[30, 20]), "set_components: a unit's members are not strictly ascending"),
        # several bad units in one call: the refusal is the lowest bit's, whichever unit set it
        (with_unit(2, members=[0, 100, c.n], of=with_unit(0, members=[30, 20])), f"set_components: a member is not a node index in [0, {c.n})"),
        (with_unit(2, size=6, of=with_unit(1, members=[30, 20], of=with_unit(0, members=[0, 100, c.n]))),
         "set_components: a unit's size is outside [0, max_size=5]"),
    ]
    _valid_refused_valid(valid, *refusals)


# ---- gss_random_sets against gss_prox_random_sets -------------------------------------------------------------------------------------------

def random_sets(name, side, handle=None, n=None, max_size=None, sets=None, null=False):
    """gss_prox_random_sets behind `handle`, else gss_random_sets -> (rc, nodes [n_sets, R, max_size], sizes [n_sets, R])"""
    c = PK.random_case(name)
    lib = _lib.load()
    sets = c.sets if sets is None else sets
    max_size = max_size or c.max_size
    ptr = np.zeros(len(sets) + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    flat = np.concatenate(list(sets) + [np.zeros(1, np.int64)]).astype(np.int32)
    bin_ptr = np.zeros(len(c.bin_list) + 1, np.int32)
    bin_ptr[1:] = np.cumsum([len(b) for b in c.bin_list])
    d = [_dev(x) for x in (ptr, flat, c.node_bin.astype(np.int32), bin_ptr, np.concatenate(c.bin_list).astype(np.int32))]
    R = c.n_random + 1
    U = len(sets) * R
    nodes, sizes = guarded(U, (max_size,)), guarded(U, ())
    rest = (side, len(sets), _lib.ptr(d[0]), None if null else _lib.ptr(d[1]), max_size, _lib.ptr(d[2]), _lib.ptr(d[3]), _lib.ptr(d[4]),
            c.n_random, c.seed, _lib.ptr(nodes[GUARD:]), _lib.ptr(sizes[GUARD:]), _lib.current_stream())
    rc = lib.gss_prox_random_sets(handle, *rest) if handle is not None else lib.gss_random_sets(c.n if n is None else n, *rest)
    torch.cuda.synchronize()
    return rc, inside(nodes, U).reshape(len(sets), R, max_size), inside(sizes, U).reshape(len(sets), R)


@pytest.fixture(scope="module")
def prox_handle():
    g = PK.graph("web_132")
    rowptr, col = _dev(g.rowptr), _dev(g.col)
    h = C.c_void_p()
    assert _lib.load().gss_prox_create(C.byref(h), g.n, _lib.ptr(rowptr), _lib.ptr(col), 1 << 30, _lib.current_stream()) == 0, _error()
    yield h
    _lib.load().gss_prox_destroy(h)


@pytest.mark.parametrize("name", PK.RANDOM_CASES)
def test_random_sets_without_a_handle_equal_those_with_one(name, prox_handle):
    c = PK.random_case(name)
    assert name != "n_random_0" or c.n_random == 0
    for side in (0, 1):
        rc0, nodes0, sizes0 = random_sets(name, side, handle=prox_handle)
        assert rc0 == 0, _error()
        rc, nodes, sizes = random_sets(name, side)
        assert rc == 0, _error()
        assert np.array_equal(nodes, nodes0) and np.array_equal(sizes, sizes0), (name, side)
        want_nodes, want_sizes = PK.table_arrays(PK.random_table(name, side), c.max_size, pad=SENT)      # and both equal the mirror
        assert np.array_equal(nodes, want_nodes) and np.array_equal(sizes, want_sizes)
        rc, nodes2, sizes2 = random_sets(name, side)
        assert rc == 0 and np.array_equal(nodes2, nodes) and np.array_equal(sizes2, sizes)


def test_random_sets_refusals_by_name_leave_nothing_behind():
    c = PK.random_case("mixed")
    outside = [np.array([3, 132], np.int64)] + list(c.sets[1:])

    def valid():
        rc, nodes, sizes = random_sets("mixed", 0)
        assert rc == 0, _error()
        return [nodes, sizes]

    _valid_refused_valid(
        valid,
        (lambda: random_sets("mixed", 0, n=0)[0], "random_sets: n=0 must be >= 1"),
        (lambda: random_sets("mixed", 2)[0], "random_sets: side=2 must be 0 (from) or 1 (to)"),
        (lambda: random_sets("mixed", 0, null=True)[0], "random_sets: null pointer"),
        (lambda: random_sets("mixed", 0, sets=outside)[0], "random_sets: a set member is not a node index in [0, 132)"),
        (lambda: random_sets("mixed", 0, max_size=c.max_size - 1)[0], f"random_sets: a set has more than max_size={c.max_size - 1} members"))
    assert "prox_" not in _error()
