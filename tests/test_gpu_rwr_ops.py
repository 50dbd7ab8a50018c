"""-m gpu: gss_rwr_rank and gss_rwr_null_stats (csrc/rwr.hip) through the C entry points on the cases of tests/rwr_cases.py, against the
mirror (tests/rwr_mirror.py; tests/test_rwr_mirror.py holds the mirror to linear algebra and shows what every case is for).

node, iters, score and p_out are compared bit for bit on every unit of every case: both sides do the same IEEE additions,
multiplications and divisions in the order include/gssgcn.h states, and nothing else.  Every output lies between guard rows that must
come back untouched; every call is made twice and must give the same bits.

No test provokes a fault: the refusals are host-side argument checks that launch nothing, or units and rows the kernel flags before it
walks a row (a size outside the table's row, a seed that is no node, seeds out of order, a row longer than the bound given, an empty
row)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import rwr_cases as K  # noqa: E402
import rwr_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD, EINVAL, ENOTCONV = 2, -22, -34
SENT_I, SENT_F = -77, -7.75
OUT = ("node", "score", "iters", "p")
STATS = ("mean", "sd", "z", "ge", "node")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _error():
    return _lib.load().gss_last_error().decode()


def bits(x):
    return x.view(np.int64) if x.dtype == np.float64 else x


def same_bits(a, b, fields=OUT):
    return all(a[f].dtype == b[f].dtype and a[f].shape == b[f].shape and np.array_equal(bits(a[f]), bits(b[f])) for f in fields)


_graphs = {}


def on_device(rowptr, col):
    key = (id(rowptr), id(col))
    if key not in _graphs:
        _graphs[key] = (_dev(rowptr), _dev(col), rowptr, col)
    return _graphs[key][:2]


def rank(c, nodes=None, sizes=None, null=(), csr=None, **over):
    """-> (rc, {field: rows}) of one gss_rwr_rank on case c; `over` replaces scalar arguments, `null` names pointers passed as NULL,
    csr = (rowptr, col) another graph"""
    lib = _lib.load()
    if nodes is None:
        nodes, sizes = K.seed_table(c)
    U, ms = nodes.shape
    n_add = over.get("n_add", c.n_add)
    rows = min(max(n_add, 1), 2048)
    rowptr, col = on_device(*(csr or (c.rowptr, c.col)))
    dn, dz = _dev(nodes), _dev(sizes)
    bufs = {"node": torch.full((U + 2 * GUARD, rows), SENT_I, dtype=torch.int32, device="cuda"),
            "score": torch.full((U + 2 * GUARD, rows), SENT_F, dtype=torch.float64, device="cuda"),
            "iters": torch.full((U + 2 * GUARD,), SENT_I, dtype=torch.int32, device="cuda"),
            "p": torch.full((U + 2 * GUARD, c.n), SENT_F, dtype=torch.float64, device="cuda")}
    ptrs = dict(rowptr=_lib.ptr(rowptr), col=_lib.ptr(col), nodes=_lib.ptr(dn), sizes=_lib.ptr(dz))
    ptrs.update({f: _lib.ptr(bufs[f][GUARD:]) for f in OUT})
    for k in null:
        ptrs[k] = None
    rc = lib.gss_rwr_rank(over.get("n", c.n), ptrs["rowptr"], ptrs["col"], over.get("max_deg", K.max_degree(c)), over.get("n_units", U),
                          over.get("max_size", ms), ptrs["nodes"], ptrs["sizes"], over.get("restart", c.restart), over.get("tol", c.tol),
                          over.get("max_iter", c.max_iter), n_add, ptrs["node"], ptrs["score"], ptrs["iters"], ptrs["p"], _lib.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(dn.cpu().numpy(), nodes) and np.array_equal(dz.cpu().numpy(), sizes)            # inputs left alone
    out = {}
    for f in OUT:
        h = bufs[f].cpu().numpy()
        sent = SENT_I if h.dtype == np.int32 else SENT_F
        assert (h[:GUARD] == sent).all() and (h[GUARD + U:] == sent).all(), f"a guard row of {f} was written"
        if f in null:
            assert (h == sent).all(), f"{f} was passed as NULL"
        out[f] = h[GUARD:GUARD + U]
    return rc, out


def check(got, want, what, fields=OUT):
    for f in fields:
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        diff = bits(got[f]) != bits(want[f])
        if want[f].dtype == np.float64:                    # NaN is NaN whatever its payload
            diff &= ~(np.isnan(got[f]) & np.isnan(want[f]))
        assert not diff.any(), (what, f, np.argwhere(diff)[:5], got[f][diff][:5], want[f][diff][:5])


@pytest.mark.parametrize("name", K.CASES)
def test_rank_equals_the_mirror_bit_for_bit(name):
    c, want = K.case(name), K.mirror(name)
    rc, got = rank(c)
    assert rc == 0, _error()
    check(got, want, name)
    rc, again = rank(c)
    assert rc == 0 and same_bits(got, again), name
    if len(c.units) <= 8:
        # rows 7 longer (where the table's limit leaves room), junk past every size
        nodes, sizes = K.seed_table(c, min(max(1, max(len(u) for u in c.units)) + 7, M.MAX_SEEDS), pad=0x7FFFFFFF)
        rc, wide = rank(c, nodes, sizes, null=("p",))
        assert rc == 0 and same_bits(got, wide, ("node", "score", "iters")), name
        rc, bare = rank(c, null=("node", "score"))
        assert rc == 0 and same_bits(got, bare, ("iters", "p")), name


def test_not_converged_is_said_with_the_last_iterate_in_place():
    c, want = K.case("not_converged"), K.mirror("not_converged")
    rc, got = rank(c)
    assert rc == ENOTCONV, (rc, _error())
    assert "rwr_rank: 3 of 3 units did not reach err < tol=1e-12 within max_iter=3" in _error(), _error()
    check(got, want, "not_converged")
    rc, got = rank(c, max_iter=1000)
    assert rc == 0, _error()
    assert (got["iters"] > 3).all() and (got["iters"] <= M.iteration_bound(c.restart, c.tol)).all()
    nodes, sizes = K.seed_table(c)                         # one of the three converges at once: the message counts the others
    rc, _ = rank(c, np.concatenate([nodes, nodes[:1]]), np.concatenate([sizes, [0]]).astype(np.int32))
    assert rc == ENOTCONV and "rwr_rank: 3 of 4 units" in _error(), _error()


def test_a_unit_is_the_same_alone_and_at_any_position():
    c, want = K.case("same"), K.mirror("same")
    rc, got = rank(c)
    assert rc == 0, _error()
    nodes, sizes = K.seed_table(c)
    rc, alone = rank(c, nodes[:1, :5].copy(), sizes[:1].copy())
    assert rc == 0, _error()
    for u in (0, 2, 5):
        assert same_bits({f: got[f][u:u + 1] for f in OUT}, alone), u
        check({f: got[f][u:u + 1] for f in OUT}, {f: want[f][:1] for f in OUT}, u)


def test_one_node_too_many_is_refused():
    c = K.case("limit")
    rc, _ = rank(c, n=M.MAX_NODES + 1)                       # a host-side check: nothing is launched
    assert rc == EINVAL and f"rwr_rank: n={M.MAX_NODES + 1} must be in [2, {M.MAX_NODES}]" in _error(), _error()
    rc, got = rank(c)
    assert rc == 0, _error()
    check(got, K.mirror("limit"), "limit")


def test_refusals_by_name_leave_nothing_behind():
    c = K.case("one")
    nodes, sizes = K.seed_table(c)                         # three units of six seeds
    rc, kept = rank(c)
    assert rc == 0, _error()

    def with_unit(u, members=None, size=None, of=None):
        n2, z2 = (nodes.copy(), sizes.copy()) if of is None else (x.copy() for x in of.table)
        if members is not None:
            n2[u, :len(members)] = members
            z2[u] = len(members)
        if size is not None:
            z2[u] = size
        call = lambda: rank(c, n2, z2)[0]  # noqa: E731
        call.table = (n2, z2)
        return call

    md = K.max_degree(c)
    lonely = (np.append(c.rowptr, c.rowptr[-1]).astype(np.int32), c.col)       # node 300 has no neighbour
    refusals = [(lambda k=k: rank(c, null=(k,))[0], "rwr_rank: null pointer") for k in ("rowptr", "col", "nodes", "sizes", "iters")]
    refusals += [
        (lambda: rank(c, null=("node",))[0], "rwr_rank: node_out and score_out are given together or not at all"),
        (lambda: rank(c, null=("score",))[0], "rwr_rank: node_out and score_out are given together or not at all"),
        (lambda: rank(c, null=("node", "score", "p"))[0], "rwr_rank: neither a ranking nor p_out is asked for"),
        (lambda: rank(c, n=1)[0], f"rwr_rank: n=1 must be in [2, {M.MAX_NODES}]"),
        (lambda: rank(c, n_units=0)[0], "rwr_rank: n_units=0 must be >= 1"),
        (lambda: rank(c, max_size=0)[0], "rwr_rank: max_size=0 must be in [1, 4096]"),
        (lambda: rank(c, max_size=4097)[0], "rwr_rank: max_size=4097 must be in [1, 4096]"),
        (lambda: rank(c, max_deg=0)[0], "rwr_rank: max_deg=0 must be >= 1"),
        (lambda: rank(c, restart=0.0)[0], "rwr_rank: restart=0 must be in (0, 1)"),
        (lambda: rank(c, restart=1.0)[0], "rwr_rank: restart=1 must be in (0, 1)"),
        (lambda: rank(c, restart=float("nan"))[0], "must be in (0, 1)"),
        (lambda: rank(c, tol=-1e-6)[0], "rwr_rank: tol=-1e-06 must be >= 0"),
        (lambda: rank(c, tol=float("nan"))[0], "must be >= 0"),
        (lambda: rank(c, max_iter=0)[0], "rwr_rank: max_iter=0 must be >= 1"),
        (lambda: rank(c, n_add=0)[0], "rwr_rank: n_add=0 must be in [1, 1024]"),
        (lambda: rank(c, n_add=1025)[0], "rwr_rank: n_add=1025 must be in [1, 1024]"),
        (lambda: rank(c, max_deg=md - 1)[0], f"rwr_rank: a row of the CSR is longer than max_deg={md - 1}"),
        (lambda: rank(c, csr=lonely, n=c.n + 1)[0], "rwr_rank: a row of the CSR is empty"),
        (with_unit(1, size=7), "rwr_rank: a unit's size is outside [0, max_size=6]"),
        (with_unit(2, size=-1), "rwr_rank: a unit's size is outside [0, max_size=6]"),
        (with_unit(0, members=[0, 10, c.n]), f"rwr_rank: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[-1, 20, 30]), f"rwr_rank: a seed is not a node index in [0, {c.n})"),
        (with_unit(1, members=[10, 20, 20]), "rwr_rank: a unit's seeds are not strictly ascending"),
        (with_unit(2, members=[30, 20]), "rwr_rank: a unit's seeds are not strictly ascending"),
        (with_unit(2, members=[0, 10, c.n], of=with_unit(0, members=[30, 20])), f"rwr_rank: a seed is not a node index in [0, {c.n})"),
        (with_unit(2, size=7, of=with_unit(1, members=[30, 20], of=with_unit(0, members=[0, 10, c.n]))),
         "rwr_rank: a unit's size is outside [0, max_size=6]"),
    ]
    for call, words in refusals:
        assert call() == EINVAL, words
        assert words in _error(), (words, _error())
        rc, again = rank(c)
        assert rc == 0 and same_bits(kept, again), words


# ---- gss_rwr_null_stats --------------------------------------------------------------------------------------------------------------------

def null_stats(p, seeds, n_add, rank_by, first=0, count=None, null=None, **over):
    """-> (rc, {field: rows}) of one gss_rwr_null_stats over the sets [first, first + count) of the case's table"""
    lib = _lib.load()
    S, R, n = p.shape
    count = S - first if count is None else count
    ms = max(1, max(len(s) for s in seeds)) + 3
    nodes = np.full((S, R, ms), 0x7FFFFFFF, np.int32)      # only sample 0's rows are read
    sizes = np.full((S, R), -5, np.int32)
    for s, x in enumerate(seeds):
        nodes[s, 0, :len(x)] = x
        sizes[s, 0] = len(x)
    if "nodes" in over:
        nodes, sizes = over["nodes"], over["sizes"]
    dp, dn, dz = _dev(p), _dev(nodes), _dev(sizes)
    rows = max(n_add, 1) if n_add <= 1024 else 1
    bufs = {f: torch.full((count + 2 * GUARD, n), SENT_F, dtype=torch.float64, device="cuda") for f in ("mean", "sd", "z")}
    bufs["ge"] = torch.full((count + 2 * GUARD, n), SENT_I, dtype=torch.int32, device="cuda")
    bufs["node"] = torch.full((count + 2 * GUARD, rows), SENT_I, dtype=torch.int32, device="cuda")
    ptrs = {f: _lib.ptr(bufs[f][GUARD:]) for f in STATS}
    ptrs.update(p=_lib.ptr(dp[first:]), nodes=_lib.ptr(dn[first:]), sizes=_lib.ptr(dz[first:]))
    if null:
        ptrs[null] = None
    rc = lib.gss_rwr_null_stats(over.get("n", n), over.get("n_sets", count), over.get("R", R), ptrs["p"], over.get("max_size", ms), ptrs["nodes"],
                                ptrs["sizes"], n_add, {"p": 0, "z": 1}.get(rank_by, rank_by), ptrs["mean"], ptrs["sd"], ptrs["z"], ptrs["ge"],
                                ptrs["node"], _lib.current_stream())
    torch.cuda.synchronize()
    assert np.array_equal(bits(dp.cpu().numpy()), bits(p))
    out = {}
    for f in STATS:
        h = bufs[f].cpu().numpy()
        sent = SENT_I if h.dtype == np.int32 else SENT_F
        assert (h[:GUARD] == sent).all() and (h[GUARD + count:] == sent).all(), f"a guard row of {f} was written"
        out[f] = h[GUARD:GUARD + count]
    return rc, out


def null_mirror(p, seeds, n_add, rank_by):
    per = [M.null_stats(p[s], seeds[s], n_add, rank_by) for s in range(len(seeds))]
    return {f: np.stack([t[f] for t in per]) for f in STATS}


@pytest.mark.parametrize("rank_by", ["p", "z"])
@pytest.mark.parametrize("name", K.NULL_CASES)
def test_null_stats_equal_the_mirror_bit_for_bit(name, rank_by):
    p, seeds, n_add = K.null_case(name)
    want = null_mirror(p, seeds, n_add, rank_by)
    rc, got = null_stats(p, seeds, n_add, rank_by)
    assert rc == 0, _error()
    check(got, want, (name, rank_by), STATS)
    rc, again = null_stats(p, seeds, n_add, rank_by)
    assert rc == 0 and same_bits(got, again, STATS)
    parts = [null_stats(p, seeds, n_add, rank_by, first, count) for first, count in ((0, 1), (1, 2))]       # 3 sets: 3, then 1 and 2 at a time
    assert all(rc == 0 for rc, _ in parts)
    assert same_bits(got, {f: np.concatenate([t[f] for _, t in parts]) for f in STATS}, STATS)
    singles = [null_stats(p, seeds, n_add, rank_by, first, 1) for first in range(3)]
    assert all(rc == 0 for rc, _ in singles)
    assert same_bits(got, {f: np.concatenate([t[f] for _, t in singles]) for f in STATS}, STATS)


def test_null_stats_refusals_by_name_leave_nothing_behind():
    p, seeds, n_add = K.null_case("r65")
    rc, kept = null_stats(p, seeds, n_add, "z")
    assert rc == 0, _error()
    S, R, n = p.shape

    def table(u, members, size=None):
        nodes = np.full((S, R, 4), -1, np.int32)
        sizes = np.zeros((S, R), np.int32)
        for s, x in enumerate(seeds):
            nodes[s, 0, :len(x)] = x
            sizes[s, 0] = len(x)
        nodes[u, 0, :len(members)] = members
        sizes[u, 0] = len(members) if size is None else size
        return lambda: null_stats(p, seeds, n_add, "z", nodes=nodes, sizes=sizes, max_size=4)[0]

    refusals = [(lambda k=k: null_stats(p, seeds, n_add, "z", null=k)[0], "rwr_null_stats: null pointer") for k in ("p", "nodes", "sizes") + STATS]
    refusals += [
        (lambda: null_stats(p, seeds, n_add, "z", n=1)[0], f"rwr_null_stats: n=1 must be in [2, {M.MAX_NODES}]"),
        (lambda: null_stats(p, seeds, n_add, "z", n=M.MAX_NODES + 1)[0], f"rwr_null_stats: n={M.MAX_NODES + 1} must be in [2, {M.MAX_NODES}]"),
        (lambda: null_stats(p, seeds, n_add, "z", n_sets=0)[0], "rwr_null_stats: n_sets=0 must be in [1, 65535]"),
        (lambda: null_stats(p, seeds, n_add, "z", R=2)[0], "rwr_null_stats: R=2 must be in [3, 1048576]"),
        (lambda: null_stats(p, seeds, n_add, "z", max_size=0)[0], "rwr_null_stats: max_size=0 must be in [1, 4096]"),
        (lambda: null_stats(p, seeds, 0, "z")[0], "rwr_null_stats: n_add=0 must be in [1, 1024]"),
        (lambda: null_stats(p, seeds, 1025, "z")[0], "rwr_null_stats: n_add=1025 must be in [1, 1024]"),
        (lambda: null_stats(p, seeds, n_add, 2)[0], "rwr_null_stats: rank_by=2 must be 0 (p) or 1 (z)"),
        (table(1, [5], size=5), "rwr_null_stats: a unit's size is outside [0, max_size=4]"),
        (table(0, [0, 1, n]), f"rwr_null_stats: a seed is not a node index in [0, {n})"),
        (table(2, [151, 150]), "rwr_null_stats: a unit's seeds are not strictly ascending"),
    ]
    for call, words in refusals:
        assert call() == EINVAL, words
        assert words in _error(), (words, _error())
        rc, again = null_stats(p, seeds, n_add, "z")
        assert rc == 0 and same_bits(kept, again, STATS), words
