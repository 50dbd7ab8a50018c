"""-m gpu: the shortest-path tree, count and between ops (csrc/paths.hip, csrc/trace.hip) op by op at the C ABI -- gss_paths_create,
gss_paths_run, gss_paths_count, gss_paths_between, gss_paths_between_fill through ctypes -- on the inputs of tests/paths_ops_cases.py,
against the closed forms of those cases and the numpy mirrors (tests/paths_mirror.py, tests/trace_mirror.py).  That the cases have the
properties the tests rely on is established on the CPU in tests/test_paths_ops_cases.py.

Every comparison is bit for bit: bytes, int32, integer-valued fp64, one multiply and one divide.  No tolerance anywhere.
Every output lies between 64 sentinel elements on either side (0xA5 bytes, -7, a NaN of a payload nothing computes); the sentinels are
checked after every call, refused ones included.  The between ops are handed the MIRROR's dist / sigma, so a failure names one kernel.

That the tests bite: value-only mutations of the kernels, one at a time (MI355X; "older" = test_gpu_predict.py + test_gpu_trace.py):
    mutation                                                       fails here                                             older tests
    1 paths_level_kernel: a bit is claimed again in a later chunk  run_tie_rule [L65, L128, L129, L200] (and what rests on it)  2 fail
      (`& ~rclaimed` dropped; with `rclaimed |=` dropped as well   all six whole-wave tie cases, the counts on them           7 fail
      the owner's `claimed` is lost too)
    2 paths_level_kernel: `excl` not zeroed at lane 0              run_tie_rule [L33 .. L200] (and what rests on it)           6 fail
    3 trace_level_kernel: the owner's own `rover`, not the ballot  count_overflow_seen_by_one_lane_reaches_the_owner           pass
    4 add_count: the `s == kMaxCount && ...` clause dropped        count_boundary [one_lane, whole_wave], count_overflow_...   pass
    5 trace_fill_kernel: `at < offset[p + 1]`, not `at < end`      fill_writes_nothing_at_or_beyond_capacity                   pass
    6 paths_level_kernel: flag 4 never raised                      borrowed_csr_that_changes_is_refused_at_run_time [both]     pass
Mutations 1 and 2 are also seen by the older tests (the random ~210-entry hub and the stand-in graph); 3 to 6 only here.  Mutation 3
passes every boundary_count_graph case -- after the butterfly every lane holds the total, so every lane sees an overflow of the total --
which is what lane_local_overcount_graph is for.

No test provokes a fault.  The run-time refusal of a column outside [0, n) is a refusal like the create-time one: paths_level_kernel
range-checks every column before it uses it as an index, in both row paths.  gss_paths_count does not re-check the columns of a
borrowed CSR, so it is never called while an entry is overwritten, and the entry is put back (try / finally) before anything else runs."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import paths_mirror as M  # noqa: E402
import paths_ops_cases as K  # noqa: E402
import trace_mirror as T  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.paths import csr_arrays  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = 64
EINVAL = -22
MAX_BYTES = 1 << 30
U8, I32, F64 = np.uint8, np.int32, np.float64
# no result equals these: hop counts here stay below 20, node indices are >= -1, and no count, weight sum or share is a NaN
SENT = {U8: 0xA5, I32: -7, F64: 0x7FF8DEADBEEF0001}
_TORCH = {U8: torch.uint8, I32: torch.int32, F64: torch.int64}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def err():
    return _lib.load().gss_last_error().decode()


def stream():
    return _lib.current_stream()


class Buf:
    """`count` elements of a device output between PAD sentinel elements on either side, pre-filled with the sentinel"""

    def __init__(self, count, kind):
        self.count, self.kind = int(count), kind
        self.full = torch.full((self.count + 2 * PAD,), SENT[kind], dtype=_TORCH[kind], device="cuda")

    @property
    def ptr(self):
        return self.full.data_ptr() + PAD * self.full.element_size()

    def zero(self):
        self.full[PAD:PAD + self.count] = 0
        return self

    def raw(self, what="output"):
        """the elements on the host as they are (sentinels where nothing was written), after checking the pads"""
        full = self.full.cpu().numpy()
        s = full.dtype.type(SENT[self.kind])
        assert (full[:PAD] == s).all(), f"{what}: written in front of the buffer"
        assert (full[PAD + self.count:] == s).all(), f"{what}: written behind the buffer"
        return full[PAD:PAD + self.count].copy()

    def host(self, what="output"):
        raw = self.raw(what)
        return raw.view(F64) if self.kind is F64 else raw

    def unwritten(self, what="output"):
        """mask of the elements that still hold the sentinel"""
        raw = self.raw(what)
        return raw == raw.dtype.type(SENT[self.kind])


class Run:
    pass


class Handle:
    """a gss_paths handle on (rowptr, col): uploaded (on_device = 0) or borrowing device tensors (on_device = 1)"""

    def __init__(self, rowptr, col, on_device=False):
        self.lib = _lib.load()
        self.rowptr = np.ascontiguousarray(rowptr, I32)
        self.col = np.ascontiguousarray(col, I32)
        self.n = len(self.rowptr) - 1
        self.h = C.c_void_p()
        if on_device:
            self.d_rowptr, self.d_col = dev(self.rowptr), dev(self.col)
            rp, cl = self.d_rowptr.data_ptr(), self.d_col.data_ptr()
        else:
            rp, cl = self.rowptr.ctypes.data, self.col.ctypes.data
        self.rc = self.lib.gss_paths_create(C.byref(self.h), self.n, len(self.col), rp, cl, int(on_device), MAX_BYTES, stream())

    @classmethod
    def of(cls, adj, on_device=False):
        h = cls(*csr_arrays(adj), on_device=on_device)
        assert h.rc == 0, err()
        return h

    def close(self):
        if self.h.value:
            self.lib.gss_paths_destroy(self.h)
        self.h = C.c_void_p()

    def run(self, targets, expect=0):
        """gss_paths_run -> Run(rc, dist uint8 [q, n], next int32 [q, n], levels, d_dist); the pads are checked whatever rc is"""
        t = np.ascontiguousarray(targets, I32)
        q, n = len(t), self.n
        r = Run()
        r.targets, r.d_dist, r.d_next = t, Buf(q * n, U8), Buf(q * n, I32)
        lv = C.c_int32(-5)
        r.rc = self.lib.gss_paths_run(self.h, q, t.ctypes.data, r.d_dist.ptr, r.d_next.ptr, C.byref(lv), stream())
        r.dist = r.d_dist.host("dist").reshape(q, n)
        r.next = r.d_next.host("next").reshape(q, n)
        r.levels = lv.value
        assert r.rc == expect, err()
        return r

    def count(self, r, w=None, expect=0):
        """gss_paths_count on the pass r -> (sigma, best, best_next) [q, n]; the pads are checked whatever the return code is"""
        q, n = len(r.targets), self.n
        sigma = Buf(q * n, F64)
        best = Buf(q * n, F64) if w is not None else None
        bnext = Buf(q * n, I32) if w is not None else None
        wd = dev(np.asarray(w, F64)) if w is not None else None
        rc = self.lib.gss_paths_count(self.h, q, r.targets.ctypes.data, r.d_dist.ptr, r.levels, _lib.ptr(wd), sigma.ptr,
                                      best.ptr if best else None, bnext.ptr if bnext else None, stream())
        out = [b.host(k).reshape(q, n) if b else None for b, k in ((sigma, "sigma"), (best, "best"), (bnext, "best_next"))]
        assert rc == expect, err()
        return out


@pytest.fixture
def handles():
    made = []

    def make(*a, **kw):
        made.append(Handle.of(*a, **kw) if not isinstance(a[0], np.ndarray) else Handle(*a, **kw))
        return made[-1]
    yield make
    for h in made:
        h.close()


# ---- gss_paths_run ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tie_case(i):
    g = K.tie_rule_graph(*K.TIE_CASES[i])
    d, nx_ = M.mirror_trees(g["adj"], g["targets"])
    assert np.array_equal(d, g["dist"]) and np.array_equal(nx_, g["next"])
    for a in (g["dist"], g["next"]):
        a.setflags(write=False)
    return g


TIE_IDS = [f"L{c[0]}" for c in K.TIE_CASES]


@pytest.mark.parametrize("i", range(len(K.TIE_CASES)), ids=TIE_IDS)
def test_run_tie_rule_at_the_row_length_boundaries(i, handles):
    """paths_level_kernel, both row paths: next of the hubs is the FIRST carrier u_p(q) for first carriers at positions 0, 31, 32, 63,
    64, 65 and L - 1 -- lane 0 and lane 63 of a 64-entry chunk (the `excl = 0` of lane 0, the prefix-OR up to lane 63), bit 63, a bit
    carried only from the second / third chunk on, a bit carried again in a later chunk (`rclaimed`), two unreachable targets (the row
    is read to its end), one target a level earlier; owners at lane 0, at lane 63, two in one wave, in the last partial wave (TIE_CASES).
    Rows of 32 entries take the one-lane path, 33 the whole-wave path.  n is no multiple of 4: a byte overrun of dist hits the pad.
    A target's rows do not depend on the pass (Q = 64, 1, 3, 63, a repeat), nor on what the handle ran before; *levels is the largest
    finite distance."""
    g = tie_case(i)
    n, t = g["n"], g["targets"]
    h = handles(g["adj"])
    r = h.run(t)
    assert same(r.dist, g["dist"]), np.argwhere(r.dist != g["dist"])[:8]
    assert same(r.next, g["next"]), [(q, v, r.next[q, v], g["next"][q, v]) for q, v in np.argwhere(r.next != g["next"])[:8]]
    assert r.levels == int(g["dist"][g["dist"] != 255].max()) == 2
    for q in range(64):                                                   # each alone
        one = h.run(t[q:q + 1])
        assert same(one.dist[0], g["dist"][q]) and same(one.next[0], g["next"][q]), q
        assert one.levels == int(g["dist"][q][g["dist"][q] != 255].max())
    for lo in range(0, 64, 3):
        three = h.run(t[lo:lo + 3])
        assert same(three.dist, g["dist"][lo:lo + 3]) and same(three.next, g["next"][lo:lo + 3]), lo
    for lo in (0, 1):
        most = h.run(t[lo:lo + 63])
        assert same(most.dist, g["dist"][lo:lo + 63]) and same(most.next, g["next"][lo:lo + 63]), lo
    twice = h.run(t[[5, 63, 5, 0]])
    assert same(twice.dist[0], twice.dist[2]) and same(twice.next[0], twice.next[2])
    assert same(twice.next, g["next"][[5, 63, 5, 0]]) and same(twice.dist, g["dist"][[5, 63, 5, 0]])
    # other targets on the used handle and on a fresh one: hubs and successors as targets (nothing reaches a hub)
    other = np.array([g["hubs"][0], g["succ"][0], 3, g["succ"][-1], n - 1], I32)
    again = h.run(other)
    fresh = handles(g["adj"]).run(other)
    md, mn = M.mirror_trees(g["adj"], other)
    assert same(again.dist, fresh.dist) and same(again.next, fresh.next) and again.levels == fresh.levels
    assert same(again.dist, md) and same(again.next, mn) and again.levels == int(md[md != 255].max())


@pytest.mark.parametrize("i", range(len(K.TIE_CASES)), ids=TIE_IDS)
def test_borrowed_device_csr_gives_the_bits_of_an_uploaded_one(i, handles):
    """gss_paths_create with on_device = 1 (the borrowed-pointer branch): the same dist / next / levels, and the same counts"""
    g = tie_case(i)
    up, on = handles(g["adj"]), handles(g["adj"], on_device=True)
    for t in (g["targets"], g["targets"][7:10], np.array([g["succ"][1], g["hubs"][-1]], I32)):
        a, b = up.run(t), on.run(t)
        assert same(a.dist, b.dist) and same(a.next, b.next) and a.levels == b.levels
        (sa, _, _), (sb, _, _) = up.count(a), on.count(b)
        assert same(sa, sb)
    assert same(b.dist, M.mirror_trees(g["adj"], t)[0])


def test_borrowed_device_csr_is_validated_at_creation():
    """the three create-time refusals on the on_device = 1 path: bad row pointer, column out of range, descending row"""
    rowptr = np.array([0, 2, 3, 3, 5], I32)
    col = np.array([1, 3, 0, 0, 2], I32)
    ok = Handle(rowptr, col, on_device=True)
    assert ok.rc == 0, err()
    ok.close()
    cases = [(np.array([0, 2, 3, 3, 6], I32), col, "rowptr is not a CSR row pointer"),
             (np.array([0, 3, 2, 3, 5], I32), col, "rowptr is not a CSR row pointer"),
             (np.array([1, 2, 3, 3, 5], I32), col, "rowptr is not a CSR row pointer"),
             (rowptr, np.array([1, 4, 0, 0, 2], I32), "a column index is outside [0, 4)"),
             (rowptr, np.array([-1, 3, 0, 0, 2], I32), "a column index is outside [0, 4)"),
             (rowptr, np.array([3, 1, 0, 0, 2], I32), "the columns of a row are not ascending"),
             (rowptr, np.array([1, 3, 0, 2, 0], I32), "the columns of a row are not ascending")]
    for rp, cl, words in cases:
        h = Handle(rp, cl, on_device=True)
        assert h.rc == EINVAL and not h.h.value and words in err(), (words, err())


@pytest.mark.parametrize("row", ["long", "short"])
def test_borrowed_csr_that_changes_is_refused_at_run_time(row):
    """flag 4 of paths_level_kernel, in the whole-wave path (a hub's row of 65 entries) and in the one-lane path (a successor's row):
    the first entry of the row of a non-target node becomes n, then -1, on the device -> gss_paths_run returns EINVAL with
    `paths_run: a column index is outside [0, n)`, the pads are intact, and with the entry back the run has its original bits"""
    g = tie_case(3)                                                        # L = 65, hubs at lanes 5 and 40
    n, t = g["n"], g["targets"]
    node = g["hubs"][1] if row == "long" else int(g["succ"][0])
    h = Handle.of(g["adj"], on_device=True)
    lens = np.diff(h.rowptr)
    assert (lens[node] > K.SHORT_ROW) == (row == "long") and node not in t.tolist()
    at = int(h.rowptr[node])
    kept = int(h.col[at])
    try:
        for bad in (n, -1):
            try:
                h.d_col[at] = bad
                r = h.run(t, expect=EINVAL)
                assert f"paths_run: a column index is outside [0, {n})" in err(), err()
            finally:
                h.d_col[at] = kept
            torch.cuda.synchronize()
            r = h.run(t)
            assert same(r.dist, g["dist"]) and same(r.next, g["next"]) and r.levels == 2
    finally:
        h.d_col[at] = kept
        torch.cuda.synchronize()
        h.close()


# ---- gss_paths_count -------------------------------------------------------------------------------------------------------------------

REFUSED = r"paths_count: node {v} has more than 2^53 shortest paths to target 0 (node 0)"


@pytest.mark.parametrize("path", ["one_lane", "whole_wave"])
def test_count_boundary_two_to_the_53_accepted_one_more_refused(path, handles):
    """add_count at its two boundaries, in the one-lane loop (top row of 8 / 9 entries) and in the whole-wave path (64 / 65 entries: the
    strided loop, the butterfly and the `__ballot(rover)` that hands the verdict to the owner): a sum of exactly 2^53 is accepted; 2^53 + 1,
    which rounds to even back to 2^53 and is caught only by `__dsub_rn(s, a) != b`, is refused naming the top node, with the extra
    entry first and last in the row.  The pads of sigma are intact after the refusals."""
    widths = K.ONE_LANE_WIDTHS if path == "one_lane" else K.WHOLE_WAVE_WIDTHS
    t = np.array([0], I32)
    g = K.boundary_count_graph(widths, False)
    h = handles(g["adj"])
    r = h.run(t)
    md, ms, _, _ = T.mirror_toward(g["adj"], t)
    assert same(r.dist, md) and r.levels == len(widths) + 1 == int(md.max())
    sigma, _, _ = h.count(r)
    assert sigma[0, g["top"]] == 2.0 ** 53 and same(sigma, ms)
    w = K.tie_weights("int", 1, g["n"])
    sigma, best, bnext = h.count(r, w)
    _, _, mb, mnb = T.mirror_toward(g["adj"], t, w)
    assert same(sigma, ms) and same(best, mb) and same(bnext, mnb)
    for chain_first in (False, True):
        e = K.boundary_count_graph(widths, True, chain_first)
        he = handles(e["adj"])
        re_ = he.run(t)
        assert re_.levels == len(widths) + 1
        he.count(re_, expect=EINVAL)
        assert REFUSED.format(v=e["top"]) in err(), err()
        he.count(re_, K.tie_weights("int", 1, e["n"]), expect=EINVAL)
        assert REFUSED.format(v=e["top"]) in err(), err()


def test_count_far_above_the_limit_names_the_largest_node(handles):
    """the whole-wave path with sums far above 2^53 (`s > kMaxCount` in the butterfly), in the last layer (2^54) and at the top (2^60):
    the status word keeps the largest (code, target, node), so the top node is named"""
    g = K.boundary_count_graph(K.FAR_ABOVE_WIDTHS, False)
    h = handles(g["adj"])
    r = h.run(np.array([0], I32))
    h.count(r, expect=EINVAL)
    assert REFUSED.format(v=g["top"]) in err(), err()


def test_count_overflow_seen_by_one_lane_reaches_the_owner(handles):
    """`__ballot(rover)` of trace_level_kernel: lane 0 alone sums 2^53 + 1 (positions 0 and 64 of a row of 65 whose other entries cannot
    reach the target), every butterfly sum is 2^53 + 0 and exact, and the row's owner is lane 43: refused, naming the apex"""
    g = K.lane_local_overcount_graph()
    h = handles(g["adj"])
    r = h.run(np.array([0], I32))
    assert r.dist[0, g["apex"]] == 11 and r.levels == 11
    h.count(r, expect=EINVAL)
    assert REFUSED.format(v=g["apex"]) in err(), err()


def test_count_duplicate_check_at_the_row_boundaries(handles):
    """trace_duplicate_kernel: equal neighbours in col[] across a row boundary, directly and over runs of empty rows, are no repeat (the
    binary search for the row of an entry, `rowptr[lo] < i`); a true repeat in the first non-empty row, in the last row, in a row behind
    empty rows, and in two rows at once (the larger row index wins the status word) is refused naming the row"""
    t = K.ROW_BOUNDARY_TARGETS
    rowptr, col = K.row_boundary_graph()
    h = handles(rowptr, col)
    assert h.rc == 0, err()
    r = h.run(t)
    adj = K.csr_of(rowptr, col)
    md, ms, _, _ = T.mirror_toward(adj, t)
    assert same(r.dist, md) and same(r.next, M.mirror_trees(adj, t)[1]) and r.levels == int(md[md != 255].max())
    sigma, _, _ = h.count(r)
    assert same(sigma, ms)
    for variant, row in (("first", 2), ("last", 19), ("after_empty", 7), ("two", 13)):
        hv = handles(*K.row_boundary_graph(variant))
        assert hv.rc == 0, err()                                          # the handle accepts it: its tie rule needs no strict order
        rv = hv.run(t)
        assert same(rv.dist, md)
        hv.count(rv, expect=EINVAL)
        assert f"paths_count: row {row} of the graph holds a column twice" in err(), (variant, err())


def test_count_status_word_keeps_the_largest_target_then_node(handles):
    """report(): the largest (code, target, node) wins -- non-finite weights at (target 0, node 5) and (target 1, node 2) name target 1,
    node 2, whichever lane reports first; a duplicate row (code 1) loses to a weight (code 4)"""
    g = K.tie_weight_graph()
    h = handles(g["adj"])
    r = h.run(g["targets"])
    w = np.zeros((2, g["n"]))
    w[0, 5], w[1, 2] = np.nan, np.inf
    for _ in range(2):
        h.count(r, w, expect=EINVAL)
        assert "paths_count: the weight of node 2 for target 1 (node 1) is not finite" in err(), err()
    w[1, 2] = 0.0
    h.count(r, w, expect=EINVAL)
    assert "paths_count: the weight of node 5 for target 0 (node 0) is not finite" in err(), err()
    rowptr, col = K.row_boundary_graph("two")
    hd = handles(rowptr, col)
    rd = hd.run(K.ROW_BOUNDARY_TARGETS)
    wd = np.zeros((3, 20))
    wd[2, 1] = -np.inf
    hd.count(rd, wd, expect=EINVAL)
    assert "the weight of node 1 for target 2 (node 0) is not finite" in err(), err()


@pytest.mark.parametrize("kind", ["zero", "int"])
def test_count_best_ties_on_rows_of_33_64_65(kind, handles):
    """beats() in the strided loop and in the butterfly of trace_level_kernel on rows of 33, 64 and 65 successors that are all one hop
    closer: equal values everywhere (only +0.0 / -0.0; small integers), the smallest index wins; best compared as int64 bits, so a -0.0
    for a +0.0 shows.  The integer table puts its largest value at positions 63 and 64 for target 0 (lane 63 against lane 0's second
    entry: the smaller index has to win through the butterfly) and at position 64 alone for target 1 (only the row of 65 sees it)"""
    g = K.tie_weight_graph()
    h = handles(g["adj"])
    r = h.run(g["targets"])
    w = K.tie_weight_tables(g, kind)
    md, ms, mb, mnb = T.mirror_toward(g["adj"], g["targets"], w)
    assert same(r.dist, md) and r.levels == 3
    sigma, best, bnext = h.count(r, w)
    assert same(sigma, ms)
    assert same(bnext, mnb), [(q, v, bnext[q, v], mnb[q, v]) for q, v in np.argwhere(bnext != mnb)[:8]]
    assert same(best, mb)
    for hub in g["hubs"].values():
        assert (bnext[:, hub] >= g["layer"][0]).all()


@pytest.mark.parametrize("i", [1, 3, 6], ids=["L33", "L65", "L200"])
def test_count_on_the_tie_rule_graphs(i, handles):
    """the counts of the hubs (whole-wave rows in which most entries are NOT one hop closer and are skipped) against the mirror, with
    integer weights"""
    g = tie_case(i)
    h = handles(g["adj"])
    r = h.run(g["targets"])
    w = K.tie_weights("int", 64, g["n"])
    _, ms, mb, mnb = T.mirror_toward(g["adj"], g["targets"], w)
    sigma, best, bnext = h.count(r, w)
    assert same(sigma, ms) and same(best, mb) and same(bnext, mnb)
    assert sigma[:, g["hubs"][0]].max() >= 2


# ---- gss_paths_between / gss_paths_between_fill ----------------------------------------------------------------------------------------

class Between:
    """between_graph with the mirror's dist / sigma of all 64 sources and targets on the device"""

    def __init__(self):
        g = K.between_graph()
        self.g, self.n, self.adj = g, g["n"], g["adj"]
        self.sources, self.targets = g["sources"], g["targets"]
        self.ds, self.ss = T.mirror_from(self.adj, self.sources)
        self.dt, self.st, _, _ = T.mirror_toward(self.adj, self.targets)
        self.dev = None

    def ids(self, ns, nt, s0=0):
        """the nine leading arguments for sources s0 .. s0 + ns and targets 0 .. nt"""
        if self.dev is None:
            self.dev = [dev(x) for x in (self.ds, self.ss, self.dt, self.st)]
        ds, ss, dt, st = self.dev
        src = np.ascontiguousarray(self.sources[s0:s0 + ns] if ns <= 64 else np.zeros(ns, I32))
        tgt = np.ascontiguousarray(self.targets[:nt])
        self.keep = (src, tgt)
        return (self.n, ns, src.ctypes.data, ds[s0:].data_ptr(), ss[s0:].data_ptr(), nt, tgt.ctypes.data, dt.data_ptr(), st.data_ptr())

    @functools.lru_cache(maxsize=None)
    def mirror(self, ns, nt, pairs=()):
        return T.mirror_between(self.adj, self.sources[:ns], self.targets[:nt], list(pairs))


@functools.lru_cache(maxsize=None)
def between():
    return Between()


def run_between(b, ns, nt, med=True, s0=0, med_bufs=None):
    lib = _lib.load()
    plen, ppaths, pnodes = Buf(ns * nt, I32), Buf(ns * nt, F64), Buf(ns * nt, I32)
    msum, mcnt = med_bufs or ((Buf(nt * b.n, F64).zero(), Buf(nt * b.n, I32).zero()) if med else (None, None))
    rc = lib.gss_paths_between(*b.ids(ns, nt, s0), plen.ptr, ppaths.ptr, pnodes.ptr, msum.ptr if msum else None,
                               mcnt.ptr if mcnt else None, stream())
    assert rc == 0, err()
    out = [plen.host("pair_len").reshape(ns, nt), ppaths.host("pair_paths").reshape(ns, nt), pnodes.host("pair_nodes").reshape(ns, nt)]
    if msum:
        out += [msum.host("med_sum").reshape(nt, b.n), mcnt.host("med_count").reshape(nt, b.n)]
    return out


@pytest.mark.parametrize("ns,nt", K.BETWEEN_PASSES)
def test_between_pair_tables_and_mediators(ns, nt):
    """trace_pair_kernel and trace_mediator_kernel on passes of (1, 1), (3, 5) and (64, 64): the three pair tables and the mediators
    bit-equal to mirror_between; with med_sum = med_count = NULL (the mediator launch skipped) the pair tables have the same bits;
    one of the two alone is refused"""
    b = between()
    m = b.mirror(ns, nt)
    plen, ppaths, pnodes, msum, mcnt = run_between(b, ns, nt)
    assert same(plen, m["length"]) and same(ppaths, m["n_paths"]) and same(pnodes, m["n_nodes"])
    assert same(msum, m["mediators"][0]) and same(mcnt, m["mediators"][1])
    if nt > 1:
        assert (plen == -1).any() and (mcnt > 0).any()
    bare = run_between(b, ns, nt, med=False)
    assert len(bare) == 3 and all(same(x, y) for x, y in zip(bare, (plen, ppaths, pnodes)))
    lib = _lib.load()
    one, outs = Buf(nt * b.n, F64).zero(), [Buf(ns * nt, k) for k in (I32, F64, I32)]
    for msum_, mcnt_ in ((one.ptr, None), (None, Buf(nt * b.n, I32).zero().ptr)):
        assert lib.gss_paths_between(*b.ids(ns, nt), *(o.ptr for o in outs), msum_, mcnt_, stream()) == EINVAL
        assert "med_sum and med_count are given together or not at all" in err(), err()
    assert all(o.unwritten().all() for o in outs) and (bits(one.host()) == 0).all()


def test_between_mediators_continue_across_passes_of_sources():
    """sources cut into passes of 2 + 1 (the `first` read-modify-write of trace_mediator_kernel) give the bits of one pass of 3"""
    b = between()
    nt = 5
    whole = run_between(b, 3, nt)
    bufs = (Buf(nt * b.n, F64).zero(), Buf(nt * b.n, I32).zero())
    first = run_between(b, 2, nt, med_bufs=bufs)
    second = run_between(b, 1, nt, s0=2, med_bufs=bufs)
    assert same(second[3], whole[3]) and same(second[4], whole[4])
    assert same(np.vstack([first[0], second[0]]), whole[0]) and same(np.vstack([first[1], second[1]]), whole[1])
    assert (first[4] != whole[4]).any()                                   # the third source does contribute


FILL_KINDS = (I32, U8, U8, F64, F64, F64)                                 # node, hops_from, hops_to, paths_from, through, share
FILL_NAMES = ("node", "hops_from", "hops_to", "paths_from", "through", "share")
FILL_NS, FILL_NT = 3, 5
FILL_PAIRS = (K.PAIR_MANY, K.PAIR_SINGLE, K.PAIR_SAME, K.PAIR_UNREACHABLE, K.PAIR_HALF, (0, 4), K.PAIR_MANY)


def run_fill(b, pairs, offset, capacity, alloc, expect=0, null=(), ns=FILL_NS, n_pairs=None):
    """gss_paths_between_fill into six outputs of `alloc` entries each -> the Bufs (raw: sentinels where nothing was written)"""
    lib = _lib.load()
    outs = [Buf(alloc, k) for k in FILL_KINDS]
    d_pairs = dev(np.asarray(pairs, I32).reshape(-1, 2)) if len(pairs) else None
    d_off = dev(np.asarray(offset, np.int64)) if len(offset) else None
    ptrs = [None if i in null else o.ptr for i, o in enumerate(outs)]
    rc = lib.gss_paths_between_fill(*b.ids(ns, FILL_NT), len(pairs) if n_pairs is None else n_pairs, _lib.ptr(d_pairs), _lib.ptr(d_off),
                                    capacity, *ptrs, stream())
    torch.cuda.synchronize()
    assert rc == expect, err()
    return outs


def fill_reference(b, pairs):
    """offset (exclusive scan of the mirror's node counts) and the six mirror tables laid out at it"""
    m = b.mirror(FILL_NS, FILL_NT, tuple(sorted(set(p for p in pairs if 0 <= p[0] < FILL_NS and 0 <= p[1] < FILL_NT))))
    counts = [int(m["n_nodes"][p]) if p in m["tables"] else 0 for p in pairs]
    offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    cols = [np.concatenate([m["tables"][p][c] for p in pairs if p in m["tables"]]) for c in range(6)]
    return offset, counts, cols


def test_fill_whole_tables():
    """trace_fill_kernel with capacity = the total: the six tables of seven pairs -- many routes over both 256-node iterations (the
    compaction carries `base` across them), one route, source = target (one row: hops 0 / 0, share 1), an unreachable pair (nothing),
    a pair listed twice (both ranges alike) -- equal the mirror's; all six pads intact"""
    b = between()
    offset, counts, cols = fill_reference(b, FILL_PAIRS)
    total = int(offset[-1])
    assert counts[3] == 0 and counts[2] == 1 and counts[0] == counts[6] > K.FILL_NODES // 2
    outs = run_fill(b, FILL_PAIRS, offset, total, total)
    for o, want, name in zip(outs, cols, FILL_NAMES):
        assert same(o.host(name), want), name
    node, hf, ht, pf, th, sh = (o.host() for o in outs)
    at = int(offset[2])
    assert (node[at], hf[at], ht[at], pf[at], th[at], sh[at]) == (b.sources[2], 0, 0, 1.0, 1.0, 1.0)
    for x in (node, hf, ht, pf, th, sh):
        assert same(x[offset[0]:offset[1]], x[offset[6]:offset[7]])
    for lo, hi in zip(offset[:-1], offset[1:]):
        assert (np.diff(node[lo:hi]) > 0).all()
    # a pass of 64 x 64 with 64 pairs over all of it
    pairs = [(i, (5 * i) % 64) for i in range(64)]
    m = T.mirror_between(b.adj, b.sources, b.targets, pairs)
    off = np.concatenate([[0], np.cumsum([m["n_nodes"][p] for p in pairs])]).astype(np.int64)
    lib = _lib.load()
    big = [Buf(off[-1], k) for k in FILL_KINDS]
    ids = b.ids(64, 64)
    d_pairs, d_off = dev(np.array(pairs, I32)), dev(off)
    assert lib.gss_paths_between_fill(*ids, 64, d_pairs.data_ptr(), d_off.data_ptr(), int(off[-1]), *(o.ptr for o in big), stream()) == 0, err()
    for c, (o, name) in enumerate(zip(big, FILL_NAMES)):
        assert same(o.host(name), np.concatenate([m["tables"][p][c] for p in pairs])), name


def test_fill_writes_nothing_at_or_beyond_capacity():
    """`end = min(offset[p + 1], cap)` of trace_fill_kernel: with capacity = total - 1, total - (count of the last pair) and one less
    (the cut inside the last pair, exactly between two pairs, inside the pair before), every entry below capacity has the bits of the
    full run and every entry at or beyond it keeps the sentinel, in all six arrays.  The outputs have the full size whatever capacity
    is: a wrong clip damages sentinels, never memory outside the buffers."""
    b = between()
    offset, counts, cols = fill_reference(b, FILL_PAIRS)
    total = int(offset[-1])
    for cap in (total - 1, total - counts[-1], total - counts[-1] - 1):
        assert 0 < cap < total
        outs = run_fill(b, FILL_PAIRS, offset, cap, total)
        for o, want, name in zip(outs, cols, FILL_NAMES):
            raw = o.host(name)
            assert same(raw[:cap], want[:cap]), (name, cap)
            assert o.unwritten(name)[cap:].all(), (name, cap, np.nonzero(~o.unwritten(name)[cap:])[0][:8] + cap)


def test_fill_ranges_shorter_than_the_pair_and_pairs_outside_the_pass():
    """the caller's offsets are the limit of a pair: a range shorter than the pair's node count holds its first nodes in ascending order
    and the neighbour's range is untouched by it; pair positions (ns, 0), (0, nt) and (-1, 0) (the early return of trace_fill_kernel)
    and the unreachable pair write nothing in the ranges they are given and do not disturb the others"""
    b = between()
    pairs = [K.PAIR_MANY, K.PAIR_HALF, (FILL_NS, 0), K.PAIR_SINGLE, (0, FILL_NT), K.PAIR_UNREACHABLE, (-1, 0), K.PAIR_SAME]
    _, counts, _ = fill_reference(b, pairs)
    m = b.mirror(FILL_NS, FILL_NT, tuple(sorted({K.PAIR_MANY, K.PAIR_HALF, K.PAIR_SINGLE, K.PAIR_SAME, K.PAIR_UNREACHABLE})))
    assert counts[0] > 40 and counts[1] > 3
    lens = [40, counts[1], 4, 3, 4, 5, 4, 1]                              # MANY cut to 40, SINGLE (6 nodes) cut to 3; 4 / 4 / 5 / 4 to stay empty
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(offset[-1])
    outs = run_fill(b, pairs, offset, total, total)
    for c, (o, name) in enumerate(zip(outs, FILL_NAMES)):
        raw, free = o.host(name), o.unwritten(name)
        for p, pair in enumerate(pairs):
            lo, hi = int(offset[p]), int(offset[p + 1])
            if pair in m["tables"] and len(m["tables"][pair][c]):
                assert same(raw[lo:hi], m["tables"][pair][c][:hi - lo]), (name, pair)
            else:
                assert free[lo:hi].all(), (name, pair)
    node = outs[0].host()
    assert (np.diff(node[:40]) > 0).all() and node[40] == m["tables"][K.PAIR_HALF][0][0]


def test_fill_with_nothing_to_do_and_refusals():
    """n_pairs = 0 and capacity = 0 return 0 and write nothing, also with null outputs; refused by name: n_pairs = 4097, capacity = -1,
    a null output with work to do, S = 65 sources"""
    b = between()
    offset, counts, cols = fill_reference(b, FILL_PAIRS)
    total = int(offset[-1])
    every = range(6)
    for pairs, off, cap, null in (((), (), total, ()), ((), (), total, every), (FILL_PAIRS, offset, 0, ()), (FILL_PAIRS, offset, 0, every),
                                  ((), (), 0, every)):
        outs = run_fill(b, pairs, off, cap, total, null=null)
        assert all(o.unwritten(name).all() for o, name in zip(outs, FILL_NAMES))
    refused = [(dict(n_pairs=4097), "paths_between_fill: 4097 pairs; a pass has at most 4096"),
               (dict(n_pairs=-1), "paths_between_fill: -1 pairs; a pass has at most 4096"),
               (dict(capacity=-1), "paths_between_fill: capacity=-1 is negative"),
               (dict(null=(0,)), "paths_between_fill: null argument"),
               (dict(null=(5,)), "paths_between_fill: null argument"),
               (dict(ns=65), "paths_between_fill: S=65 sources; a pass takes 1 to 64")]
    for kw, words in refused:
        cap = kw.pop("capacity", total)
        outs = run_fill(b, FILL_PAIRS, offset, cap, total, expect=EINVAL, **kw)
        assert words in err(), (words, err())
        assert all(o.unwritten(name).all() for o, name in zip(outs, FILL_NAMES)), words
    outs = run_fill(b, FILL_PAIRS, offset, total, total)                  # and the valid call still has its bits
    assert all(same(o.host(name), want) for o, want, name in zip(outs, cols, FILL_NAMES))
