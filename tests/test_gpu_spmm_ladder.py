"""-m gpu: spmm_balanced_kernel (csrc/spmm.hip) at every block class of its schedule, exactly.

Every SpMM mode runs through one body, spmm_balanced_block, and how it sums a row depends on the row's block class (csrc/segments.h):
p = 1 lane group, 1 < p <= GPW groups combined by the xor-shuffle ladder inside a wave, p > GPW combined through part[] in LDS by the
block's first wave, and the whole workgroup with longer segments.  The graphs of the other op-by-op suites hold rows of at most 17 and of
600+ entries only; the ladder graph of tests/spmm_ladder_cases.py holds a length below, on and above every power of two of segments, and
its operands are small integers, so that every sum is exact in fp32 whatever its order: the device result must EQUAL the int64 reference
(scipy, no project code) on every element -- np.array_equal, no tolerance.  The one exception: dp on the four planted elements of the
planted rows (p = +0, -0, tiny, -20), held to sparse_hop_mirror.bound like in the other hop suites.  Outputs are pre-filled with a NaN of
a known payload: a written row holds it nowhere, a skipped row everywhere.  tests/test_spmm_ladder_cases.py asserts on the CPU that the
graphs reach the classes claimed here.  A failing comparison names the rows' lengths and their block class at the launch's width.

Widths 16 ... 1024: one per lane-group class, plus 64.  At 8320 operand rows the automatic policy cuts d >= 256 into feature slices of
64 or 128 floats (16- and 32-lane groups); "whole" (spmm_slices = 1) is what reaches the 64-lane classes those widths stand for, "auto"
what a plan would launch.

Why each combine path is red if it is lost (argued from spmm_balanced_block / launch_giant, not demonstrated):
  * the `pcount > o` ladder.  Without the guard a group adds its neighbour blocks' sums: every row of fewer than GPW groups that shares
    a wave differs (all short rows at d <= 128).  A ladder one step short leaves the blocks of exactly GPW groups with half their
    segments: rows of 257..512 entries at d = 16, 129..256 at d = 32, 65..128 at d = 48 / 64, 33..64 at d = 128.  A guard that is right
    per wave but not per lane group fails in the wave that mixes block sizes (d <= 64).  Red: test_every_mode_once[plain-...] at those
    widths, naming plog <= log2 GPW, 1 wave per block.
  * the part[] sum.  A lost slot (k < nw - 1, a wrong wave index, a missing barrier) drops or replaces the segments of one wave of every
    block with p > GPW: rows above 32 GPW entries differ by integers.  Red: the same tests, naming 2 .. 16 waves per block -- the
    two-wave block of d = 128 (65..128 entries) and plog 8 of d = 16 (4097..8192) among them.
  * y_in added once in the multi-wave epilogue.  Added per slot, by every wave, or not at all, a multi-wave row of the second pass is
    off by a multiple of the first pass's sum.  Red: test_second_pass_in_place, on rows whose second half spans several waves; the
    in-wave rows of the same launch stay green, which separates it from the part[] sum.
  * an empty segment inside a block (e1 == e0 after the row's last entry: 513, 1025, 2049, 4097 entries, 8193 at d = 32).  It must add
    zero and still take part in the ladder and the barrier; a group that walked on into the next row's entries (the two-pair loads of
    the narrow groups prefetch behind e1) would add them.  Red: test_every_mode_once at d <= 128 naming those lengths, "1 empty
    segment(s)".
  * the finish pass over chunk sums.  Under spmm_giant = 64 a row above 64 entries is the sum of its chunks' sums, gathered by a
    [rows] x [chunks] matrix of ones over the scratch; a chunk lost at a chunk edge (80 = 5 chunks, 81 = 5 chunks + 1 entry), a stale
    scratch row or y_in added in both the short and the finish pass shows on every giant row.  Red: test_giant_rows_change_no_bit.
No test provokes a fault: every launch gets valid arguments."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import sparse_hop_mirror as M
import spmm_ladder_cases as L
from gpu_hop_common import G, cu, dev_csr, fully_written, host, knobs, prefilled, ptr, torch, untouched  # noqa: F401 (G: the fixture)

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5
WIDE = (256, 512, 1024)          # the widths the automatic policy slices at 8320 operand rows
ON_BOTH = [(kind, d, how) for kind in L.KINDS for d in L.WIDTHS for how in (("whole", "auto") if kind == "ladder" and d in WIDE else ("whole",))]
ON_LADDER = [(d, how) for kind, d, how in ON_BOTH if kind == "ladder"]
MODES = ("plain", "fwd1", "bwd1", "bwd2", "bwd1s", "bwd2s")
DENSE = ("plain", "fwd1", "bwd1", "bwd2")
GATHERED = {"plain": "x0", "fwd1": "x0", "bwd1": "x1", "bwd2": "x0", "bwd2s": "x0z"}      # the operand a mode gathers from
IN_PLACE = {"plain": 0, "fwd1": 0, "bwd1": 1, "bwd2": 0, "bwd2s": 0}                      # the output y_in aliases: y, y, t, dp, dp
_DEV = {}


# ---------------------------------------------------------------- inputs on the device
def dv(kind, d, name):
    key = (kind, d, name)
    if key not in _DEV:
        _DEV[key] = cu(L.masked_operand(kind, d, name) if name in ("x0z", "tz") else L.operand(kind, d, name))
    return _DEV[key]


def sparse_dv(kind, d):
    key = (kind, d, "sparse")
    if key not in _DEV:
        g, cs, r2 = L.graph(kind), L.bwd1s_case(kind, d), L.bwd2s_ref(kind, d)
        nz0 = np.zeros(M.words_for(g.n_cols) + 2, np.uint32)          # a plan's bitmap: own rows clear, halo bits and padding set, guard words
        nz0[:-2] = M.bits_fill(nz0[:-2], g.n_rows, (len(nz0) - 2) * 32)
        nz0[-2:] = GUARD
        _DEV[key] = dict(g_am_b=cu(cs.g_am_b), g_ax_b=cu(cs.g_ax_b), pos=cu(cs.pos), pos_row=cu(cs.pos_row),
                         posbits=cu(M.pack_bits(cs.ids, g.n_cols)), live=cu(M.pack_bits(np.flatnonzero(cs.live), g.n_rows)), nz0=nz0,
                         res_b=cu(r2.res_b), pos_row2=cu(r2.pos_row), nzbits=cu(M.pack_bits(np.flatnonzero(L.inside(kind)), g.n_cols)))
    return _DEV[key]


def csr_of(G, kind, which="all", tag=""):
    return dev_csr(G, L.part(kind, which), ("ladder suite", kind, which, tag))


@contextlib.contextmanager
def sliced(G, kind, d, how):
    """how: "whole" (one slice), "auto" (the policy's choice), or (slices, pin).  Yields log2 of the groups per wave of the launch"""
    if how == "auto":
        ns, pin = C.c_int32(-1), C.c_int32(-1)
        G._lib.check(G.lib.gss_spmm_auto_slices(d, L.graph(kind).n_cols, C.byref(ns), C.byref(pin)))
        assert ns.value > 1, "the automatic policy no longer slices this width: the case is the `whole` one"
        yield L.gpw_log2_of(d, ns.value)
    elif how == "whole":
        with knobs(G, spmm_slices=1):
            yield L.gpw_log2_of(d)
    else:
        assert (d // 4) % how[0] == 0 and d // 4 // how[0] >= 4
        with knobs(G, spmm_slices=how[0], spmm_pin=how[1]):
            yield L.gpw_log2_of(d, how[0])


# ---------------------------------------------------------------- one launch of a mode
def run(G, mode, kind, d, which="all", y_in=None, tag="", res=True, gx=True, plan=False, nzbits=False, x="x0", h="h"):
    """-> the mode's outputs on the host (None for one not asked for).  y_in: the first pass's sums IN the buffer this pass writes
    (IN_PLACE).  plan (bwd1s): posbits, nzbits_out, skip_zero_rows and live_rows, as a single-shard plan runs it -> + the bitmap"""
    g = L.graph(kind)
    csr = csr_of(G, kind, which, tag)
    n, st, lib, chk = g.n_rows, G.st(), G.lib, G._lib.check
    o0 = y_in if y_in is not None and IN_PLACE[mode] == 0 else prefilled(n, d)
    o1 = y_in if y_in is not None and IN_PLACE[mode] == 1 else prefilled(n, d)
    if mode in ("plain", "fwd1"):
        fused = mode == "fwd1"
        if y_in is None:
            chk(lib.gss_spmm(csr.handle, d, ptr(dv(kind, d, x)), ptr(o0), ptr(dv(kind, d, h)) if fused else None, ptr(o1) if fused else None, st))
        else:
            chk(lib.gss_spmm_add(csr.handle, d, ptr(dv(kind, d, x)), ptr(y_in), ptr(o0), ptr(dv(kind, d, h)) if fused else None,
                                 ptr(o1) if fused else None, st))
        return host(o0), host(o1)
    if mode == "bwd1":
        chk(lib.gss_spmm_bwd1_ex(csr.handle, d, ptr(dv(kind, d, "x1")), ptr(dv(kind, d, "g_ax")), ptr(dv(kind, d, "x_in")), ptr(dv(kind, d, "ax")),
                                 ptr(o0), ptr(o1), ptr(y_in), st))
        return host(o0), host(o1)
    if mode == "bwd2":
        chk(lib.gss_spmm_bwd2_ex(csr.handle, d, ptr(dv(kind, d, "x0")), ptr(dv(kind, d, "t")), ptr(dv(kind, d, "p")), L.C,
                                 ptr(dv(kind, d, "res")) if res else None, ptr(o0), ptr(o1) if gx else None, ptr(y_in), 0, st))
        return host(o0), host(o1)
    sd = sparse_dv(kind, d)
    if mode == "bwd1s":
        nz = cu(sd["nz0"]) if plan else None
        chk(lib.gss_spmm_bwd1_sparse_ex(csr.handle, d, ptr(sd["g_am_b"]), ptr(sd["g_ax_b"]), ptr(sd["pos"]), ptr(sd["pos_row"]), ptr(dv(kind, d, "x_in")),
                                        ptr(dv(kind, d, "ax")), ptr(o0), ptr(o1), ptr(sd["posbits"]) if plan else None, ptr(nz), int(plan),
                                        ptr(sd["live"]) if plan else None, st))
        return host(o0), host(o1), (host(nz) if plan else None)
    assert mode == "bwd2s"
    chk(lib.gss_spmm_bwd2_sparse_res(csr.handle, d, ptr(dv(kind, d, "x0z")), ptr(dv(kind, d, "tz")), ptr(dv(kind, d, "p")), L.C, ptr(sd["res_b"]),
                                     ptr(sd["pos_row2"]), ptr(o0), ptr(o1) if gx else None, ptr(sd["nzbits"]) if nzbits else None, ptr(y_in), 0, st))
    return host(o0), host(o1)


def first_pass(G, mode, kind, d, tag=""):
    """the plain product of the first column half into a fresh buffer: what a plan's overlapped hop launches first"""
    buf = prefilled(L.graph(kind).n_rows, d)
    G._lib.check(G.lib.gss_spmm(csr_of(G, kind, "first", tag).handle, d, ptr(dv(kind, d, GATHERED[mode])), ptr(buf), None, None, G.st()))
    return buf


# ---------------------------------------------------------------- the checks
def exact(got, ref, lens, gl, what, rows=None, skip=None):
    """equal in value on every element (of `rows`; but for the elements `skip`); the message names the failing rows' block classes"""
    bad = got.astype(np.float64) != np.asarray(ref, np.float64)       # (the pre-fill, a NaN, equals nothing)
    if skip is not None:
        bad &= ~skip
    bad = bad.any(1)
    if rows is not None:
        bad &= rows
    assert not bad.any(), f"{what}: not the integer reference in " + L.describe(lens, np.flatnonzero(bad), gl)


def write_set(got, written, what):
    assert untouched(got)[~written].all(), f"{what}: a row the contract skips was written: {np.flatnonzero(~untouched(got) & ~written)[:8]}"
    assert fully_written(got)[written].all(), f"{what}: a written row keeps the pre-fill: rows {np.flatnonzero(~fully_written(got) & written)[:8]}"


def check_dp(got, ref, kind, lens, gl, what):
    """dp: exact but for the four planted elements of the planted rows, which get the mirror's bound"""
    g = L.graph(kind)
    planted = np.zeros(got.shape, bool)
    planted[list(L.plant_rows(g)), :4] = True
    exact(got, ref.dp, lens, gl, what + " dp", skip=planted)
    err = np.abs(got.astype(np.float64) - ref.dp)
    assert (err[planted] <= M.bound(ref.k, ref.s_dp)[planted]).all(), f"{what}: dp beyond (k + 4) 2^-24 S on a planted element"


def check(mode, out, kind, d, gl, what, lens=None, two_pass=False, res=True, gx=True, plan=False, x="x0", h="h"):
    g = L.graph(kind)
    lens = g.lens if lens is None else lens
    every = np.ones(g.n_rows, bool)
    none = ~every
    if mode in ("plain", "fwd1"):
        ref = L.fwd_ref(kind, d, x, h)
        write_set(out[0], every, what + " y")
        exact(out[0], ref.y, lens, gl, what + " y")
        write_set(out[1], every if mode == "fwd1" else none, what + " m")
        if mode == "fwd1":
            exact(out[1], ref.m, lens, gl, what + " m")
    elif mode == "bwd1":
        ref = L.bwd1_ref(kind, d)
        for k, name in enumerate("ut"):
            write_set(out[k], every, f"{what} {name}")
            exact(out[k], getattr(ref, name), lens, gl, f"{what} {name}")
    elif mode == "bwd2":
        ref = L.bwd2_ref(kind, d, res, two_pass)
        write_set(out[0], every, what + " dp")
        check_dp(out[0], ref, kind, lens, gl, what)
        write_set(out[1], every if gx else none, what + " gx")
        if gx:
            exact(out[1], ref.gx, lens, gl, what + " gx")
    elif mode == "bwd1s":
        gl = L.gpw_log2_of(d)                  # (the sparse mode is never sliced)
        ref = L.bwd1s_ref(kind, d)
        written = ref.nz if plan else every
        for k, name in enumerate("ut"):
            write_set(out[k], written, f"{what} {name}")
            exact(out[k], getattr(ref, name), lens, gl, f"{what} {name}", rows=written)
        if plan:
            nz0 = sparse_dv(kind, d)["nz0"]
            got = M.unpack_bits(out[2][:-2], g.n_rows)
            assert np.array_equal(got, ref.nz), f"{what}: nzbits_out differs in " + L.describe(lens, np.flatnonzero(got != ref.nz), gl)
            want = nz0.copy()
            want[:-2] |= M.pack_bits(np.flatnonzero(ref.nz), (len(nz0) - 2) * 32)
            assert np.array_equal(out[2], want), f"{what}: a bit outside [0, n_rows) changed"
    else:
        ref = L.bwd2s_ref(kind, d, two_pass)
        write_set(out[0], every, what + " dp")
        check_dp(out[0], ref, kind, lens, gl, what)
        write_set(out[1], every if gx else none, what + " gx")
        if gx:
            exact(out[1], ref.gx, lens, gl, what + " gx")


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


VARIANTS = {"plain": [{}], "fwd1": [{}], "bwd1": [{}],
            "bwd2": [dict(res=True, gx=True), dict(res=False, gx=True), dict(res=True, gx=False), dict(res=False, gx=False)],
            "bwd1s": [dict(plan=False), dict(plan=True)], "bwd2s": [dict(nzbits=False), dict(nzbits=True, gx=False), dict(nzbits=True)]}


def check_kw(kw):
    return {k: v for k, v in kw.items() if k != "nzbits"}


# ================================================================ a. every mode at every width; e. twice, the same bits
@pytest.mark.parametrize("kind,d,how", ON_BOTH)
@pytest.mark.parametrize("mode", MODES)
def test_every_mode_once(G, mode, kind, d, how):
    """one launch per option set of the mode (bwd2: with and without res and gx; bwd1s: the pos map alone, and as a single-shard plan
    runs it, whole and listed; bwd2s: without and with the non-zero-row bitmap): the write set, the integer reference, and the same
    bits from a second launch"""
    with sliced(G, kind, d, how) as gl:
        for kw in VARIANTS[mode]:
            for listing in ((0, 1) if kw.get("plan") else (2048,)):
                what = f"{mode} {kw} listing={listing}"
                with knobs(G, spmm_list_blocks=listing):
                    out = run(G, mode, kind, d, **kw)
                    again = run(G, mode, kind, d, **kw)
                check(mode, out, kind, d, gl, what, **check_kw(kw))
                assert same_bits(out, again), what + ": two launches differ"


# ================================================================ b. the second pass, in place
@pytest.mark.parametrize("d,how", ON_LADDER)
@pytest.mark.parametrize("mode", ["fwd1", "bwd1", "bwd2", "bwd2s"])
def test_second_pass_in_place(G, mode, d, how):
    """the entries split by column at n_cols // 3: gss_spmm of the first half into the output buffer, then the mode over the second
    half with y_in = that buffer.  Still exact -- and every row has another block class in either half than in the whole"""
    lens = np.diff(L.part("ladder", "second").indptr)
    with sliced(G, "ladder", d, how) as gl:
        for which in ("first", "second"):
            assert set(L.schedule(np.diff(L.part("ladder", which).indptr), gl).plog.tolist()) >= {1, 2, 3, 4}
        for kw in ([dict(nzbits=False), dict(nzbits=True)] if mode == "bwd2s" else [{}]):
            buf = first_pass(G, mode, "ladder", d)
            exact(host(buf), L.product("ladder", d, GATHERED[mode], "first"), np.diff(L.part("ladder", "first").indptr), gl, "first pass")
            out = run(G, mode, "ladder", d, which="second", y_in=buf, **kw)
            check(mode, out, "ladder", d, gl, f"{mode} second pass {kw}", lens=lens, two_pass=True)


# ================================================================ c. row-filtered and listed forms
@pytest.mark.parametrize("d", L.WIDTHS)
@pytest.mark.parametrize("form", ["row_pos", "row_bits", "fwd1 row_bits", "gather_bits"])
def test_filtered_forms(G, form, d):
    """the filter keeps the first row of every length and drops the second: the kept rows exact, the dropped ones untouched, with the
    live workgroups listed (spmm_list_blocks = 1) and dispatched whole (0).  gather_bits: over an operand that is zero outside the set"""
    g = L.graph("ladder")
    csr = csr_of(G, "ladder")
    fused = form.startswith("fwd1")
    with sliced(G, "ladder", d, "whole") as gl:
        if form == "gather_bits":
            y = prefilled(g.n_rows, d)
            G._lib.check(G.lib.gss_spmm_filtered(csr.handle, d, ptr(dv("ladder", d, "x0z")), ptr(y), None, None, None, None, None,
                                                 ptr(sparse_dv("ladder", d)["nzbits"]), G.st()))
            y = host(y)
            write_set(y, np.ones(g.n_rows, bool), form)
            exact(y, L.product("ladder", d, "x0z"), g.lens, gl, form)
            return
        row_pos = np.full(g.n_rows, -1, np.int32)
        row_pos[g.keep] = np.arange(int(g.keep.sum()), dtype=np.int32)
        d_pos = cu(row_pos) if form == "row_pos" else None
        d_bits = None if form == "row_pos" else cu(M.pack_bits(np.flatnonzero(g.keep), g.n_rows))
        ref = L.fwd_ref("ladder", d)
        outs = []
        for listing in (0, 1):
            y, m = prefilled(g.n_rows, d), prefilled(g.n_rows, d)
            with knobs(G, spmm_list_blocks=listing):
                G._lib.check(G.lib.gss_spmm_filtered(csr.handle, d, ptr(dv("ladder", d, "x0")), ptr(y), ptr(dv("ladder", d, "h")) if fused else None,
                                                     ptr(m) if fused else None, ptr(d_pos), ptr(d_bits), None, None, G.st()))
            y, m = host(y), host(m)
            what = f"{form} listing={listing}"
            write_set(y, g.keep, what + " y")
            exact(y, ref.y, g.lens, gl, what + " y", rows=g.keep)
            write_set(m, g.keep if fused else np.zeros(g.n_rows, bool), what + " m")
            if fused:
                exact(m, ref.m, g.lens, gl, what + " m", rows=g.keep)
            outs.append((y, m))
        assert same_bits(outs[0], outs[1]), form + ": listed and whole dispatch differ"


# ================================================================ d. schedule variants that must not change a bit of an exact result
GIANT_EXTRA = [(m, d, "whole") for m in ("bwd2s", "plain row_pos", "fwd1 row_bits") for d in (16, 128, 512)]


@pytest.mark.parametrize("mode,d,how", [(m, d, how) for m in DENSE + ("bwd1+y_in", "bwd2+y_in") for d, how in ON_LADDER] + GIANT_EXTRA)
def test_giant_rows_change_no_bit(G, mode, d, how):
    """spmm_giant = 64: every row above 64 entries -- almost every ladder row -- is summed chunk by chunk (chunk pass), the others by
    the short pass, and the finish pass adds the chunks' sums and runs the epilogue: the dense modes, their second pass in place (y_in
    once per row, in whichever pass owns the row), the row-filtered forms (a chunk is computed only for a kept row) and one sparse mode
    (which keeps the single schedule)"""
    g = L.graph("ladder")
    tag = "giant"     # handles of their own: a handle rebuilds its chunked views whenever the knob changes under it
    with sliced(G, "ladder", d, how) as gl, knobs(G, spmm_giant=L.GIANT):
        what = f"{mode}, chunked (spmm_giant = {L.GIANT})"
        if mode.endswith("+y_in"):
            m = mode[:4]
            buf = first_pass(G, m, "ladder", d, tag)
            out = run(G, m, "ladder", d, which="second", y_in=buf, tag=tag)
            check(m, out, "ladder", d, gl, what, lens=np.diff(L.part("ladder", "second").indptr), two_pass=True)
        elif " " in mode:
            fused = mode.startswith("fwd1")
            row_pos = np.full(g.n_rows, -1, np.int32)
            row_pos[g.keep] = np.arange(int(g.keep.sum()), dtype=np.int32)
            d_pos = None if fused else cu(row_pos)
            d_bits = cu(M.pack_bits(np.flatnonzero(g.keep), g.n_rows)) if fused else None
            ref = L.fwd_ref("ladder", d)
            for listing in (0, 1):
                y, m = prefilled(g.n_rows, d), prefilled(g.n_rows, d)
                with knobs(G, spmm_list_blocks=listing):
                    G._lib.check(G.lib.gss_spmm_filtered(csr_of(G, "ladder", "all", tag).handle, d, ptr(dv("ladder", d, "x0")), ptr(y),
                                                         ptr(dv("ladder", d, "h")) if fused else None, ptr(m) if fused else None, ptr(d_pos),
                                                         ptr(d_bits), None, None, G.st()))
                y, m = host(y), host(m)
                write_set(y, g.keep, f"{what} listing={listing} y")
                exact(y, ref.y, g.lens, gl, f"{what} listing={listing} y", rows=g.keep)
                write_set(m, g.keep if fused else np.zeros(g.n_rows, bool), f"{what} listing={listing} m")
                if fused:
                    exact(m, ref.m, g.lens, gl, f"{what} listing={listing} m", rows=g.keep)
        else:
            kw = dict(nzbits=True) if mode == "bwd2s" else {}
            out = run(G, mode, "ladder", d, tag=tag, **kw)
            check(mode, out, "ladder", d, gl, what)
        n_giant, n_chunks = C.c_int32(-1), C.c_int32(-1)
        G._lib.check(G.lib.gss_csr_giant_rows(csr_of(G, "ladder", "all", tag).handle, C.byref(n_giant), C.byref(n_chunks)))
        gi = L.giant_items(g.lens, L.GIANT)
        assert (n_giant.value, n_chunks.value) == (len(gi.rows), len(gi.chunks))


@pytest.mark.parametrize("d", [128, 512, 1024])
@pytest.mark.parametrize("slices,pin", [(2, 0), (2, 1), (4, 1), (8, 0)])
@pytest.mark.parametrize("mode", ["plain", "fwd1", "bwd1", "bwd2", "bwd2s", "bwd1+y_in", "bwd2+y_in"])
def test_feature_slices_change_no_bit(G, mode, slices, pin, d):
    """spmm_slices / spmm_pin: a sliced launch uses the narrower class's descriptors and addresses operands, y_in and outputs by slice"""
    with sliced(G, "ladder", d, (slices, pin)) as gl:
        if mode.endswith("+y_in"):
            m = mode[:4]
            buf = first_pass(G, m, "ladder", d)
            out = run(G, m, "ladder", d, which="second", y_in=buf)
            check(m, out, "ladder", d, gl, f"{mode} slices={slices} pin={pin}", lens=np.diff(L.part("ladder", "second").indptr), two_pass=True)
        else:
            kw = dict(nzbits=True) if mode == "bwd2s" else {}
            check(mode, run(G, mode, "ladder", d, **kw), "ladder", d, gl, f"{mode} slices={slices} pin={pin}")


@pytest.mark.parametrize("d", L.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_a_declared_hot_set_changes_no_bit(G, mode, d):
    """spmm_hot_rows: 0 declares no hot set; 5 and n_cols // 2 put hot rows in front of cold ones, which takes the launch to the
    instantiation with 64-bit offsets and non-temporal gathers of the cold rows"""
    g = L.graph("ladder")
    kw = dict(plan=True) if mode == "bwd1s" else dict(nzbits=True) if mode == "bwd2s" else {}
    with sliced(G, "ladder", d, "whole") as gl:
        for hot in (0, 5, g.n_cols // 2):
            with knobs(G, spmm_hot_rows=hot):
                out = run(G, mode, "ladder", d, **kw)
            check(mode, out, "ladder", d, gl, f"{mode} spmm_hot_rows={hot}", **check_kw(kw))


@pytest.mark.parametrize("kind,d,how", ON_BOTH)
@pytest.mark.parametrize("mode", ["plain", "fwd1"])
def test_the_paired_launch(G, mode, kind, d, how):
    """gss_spmm_fwd_pair: two products over one matrix in one launch, each exact on its own operands"""
    g = L.graph(kind)
    fused = mode == "fwd1"
    csr = csr_of(G, kind)
    with sliced(G, kind, d, how) as gl:
        y0, y1, m0, m1 = (prefilled(g.n_rows, d) for _ in range(4))
        paired = C.c_int32(-1)
        G._lib.check(G.lib.gss_spmm_fwd_pair(csr.handle, d, ptr(dv(kind, d, "x0")), ptr(y0), ptr(dv(kind, d, "h")) if fused else None,
                                             ptr(m0) if fused else None, ptr(dv(kind, d, "x1")), ptr(y1), ptr(dv(kind, d, "h1")) if fused else None,
                                             ptr(m1) if fused else None, None, 0, None, None, None, None, C.byref(paired), G.st()))
        assert paired.value == 1, "the launch was not paired"
        check(mode, (host(y0), host(m0)), kind, d, gl, f"{mode} first of the pair")
        check(mode, (host(y1), host(m1)), kind, d, gl, f"{mode} second of the pair", x="x1", h="h1")


@pytest.mark.parametrize("d", [16, 128, 512])
@pytest.mark.parametrize("mode", DENSE)
def test_the_row_per_wave_variant(G, mode, d):
    """spmm_variant = 1: spmm_rows_kernel up to 512 entries, spmm_long_kernel above (512 stays, 513 moves)"""
    g = L.graph("ladder")
    assert {512, 513} <= set(g.lens.tolist())
    with knobs(G, spmm_variant=1):
        out = run(G, mode, "ladder", d)
    check(mode, out, "ladder", d, L.gpw_log2_of(d), f"{mode} spmm_variant=1")
