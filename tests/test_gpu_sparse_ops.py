"""-m gpu: the row-sparse SpMM modes of csrc/spmm.hip, op by op, against their fp64 contract (tests/sparse_hop_mirror.py): SPMM_BWD1S
(gss_spmm_bwd1_sparse[_ex]), SPMM_BWD2S (gss_spmm_bwd2_sparse_res), the row- and gather-filtered forward products (gss_spmm_filtered),
the bitmap builders (gss_mark_rows_and_neighbours, gss_batch_bits, gss_bits_fill), the listed-workgroup dispatch (knob
spmm_list_blocks = 1) and gss_scatter_add_rows.

What every value check asserts is the mirror's derived bound, per element: |got - ref| <= (k + 4) 2^-24 S with k the row's contributing
entries and S the mode's expression over absolute values (sparse_hop_mirror.py; checked on the CPU in test_sparse_hop_mirror.py) --
no measured tolerance, and tight enough that one dropped or doubled entry of a degree-1 row fails.  Every output is pre-filled with a
NaN of a recognisable payload: rows the contract skips must still hold it bit for bit, rows it writes must hold it nowhere.
No test provokes a fault: every launch that runs gets valid arguments; the refusals are refused before any launch."""
import functools
import itertools

import numpy as np
import pytest

import sparse_hop_cases as K
import sparse_hop_mirror as M
from gpu_hop_common import G, PREFILL, assert_rows, cu, dev_csr, fully_written, host, knobs, prefilled, ptr, torch, untouched  # noqa: F401 (G: the fixture)

pytestmark = pytest.mark.gpu

GUARD = 0xA5A5A5A5                   # bitmap words behind the last one a kernel may touch


def bitmap_words(n_bits, n_clear):
    """a bitmap of n_bits bits: [0, n_clear) clear, every bit behind them set (a plan's halo bits and the padding), + 2 guard words"""
    w = np.zeros(M.words_for(n_bits) + 2, np.uint32)
    w[:-2] = M.bits_fill(w[:-2], n_clear, (len(w) - 2) * 32)
    w[-2:] = GUARD
    return w


# ================================================================ SPMM_BWD1S
@functools.lru_cache(maxsize=None)
def bwd1_ref(kind, d, b, inside, use_live):
    cs = K.bwd1_case(kind, d, b, inside)
    live = M.pack_bits(np.flatnonzero(K.live_rows_of(cs, extra=(1, cs.g.n_rows - 2))), cs.g.n_rows) if use_live else None
    return M.bwd1_sparse(cs.g.a, cs.g_am_b, cs.g_ax_b, cs.pos, cs.pos_row, cs.x_in, cs.ax, live_rows=live)


def bwd1_dev(cs):
    if not hasattr(cs, "dev"):
        cs.dev = {k: cu(getattr(cs, k)) for k in ("g_am_b", "g_ax_b", "pos", "pos_row", "x_in", "ax")}
    return cs.dev


def run_bwd1s(G, cs, posbits=False, nzbits=False, skip=False, live=False, entry="ex"):
    g, dv = cs.g, bwd1_dev(cs)
    csr = dev_csr(G, g.a, g.kind)
    u, t = prefilled(g.n_rows, cs.d), prefilled(g.n_rows, cs.d)
    pb = cu(M.pack_bits(cs.ids, g.n_cols)) if posbits else None
    nz0 = bitmap_words(g.n_cols, g.n_rows)
    nz = cu(nz0) if nzbits else None
    lv = cu(M.pack_bits(np.flatnonzero(K.live_rows_of(cs, extra=(1, g.n_rows - 2))), g.n_rows)) if live else None
    if entry == "ex":
        rc = G.lib.gss_spmm_bwd1_sparse_ex(csr.handle, cs.d, ptr(dv["g_am_b"]), ptr(dv["g_ax_b"]), ptr(dv["pos"]), ptr(dv["pos_row"]), ptr(dv["x_in"]),
                                           ptr(dv["ax"]), ptr(u), ptr(t), ptr(pb), ptr(nz), int(skip), ptr(lv), G.st())
    else:
        rc = G.lib.gss_spmm_bwd1_sparse(csr.handle, cs.d, ptr(dv["g_am_b"]), ptr(dv["g_ax_b"]), ptr(dv["pos"]), ptr(dv["pos_row"]), ptr(dv["x_in"]),
                                        ptr(dv["ax"]), ptr(u), ptr(t), G.st())
    G._lib.check(rc)
    return host(u), host(t), (host(nz) if nzbits else None), nz0


def check_bwd1s(out, ref, skip, g, what):
    u, t, nz, nz0 = out
    written = ref.nz if skip else np.ones(g.n_rows, bool)
    assert_rows(u, ref.u, ref.s_u, ref.k, written, what + " u")
    assert_rows(t, ref.t, ref.s_t, ref.k, written, what + " t")
    if nz is not None:
        got = M.unpack_bits(nz[:-2], g.n_rows)
        assert np.array_equal(got, ref.nz), f"{what}: nzbits_out differs at rows {np.flatnonzero(got != ref.nz)[:8]}"
        want = nz0.copy()
        want[:-2] |= M.pack_bits(np.flatnonzero(ref.nz), (len(nz0) - 2) * 32)
        assert np.array_equal(nz, want), f"{what}: a bit outside [0, n_rows) changed"


def dense_bwd1(G, cs):
    """gss_spmm_bwd1 on the scattered [n][d] operands"""
    g, dv = cs.g, bwd1_dev(cs)
    csr = dev_csr(G, g.a, g.kind)
    gam = torch.zeros(g.n_cols, cs.d, device="cuda")
    gax = torch.zeros(g.n_rows, cs.d, device="cuda")
    ids = cu(cs.ids.astype(np.int64))
    gam[ids] = dv["g_am_b"]
    own = ids < g.n_rows
    gax[ids[own]] = dv["g_ax_b"][own]
    u, t = prefilled(g.n_rows, cs.d), prefilled(g.n_rows, cs.d)
    G._lib.check(G.lib.gss_spmm_bwd1(csr.handle, cs.d, ptr(gam), ptr(gax), ptr(dv["x_in"]), ptr(dv["ax"]), ptr(u), ptr(t), G.st()))
    return host(u), host(t)


@pytest.mark.parametrize("kind,d,b", K.BWD1_CASES)
def test_bwd1_sparse_values_write_set_bits_and_the_dense_form(G, kind, d, b):
    """SPMM_BWD1S at every width / batch size / graph: without any option (both entry points), with nzbits_out alone (every row still
    written), with a live-row filter alone (a filtered row is written as zeros), and as a single-shard plan runs it (posbits, nzbits_out,
    skip_zero_rows, live_rows; listed workgroups).  Then against gss_spmm_bwd1 on the scattered operands: t = dm (.) ax is one rounding
    of the same sum, so == holds wherever the sums are ordered alike -- every row, except rows the dense product chunks under
    spmm_giant = 64 (rounding level by spmm.hip's own account: those rows get the bound only).  u likewise, except on member rows with
    a non-zero sum: there the dense epilogue's g_ax + dm (.) x_in is one contracted multiply-add while the sparse epilogue rounds the
    product first (it passes a select before g_ax is added) -- one rounding apart, no promise of equal bits; those rows get the bound."""
    insides = (True, False) if (kind == "giant" and b > 1) else (True,)
    for inside in insides:
        cs = K.bwd1_case(kind, d, b, inside)
        g = cs.g
        assert (cs.pos[g.hubs[0]] >= 0) == inside or b == 1
        ref, ref_live = bwd1_ref(kind, d, b, inside, False), bwd1_ref(kind, d, b, inside, True)
        with knobs(G, spmm_giant=64 if kind == "giant" else 32768):
            base = run_bwd1s(G, cs)
            check_bwd1s(base, ref, False, g, "plain")
            old = run_bwd1s(G, cs, entry="11-argument")
            assert np.array_equal(old[0], base[0]) and np.array_equal(old[1], base[1])
            check_bwd1s(run_bwd1s(G, cs, nzbits=True), ref, False, g, "nzbits_out")
            check_bwd1s(run_bwd1s(G, cs, live=True), ref_live, False, g, "live_rows")
            with knobs(G, spmm_list_blocks=1):
                full = run_bwd1s(G, cs, posbits=True, nzbits=True, skip=True, live=True)
            check_bwd1s(full, ref_live, True, g, "as a plan runs it")
            w = ref.nz
            assert np.array_equal(full[0][w], base[0][w]) and np.array_equal(full[1][w], base[1][w]), "a filter changed a sum"
            du_chunked, dt_chunked = dense_bwd1(G, cs)
        du, dt = dense_bwd1(G, cs)
        chunked = g.lens > 64 if kind == "giant" else np.zeros(g.n_rows, bool)
        everything = np.ones(g.n_rows, bool)
        for (xu, xt), rows in (((du, dt), everything), ((du_chunked, dt_chunked), ~chunked)):
            assert np.array_equal(xt[rows], base[1][rows]), f"t differs from the dense form at rows {np.flatnonzero((xt != base[1]).any(1) & rows)[:8]}"
            rows = rows & ~((cs.pos_row >= 0) & (ref.s_t != 0).any(1))
            assert np.array_equal(xu[rows], base[0][rows]), f"u differs from the dense form at rows {np.flatnonzero((xu != base[0]).any(1) & rows)[:8]}"
        assert_rows(du, ref.u, ref.s_u, ref.k, everything, "dense u")
        assert_rows(du_chunked, ref.u, ref.s_u, ref.k, everything, "dense, chunked u")
        assert_rows(dt_chunked, ref.t, ref.s_t, ref.k, everything, "dense, chunked t")


@pytest.mark.parametrize("kind,b", [("hub", 300), ("rect", 17)])
def test_bwd1_sparse_full_option_grid_at_d128(G, kind, b):
    """posbits x nzbits_out x skip_zero_rows x live_rows x listing at d = 128: every combination the launcher accepts meets the contract
    (values, write set, bitmap), the one it refuses (skip_zero_rows without nzbits_out) is refused by name, and since every option is a
    pure filter all of them give the sums of the option-free launch"""
    cs = K.bwd1_case(kind, 128, b)
    g = cs.g
    ref, ref_live = bwd1_ref(kind, 128, b, True, False), bwd1_ref(kind, 128, b, True, True)
    base = run_bwd1s(G, cs)
    for listing, posbits, nzbits, skip, live in itertools.product((0, 1), (False, True), (False, True), (False, True), (False, True)):
        what = f"listing={listing} posbits={posbits} nzbits_out={nzbits} skip_zero_rows={skip} live_rows={live}"
        with knobs(G, spmm_list_blocks=listing):
            if skip and not nzbits:
                with pytest.raises(G._lib.GssError, match="spmm_bwd1_sparse"):
                    run_bwd1s(G, cs, posbits=posbits, nzbits=nzbits, skip=skip, live=live)
                continue
            out = run_bwd1s(G, cs, posbits=posbits, nzbits=nzbits, skip=skip, live=live)
        check_bwd1s(out, ref_live if live else ref, skip, g, what)
        w = ref.nz if skip else np.ones(g.n_rows, bool)
        assert np.array_equal(out[0][w], base[0][w]) and np.array_equal(out[1][w], base[1][w]), what + ": not the option-free sums"


# ================================================================ SPMM_BWD2S
def bwd2_dev(cs):
    """pos_row_limit > 0: t and pos_row ARE `limit` rows long; they sit at the front of buffers of n_rows rows whose tail holds large
    values / a valid compact row, so that a kernel that read them behind the limit would stay inside an allocation and show a wrong value"""
    if not hasattr(cs, "dev"):
        cs.dev = {k: cu(getattr(cs, k)) for k in ("u", "p", "res_b")}
        rng = np.random.RandomState(cs.limit)
        tail = cs.g.n_rows - cs.t.shape[0]
        cs.dev["t"] = cu(np.concatenate([cs.t, 100 + 100 * rng.rand(tail, cs.d).astype(np.float32)]))
        cs.dev["pos_row"] = cu(np.concatenate([cs.pos_row, rng.randint(0, cs.b, tail).astype(np.int32)]))
        cs.dev["nzbits"] = cu(M.pack_bits(np.flatnonzero(cs.inside), cs.g.n_cols))
    return cs.dev


def run_bwd2s(G, cs, csr, nzbits=False, want_gx=True, y_in=None):
    """y_in: the first pass's sums, in the buffer this pass writes dp to (as a shard's overlapped hop does)"""
    g, dv = cs.g, bwd2_dev(cs)
    dp = y_in if y_in is not None else prefilled(g.n_rows, cs.d)
    gx = prefilled(g.n_rows, cs.d) if want_gx else None
    G._lib.check(G.lib.gss_spmm_bwd2_sparse_res(csr.handle, cs.d, ptr(dv["u"]), ptr(dv["t"]), ptr(dv["p"]), cs.c, ptr(dv["res_b"]), ptr(dv["pos_row"]),
                                                ptr(dp), ptr(gx), ptr(dv["nzbits"]) if nzbits else None, ptr(y_in), cs.limit, G.st()))
    return host(dp), (host(gx) if want_gx else None)


@functools.lru_cache(maxsize=None)
def bwd2_ref(kind, d, b, limit, nzbits):
    cs = K.bwd2_case(kind, d, b, limit)
    bits = M.pack_bits(np.flatnonzero(cs.inside), cs.g.n_cols) if nzbits else None
    return M.bwd2_sparse_res(cs.g.a, cs.u, cs.t, cs.p, cs.c, cs.res_b, cs.pos_row, nzbits=bits, pos_row_limit=limit)


def check_bwd2s(out, ref, g, what):
    every = np.ones(g.n_rows, bool)
    assert_rows(out[0], ref.dp, ref.s_dp, ref.k, every, what + " dp")
    if out[1] is not None:
        assert_rows(out[1], ref.gx, ref.s_gx, ref.k, every, what + " gx")


@pytest.mark.parametrize("kind,d,b", K.BWD2_CASES)
def test_bwd2_sparse_res_values_filter_and_the_dense_form(G, kind, d, b):
    """SPMM_BWD2S with the residual held compactly: without and with the non-zero-row bitmap (given as exactly the non-zero rows of u: a
    pure filter, == on every element), with and without gx_out; then == gss_spmm_bwd2 with the scattered residual (rows the dense
    product chunks under spmm_giant = 64: the bound only)"""
    cs = K.bwd2_case(kind, d, b)
    g, dv = cs.g, bwd2_dev(cs)
    csr = dev_csr(G, g.a, g.kind)
    res = torch.zeros(g.n_rows, d, device="cuda")
    ids = cu(cs.ids.astype(np.int64))
    own = ids < g.n_rows
    res[ids[own]] = dv["res_b"][own]

    def dense():
        dp, gx = prefilled(g.n_rows, d), prefilled(g.n_rows, d)
        G._lib.check(G.lib.gss_spmm_bwd2(csr.handle, d, ptr(dv["u"]), ptr(dv["t"]), ptr(dv["p"]), cs.c, ptr(res), ptr(dp), ptr(gx), G.st()))
        return host(dp), host(gx)

    with knobs(G, spmm_giant=64 if kind == "giant" else 32768):
        base = run_bwd2s(G, cs, csr)
        check_bwd2s(base, bwd2_ref(kind, d, b, 0, False), g, "plain")
        filt = run_bwd2s(G, cs, csr, nzbits=True)
        check_bwd2s(filt, bwd2_ref(kind, d, b, 0, True), g, "nzbits")
        assert np.array_equal(filt[0], base[0]) and np.array_equal(filt[1], base[1]), "the non-zero-row filter changed a sum"
        nogx = run_bwd2s(G, cs, csr, nzbits=True, want_gx=False)
        assert np.array_equal(nogx[0], base[0])
        chunked_out = dense()
    whole = dense()
    chunked = g.lens > 64 if kind == "giant" else np.zeros(g.n_rows, bool)
    for got, rows in ((whole, np.ones(g.n_rows, bool)), (chunked_out, ~chunked)):
        for k in (0, 1):
            assert np.array_equal(got[k][rows], base[k][rows]), f"{'dp gx'.split()[k]} differs from the dense form at rows {np.flatnonzero((got[k] != base[k]).any(1) & rows)[:8]}"
    check_bwd2s(chunked_out, bwd2_ref(kind, d, b, 0, False), g, "dense, chunked")


@pytest.mark.parametrize("kind,d,b", [("hub", 128, 17), ("rect", 48, 17), ("hub", 512, 300), ("giant", 16, 17)])
@pytest.mark.parametrize("nzbits", [False, True])
def test_bwd2_sparse_res_second_pass_of_a_two_pass_product(G, kind, d, b, nzbits):
    """The entries split by column at c0 (a shard's own-column / boundary-column halves): a plain product of the first half (under the
    same bitmap as a gather filter), then SPMM_BWD2S over the second half with the first pass's sums as y_in, in place.  Within the bound
    of the one-pass mirror everywhere; the same bits as the one-pass kernel on rows whose entries all lie in one half"""
    cs = K.bwd2_case(kind, d, b)
    g, dv = cs.g, bwd2_dev(cs)
    c0 = g.n_cols // 3
    first, second = K.split_by_column(g.a, c0)
    one = run_bwd2s(G, cs, dev_csr(G, g.a, g.kind), nzbits=nzbits)
    y = prefilled(g.n_rows, d)
    G._lib.check(G.lib.gss_spmm_filtered(dev_csr(G, first, (kind, "first")).handle, d, ptr(dv["u"]), ptr(y), None, None, None, None, None,
                                         ptr(dv["nzbits"]) if nzbits else None, G.st()))
    two = run_bwd2s(G, cs, dev_csr(G, second, (kind, "second")), nzbits=nzbits, y_in=y)
    check_bwd2s(two, bwd2_ref(kind, d, b, 0, nzbits), g, "two passes")
    one_sided = (np.diff(first.indptr) == 0) | (np.diff(second.indptr) == 0)
    assert one_sided.sum() > 50
    assert np.array_equal(two[0][one_sided], one[0][one_sided]) and np.array_equal(two[1][one_sided], one[1][one_sided])


@pytest.mark.parametrize("kind,d,b,limit", K.LIMIT_CASES)
def test_bwd2_sparse_res_rows_behind_pos_row_limit_have_neither_t_nor_a_residual(G, kind, d, b, limit):
    """pos_row_limit on the rectangular operand: t and pos_row have exactly `limit` rows and what lies behind them in memory is not
    zero (bwd2_dev), so a kernel that read them for a row behind the limit would show a wrong value: those rows get
    dp = c (A u) (.) elu'(p)"""
    cs = K.bwd2_case(kind, d, b, limit)
    g = cs.g
    assert 0 < limit < g.n_rows and cs.t.shape[0] == limit and cs.pos_row.shape[0] == limit
    csr = dev_csr(G, g.a, g.kind)
    for nzbits in (False, True):
        out = run_bwd2s(G, cs, csr, nzbits=nzbits)
        check_bwd2s(out, bwd2_ref(kind, d, b, limit, nzbits), g, f"limit, nzbits={nzbits}")
    # stated once more without the mirror's help, for the rows behind the limit
    au = (g.a.astype(np.float64) @ cs.u.astype(np.float64))[limit:]
    want = cs.c * au * np.where(cs.p[limit:] > 0, 1.0, np.exp(np.minimum(cs.p[limit:], 0).astype(np.float64)))
    ref = bwd2_ref(kind, d, b, limit, False)
    assert np.all(np.abs(out[0][limit:] - want) <= M.bound(ref.k, ref.s_dp)[limit:] + 1e-13 * ref.s_dp[limit:])


# ================================================================ filtered forward products
@pytest.mark.parametrize("kind,d,b", K.FWD_CASES)
def test_filtered_forward_products(G, kind, d, b):
    """SPMM_PLAIN under a row map / a row bitmap / both / a gather filter, SPMM_FWD1 under a row bitmap, and the second pass (y_in) of
    both: the bound on the rows the filter lets through, the pre-fill on every other row, the same bits with the live workgroups listed
    (spmm_list_blocks = 1) and dispatched whole (0), and the same bits as the unfiltered product on the rows computed.  On the giant
    graph (spmm_giant = 64) the row that holds every column is computed chunk by chunk -- once inside the filter, once outside"""
    cs = K.fwd_case(kind, d, b)
    g = cs.g
    csr = dev_csr(G, g.a, g.kind)
    x, xz, h = cu(cs.x), cu(cs.xz), cu(cs.h)
    gather = M.pack_bits(np.flatnonzero(cs.inside), g.n_cols)
    variants = [cs.rows]
    if kind == "giant" and b > 1:
        assert 40 in cs.rows
        variants.append(cs.rows[cs.rows != 40])
    with knobs(G, spmm_giant=64 if kind == "giant" else 32768):
        full_y, full_m = prefilled(g.n_rows, d), prefilled(g.n_rows, d)
        G._lib.check(G.lib.gss_spmm(csr.handle, d, ptr(x), ptr(full_y), ptr(h), ptr(full_m), G.st()))
        full_y, full_m = host(full_y), host(full_m)
        for rows in variants:
            row_pos = np.full(g.n_rows, -1, np.int32)
            row_pos[rows] = np.arange(len(rows), dtype=np.int32)
            rlist = np.concatenate([rows, [-1, -1]]).astype(np.int32)
            bits0 = np.zeros(M.words_for(g.n_cols) + 2, np.uint32)
            bits0[-2:] = GUARD
            bits, d_rlist = cu(bits0), cu(rlist)
            G._lib.check(G.lib.gss_mark_rows_and_neighbours(csr.handle, ptr(d_rlist), len(rlist), ptr(bits), G.st()))
            bits_h = host(bits)
            want_bits = bits0.copy()
            want_bits[:-2] = M.mark_rows_and_neighbours(g.a, rlist, bits0[:-2])
            assert np.array_equal(bits_h, want_bits), "mark_rows_and_neighbours: not exactly the rows and their columns"
            rp = cu(row_pos)
            y_prev = cu(np.random.RandomState(d + b).randn(g.n_rows, d).astype(np.float32))
            configs = [("row_pos", dict(row_pos=row_pos), rp, None, None, None, False),
                       ("row_bits", dict(row_bits=bits_h[:-2]), None, bits, None, None, False),
                       ("row_pos + row_bits", dict(row_pos=row_pos, row_bits=bits_h[:-2]), rp, bits, None, None, False),
                       ("fwd1 row_bits", dict(row_bits=bits_h[:-2]), None, bits, None, None, True),
                       ("row_pos + y_in", dict(row_pos=row_pos, y_in=host(y_prev)), rp, None, y_prev, None, False),
                       ("fwd1 row_bits + y_in", dict(row_bits=bits_h[:-2], y_in=host(y_prev)), None, bits, y_prev, None, True)]
            for what, kw, d_pos, d_bits, d_yin, _, fused in configs:
                ref = M.spmm_filtered(g.a, cs.x, h=cs.h if fused else None, **kw)
                outs = []
                for listing in (0, 1):
                    y, m = prefilled(g.n_rows, d), prefilled(g.n_rows, d)
                    with knobs(G, spmm_list_blocks=listing):
                        G._lib.check(G.lib.gss_spmm_filtered(csr.handle, d, ptr(x), ptr(y), ptr(h) if fused else None, ptr(m) if fused else None,
                                                             ptr(d_pos), ptr(d_bits), ptr(d_yin), None, G.st()))
                    y, m = host(y), host(m)
                    assert_rows(y, ref.y, ref.s_y, ref.k, ref.written, f"{what} listing={listing} y")
                    if fused:
                        assert_rows(m, ref.m, ref.s_m, ref.k, ref.written, f"{what} listing={listing} m")
                    else:
                        assert untouched(m).all()
                    outs.append((y, m))
                w = ref.written
                assert np.array_equal(outs[0][0][w], outs[1][0][w]) and np.array_equal(outs[0][1].view(np.int32), outs[1][1].view(np.int32)), what
                if d_yin is None:   # a computed row is summed exactly as in the unfiltered launch
                    assert np.array_equal(outs[0][0][w], full_y[w]), what
                    if fused:
                        assert np.array_equal(outs[0][1][w], full_m[w]), what
    # the gather filter (the first pass of a two-pass SPMM_BWD2S): columns outside the set are skipped; over an operand that is zero
    # there it is a pure filter.  The filtered walk keeps the single schedule, so compare with the unchunked product
    ref = M.spmm_filtered(g.a, cs.xz, gather_bits=gather)
    y, y0, d_gather = prefilled(g.n_rows, d), prefilled(g.n_rows, d), cu(gather)
    G._lib.check(G.lib.gss_spmm_filtered(csr.handle, d, ptr(xz), ptr(y), None, None, None, None, None, ptr(d_gather), G.st()))
    G._lib.check(G.lib.gss_spmm(csr.handle, d, ptr(xz), ptr(y0), None, None, G.st()))
    y, y0 = host(y), host(y0)
    assert_rows(y, ref.y, ref.s_y, ref.k, ref.written, "gather_bits")
    assert ref.written.all() and np.array_equal(y, y0), "the gather filter changed a sum"


@pytest.mark.parametrize("d,slices,pin", [(48, 2, 1), (128, 2, 0), (128, 4, 1), (512, 4, 1), (512, 8, 0)])
def test_feature_sliced_launches_meet_the_same_contract(G, d, slices, pin):
    """The balanced kernel cut into feature slices (knob spmm_slices; time-separated or pinned to XCDs -- what the automatic policy
    picks for operands beyond the L2s): the compact operands, y_in and the outputs are then addressed by slice.  SPMM_BWD2S (bitmap,
    pos_row_limit) and the row-filtered forward products, the listed dispatch included (a list item is a (workgroup, slice) pair when
    the slices are pinned), meet the same bound and write set"""
    with knobs(G, spmm_slices=slices, spmm_pin=pin):
        for kind, limit in (("hub", 0), ("rect", 600)):
            cs = K.bwd2_case(kind, d, 17, limit)
            csr = dev_csr(G, cs.g.a, kind)
            for nzbits in (False, True):
                check_bwd2s(run_bwd2s(G, cs, csr, nzbits=nzbits), bwd2_ref(kind, d, 17, limit, nzbits), cs.g, f"{kind} nzbits={nzbits}")
        cs = K.fwd_case("hub", d, 17)
        g = cs.g
        csr = dev_csr(G, g.a, g.kind)
        x, h, rp = cu(cs.x), cu(cs.h), cu(cs.row_pos)
        bits_h = M.mark_rows_and_neighbours(g.a, cs.rows, np.zeros(M.words_for(g.n_cols), np.uint32))
        bits = cu(bits_h)
        y_prev = cu(np.random.RandomState(d).randn(g.n_rows, d).astype(np.float32))
        for what, kw, d_pos, d_bits, d_yin, fused in (("row_pos", dict(row_pos=cs.row_pos), rp, None, None, False),
                                                      ("fwd1 row_bits + y_in", dict(row_bits=bits_h, y_in=host(y_prev)), None, bits, y_prev, True)):
            ref = M.spmm_filtered(g.a, cs.x, h=cs.h if fused else None, **kw)
            outs = []
            for listing in (0, 1):
                y, m = prefilled(g.n_rows, d), prefilled(g.n_rows, d)
                with knobs(G, spmm_list_blocks=listing):
                    G._lib.check(G.lib.gss_spmm_filtered(csr.handle, d, ptr(x), ptr(y), ptr(h) if fused else None, ptr(m) if fused else None,
                                                         ptr(d_pos), ptr(d_bits), ptr(d_yin), None, G.st()))
                y, m = host(y), host(m)
                assert_rows(y, ref.y, ref.s_y, ref.k, ref.written, f"{what} listing={listing} y")
                if fused:
                    assert_rows(m, ref.m, ref.s_m, ref.k, ref.written, f"{what} listing={listing} m")
                outs.append((y, m))
            assert np.array_equal(outs[0][0].view(np.int32), outs[1][0].view(np.int32)) and np.array_equal(outs[0][1].view(np.int32), outs[1][1].view(np.int32))


# ================================================================ bitmap builders
def test_batch_bits_set_then_clear_and_bits_fill(G):
    rng = np.random.RandomState(11)
    n = 3000
    for b in K.BATCHES:
        ids = np.unique(np.concatenate([rng.permutation(n)[:b], [0, 31, 32, 63, 64, n - 1]][:1 if b == 1 else 2])).astype(np.int32)
        ids = np.concatenate([ids, [-1, -5]]).astype(np.int32)[rng.permutation(len(ids) + 2)]
        start = rng.randint(0, 2 ** 32, M.words_for(n) + 2, dtype=np.uint64).astype(np.uint32)
        start[np.unique(ids[ids >= 0] >> 5)] = 0          # the contract: every set bit of a member's word belongs to a member
        start[-2:] = GUARD
        bits, d_ids = cu(start), cu(ids)
        G._lib.check(G.lib.gss_batch_bits(ptr(d_ids), len(ids), ptr(bits), 1, G.st()))
        assert np.array_equal(host(bits), M.batch_bits(ids, start, 1))
        assert M.unpack_bits(host(bits), n).sum() == M.unpack_bits(start, n).sum() + (ids >= 0).sum()
        G._lib.check(G.lib.gss_batch_bits(ptr(d_ids), len(ids), ptr(bits), 0, G.st()))
        assert np.array_equal(host(bits), start), "set then clear does not return the bitmap to its start"
    start = rng.randint(0, 2 ** 32, 40, dtype=np.uint64).astype(np.uint32)
    for first, last in ((5, 6), (5, 37), (31, 33), (32, 64), (33, 63), (70, 999), (0, 1000), (1, 1279), (640, 640), (700, 650)):
        bits = cu(start)
        G._lib.check(G.lib.gss_bits_fill(ptr(bits), first, last, G.st()))
        assert np.array_equal(host(bits), M.bits_fill(start, first, last)), (first, last)


# ================================================================ refusals
def test_refusals_name_the_function_and_launch_nothing(G):
    cs = K.bwd1_case("hub", 128, 17)
    g, dv = cs.g, bwd1_dev(cs)
    csr = dev_csr(G, g.a, g.kind)
    u, t = prefilled(g.n_rows, 128), prefilled(g.n_rows, 128)
    nz = cu(bitmap_words(g.n_cols, g.n_rows))
    good = [csr.handle, 128, ptr(dv["g_am_b"]), ptr(dv["g_ax_b"]), ptr(dv["pos"]), ptr(dv["pos_row"]), ptr(dv["x_in"]), ptr(dv["ax"]), ptr(u), ptr(t),
            None, ptr(nz), 0, None, G.st()]

    def refused(fn, args, name):
        assert fn(*args) != 0
        assert name in G.lib.gss_last_error().decode(), G.lib.gss_last_error()

    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):
        refused(G.lib.gss_spmm_bwd1_sparse_ex, good[:i] + [None] + good[i + 1:], "spmm_bwd1_sparse")
    refused(G.lib.gss_spmm_bwd1_sparse_ex, good[:11] + [None, 1] + good[13:], "spmm_bwd1_sparse")       # skip_zero_rows without nzbits_out
    c2 = K.bwd2_case("hub", 128, 17)
    d2 = bwd2_dev(c2)
    dp = prefilled(g.n_rows, 128)
    good2 = [csr.handle, 128, ptr(d2["u"]), ptr(d2["t"]), ptr(d2["p"]), 0.3, ptr(d2["res_b"]), ptr(d2["pos_row"]), ptr(dp), None, None, None, 0, G.st()]
    for i in (0, 2, 3, 4, 6, 7, 8):
        refused(G.lib.gss_spmm_bwd2_sparse_res, good2[:i] + [None] + good2[i + 1:], "spmm_bwd2_sparse_res")
    x = d2["u"]
    good3 = [csr.handle, 128, ptr(x), ptr(dp), None, None, ptr(dv["pos_row"]), None, None, None, G.st()]
    for i in (0, 2, 3):
        refused(G.lib.gss_spmm_filtered, good3[:i] + [None] + good3[i + 1:], "spmm_filtered")
    refused(G.lib.gss_mark_rows_and_neighbours, [None, ptr(dv["pos"]), 4, ptr(nz), G.st()], "mark_rows_and_neighbours")
    refused(G.lib.gss_mark_rows_and_neighbours, [csr.handle, None, 4, ptr(nz), G.st()], "mark_rows_and_neighbours")
    refused(G.lib.gss_batch_bits, [None, 4, ptr(nz), 1, G.st()], "batch_bits")
    refused(G.lib.gss_batch_bits, [ptr(dv["pos"]), 4, None, 1, G.st()], "batch_bits")
    refused(G.lib.gss_bits_fill, [None, 0, 8, G.st()], "bits_fill")
    with knobs(G, spmm_variant=1):      # the row-per-wave SpMM has none of the sparse modes
        refused(G.lib.gss_spmm_bwd1_sparse_ex, good, "spmm_bwd1_sparse")
        refused(G.lib.gss_spmm_bwd1_sparse, good[:10] + [G.st()], "spmm_bwd1_sparse")
        refused(G.lib.gss_spmm_bwd2_sparse_res, good2, "spmm_bwd2_sparse_res")
        refused(G.lib.gss_spmm_filtered, good3, "spmm")
    torch.cuda.synchronize()
    assert untouched(u.cpu().numpy()).all() and untouched(t.cpu().numpy()).all() and untouched(dp.cpu().numpy()).all()   # nothing was launched
    G._lib.check(G.lib.gss_spmm_bwd1_sparse_ex(*good))          # ... and the same arguments run once the knob is back
    assert fully_written(host(u)).all()


# ================================================================ gss_scatter_add_rows
@pytest.mark.parametrize("b", [1, 333])
@pytest.mark.parametrize("d", [16, 256])
def test_scatter_add_rows_adds_the_listed_rows_and_touches_no_other(G, d, b):
    """dst[rows[r]] += src[r]: np.add.at over distinct rows (the header demands unique rows), negative entries skipped, every row that
    is not listed untouched bit for bit (the destination holds NaNs of a known payload there).  One fp32 addition per element: exact"""
    rng = np.random.RandomState(d + b)
    n = 1000
    rows = rng.permutation(n)[:b].astype(np.int32)
    if b > 1:
        rows[:4] = [0, n - 1, 31, 32]
        rows = np.unique(rows).astype(np.int32)[rng.permutation(len(np.unique(rows)))]
        rows[5::7] = -1
        rows[-1] = -3
    listed = rows[rows >= 0]
    src = rng.randn(len(rows), d).astype(np.float32)
    dst0 = np.full((n, d), PREFILL, np.int32).view(np.float32)
    dst0[listed] = rng.randn(len(listed), d).astype(np.float32)
    dst, d_src, d_rows = cu(dst0), cu(src), cu(rows)
    G._lib.check(G.lib.gss_scatter_add_rows(d, ptr(d_src), ptr(d_rows), len(rows), ptr(dst), G.st()))
    got = host(dst)
    want = dst0.copy()
    np.add.at(want, listed, src[rows >= 0])
    assert np.array_equal(got[listed], want[listed])
    other = np.ones(n, bool)
    other[listed] = False
    assert np.array_equal(got.view(np.int32)[other], dst0.view(np.int32)[other])
