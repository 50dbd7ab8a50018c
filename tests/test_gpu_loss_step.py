"""-m gpu: the loss of a plan's step, op by op, against its fp64 contract (tests/loss_step_mirror.py).  A plan reaches csrc/loss.hip through
loss_step (the sweep, then loss_finish_bwd_kernel or loss_finish_dgrad_kernel), loss_step_slab_sweep (loss_slab_sum_kernel) and the three
gathers; the entry points gss_loss_step, gss_loss_slab_sweep and gss_loss_gather_* call exactly those.

Inputs come from tests/loss_step_cases.py; every test asserts on its reference, before it compares anything, that no pair of the batch
can land on the other side of S = 0 in fp32 (loss_step_mirror.pair_guard, zero pairs excluded).  Bounds (tests/tolerances.py): loss
2e-6 relative and dE 5e-6 of the largest entry, as test_loss_fwd_bwd; the composite outputs 8 x the error of the reference's own
formulas in numpy float32, or the project's 3e-6 where that is larger.  Every output sits between canary elements and starts as a NaN
of a recognisable payload; the workspace is exactly gss_loss_workspace_bytes[_parts] long inside a canary-filled buffer.
No test provokes a fault: every launch that runs gets valid arguments, the refusals are refused before any launch."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from guarded import CANARY, PAD, PREFILL, WS_BYTE, WS_TAIL, Out, Workspace, bits, close, cu, ptr, written  # noqa: F401
import loss_step_cases as K
import loss_step_mirror as M
import tolerances as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POS_FREE = -7                        # a batch-position map entry nobody wrote


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import gcn_drug_repurposing_amd as pkg
    from gcn_drug_repurposing_amd import _lib

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib = pkg.load(), _lib
    ns.st = lambda: _lib.current_stream()
    ns.dev = {}
    return ns


@contextlib.contextmanager
def loss_wgs(G, value):
    """the knob that sets the j split of the sweep and the workspace layout; back to its default whatever happens"""
    try:
        G._lib.check(G.lib.gss_debug_set_option(b"loss_wgs", value))
        yield
    finally:
        G._lib.check(G.lib.gss_debug_set_option(b"loss_wgs", 256))


def close_loss(got, ref, what):
    err = abs(got - ref) / abs(ref)
    print(f"{what}: err {err:.3e} (bound {T.LOSS_STEP_LOSS_RTOL:.1e})")
    assert err <= T.LOSS_STEP_LOSS_RTOL, f"{what}: {got!r} against {ref!r}"


def guarded_case(regime, d, b):
    """the inputs, after the check that no pair of the batch sits where fp32 and fp64 could disagree about the sign of S"""
    c = K.case(regime, d, b)
    assert M.pair_guard(c["e_b"]) == 0
    return c


def device(G, c):
    key = (c["regime"], c["d"], c["b"])
    if key not in G.dev:
        G.dev[key] = {k: cu(c[k]) for k in ("e", "e_b", "p", "inv_den", "p_b", "inv_b", "rows", "keep", "w1t", "w2t")}
    return G.dev[key]


def run_step(G, c, D, form, keep=False, weights=False, dgrad_all=0, pos_ids="same", de_x=None, e_b="given", rows=None, want_rc=False):
    """one gss_loss_step call with guarded outputs.  form "ids": rows = the batch's ids, p / inv_den of all n rows; "member": rows NULL,
    p / inv_den per member.  pos_ids: "same" (the ids), None (NULL: the keys are `rows`), or an int32 array.
    -> dict of host arrays (loss, dx, dp, gax, gam, pos), done"""
    d, b, n = c["d"], c["b"], c["n"]
    o = dict(loss=Out(1), dx=Out(b, d), dp=Out(b, d), gax=Out(b, d), gam=Out(b, d), pos=Out(n + 5, fill=POS_FREE, dtype=torch.int32))
    ws = Workspace(G.lib.gss_loss_workspace_bytes(b, d))
    rows_d = (D["rows"] if rows is None else rows) if form == "ids" else None
    keys = D["rows"] if isinstance(pos_ids, str) else (None if pos_ids is None else cu(pos_ids))
    use_pos = keys is not None or rows_d is not None
    done = C.c_int32(-1)
    rc = G.lib.gss_loss_step(d, b, c["beta"], c["alpha"], o["loss"].ptr, ptr(D["e_b"]) if isinstance(e_b, str) else ptr(e_b), ptr(rows_d), ptr(keys),
                             o["pos"].ptr if use_pos else None, ptr(D["keep"]) if keep else None,
                             ptr(D["inv_den"] if form == "ids" else D["inv_b"]), ptr(D["p"] if form == "ids" else D["p_b"]), c["c"],
                             o["dx"].ptr, o["dp"].ptr, ptr(D["w1t"]) if weights else None, ptr(D["w2t"]) if weights else None,
                             o["gax"].ptr if weights else None, o["gam"].ptr if weights else None, dgrad_all, ptr(de_x), ws.ptr, G.st(),
                             C.byref(done))
    if want_rc:
        return rc, o, ws
    G._lib.check(rc, "gss_loss_step")
    out = {k: v.host(k) for k, v in o.items()}
    ws.check()
    out["done"] = done.value
    return out


def check_pos(got, keys, n):
    want = np.full(n + 5, POS_FREE, np.int32)
    r = np.arange(len(keys), dtype=np.int32)
    want[keys[keys >= 0]] = r[keys >= 0]
    assert np.array_equal(got, want), "the batch-position map: pos_set[key[r]] == r for keys >= 0, nothing else written"


def check_finish(got, ref, what):
    for k in ("dx", "dp"):
        close(written(got[k], f"{what} {k}"), ref[k], T.LOSS_STEP_BOUND[k], ref["scale"][k], f"{what} {k}")


# ================================================================ the sweep and the finish without weights
@pytest.mark.parametrize("regime,d,b,wgs", K.STEP_CASES)
def test_step_matches_the_mirror(G, regime, d, b, wgs):
    c = guarded_case(regime, d, b)
    D = device(G, c)
    n = c["n"]
    ref_ids, ref_mem = K.reference(regime, d, b, "ids"), K.reference(regime, d, b, "member")
    with loss_wgs(G, wgs):
        # (1) rows and pos_ids equal to the permutation's ids, keep NULL
        a = run_step(G, c, D, "ids")
        assert a["done"] == 0 and (bits(a["gax"]) == np.int32(PREFILL)).all() and (bits(a["gam"]) == np.int32(PREFILL)).all()
        close_loss(float(a["loss"][0]), ref_ids["loss"], "loss")
        check_finish(a, ref_ids, "rows = ids")
        check_pos(a["pos"], c["rows"], n)
        # (2) pos_ids NULL: the keys are the rows
        a2 = run_step(G, c, D, "ids", pos_ids=None)
        check_pos(a2["pos"], c["rows"], n)
        assert all(np.array_equal(bits(a2[k]), bits(a[k])) for k in ("loss", "dx", "dp"))
        # (3) rows NULL: p / inv_den per member, keep NULL -- the same operands, the same bits; no keys: no map
        m = run_step(G, c, D, "member", pos_ids=None)
        assert all(np.array_equal(bits(m[k]), bits(a[k])) for k in ("loss", "dx", "dp")) and (m["pos"] == POS_FREE).all()
        # (4) rows NULL with keep (a third zeros: the first and last member and one whole tile among them), keys of -1 skipped
        keys = c["rows"].copy()
        keys[::4] = -1
        k = run_step(G, c, D, "member", keep=True, pos_ids=keys)
        check_finish(k, ref_mem, "keep")
        kept = c["keep"] != 0
        assert not k["dx"][~kept].any() and not k["dp"][~kept].any(), "rows with keep == 0 are zeros"
        assert np.array_equal(bits(k["dx"])[kept], bits(a["dx"])[kept]) and np.array_equal(bits(k["dp"])[kept], bits(a["dp"])[kept])
        assert np.array_equal(bits(k["loss"]), bits(a["loss"]))
        check_pos(k["pos"], keys, n)
        # the loss is gss_loss_fwd_bwd's bit for bit (same partials, same order); dE is observable there at the same loss_wgs
        loss, de = Out(1), Out(b, d)
        ws = Workspace(G.lib.gss_loss_workspace_bytes(b, d))
        G._lib.check(G.lib.gss_loss_fwd_bwd(n, d, ptr(D["e"]), ptr(D["rows"]), b, c["beta"], c["alpha"], loss.ptr, de.ptr, ws.ptr, G.st()))
        assert np.array_equal(bits(loss.host()), bits(a["loss"]))
        close(written(de.host("dE"), "dE"), ref_ids["de"], T.LOSS_STEP_DE_REL, np.abs(ref_ids["de"]).max(), "dE")
        ws.check()


@pytest.mark.parametrize("regime,d,b,wgs", K.REPEAT_CASES)
def test_repeated_ids_loss_and_de(G, regime, d, b, wgs):
    """a batch with repeated ids (pos_set NULL: the map has one position per node), gathered by gss_loss_gather_rows into the workspace
    and swept from there (e_b NULL)"""
    c, rows = K.repeated(regime, d, b)
    e_b = c["e"][rows]
    assert M.pair_guard(e_b) == 0
    D = device(G, c)
    rows_d = cu(rows)
    ref_loss, ref_de = M.sweep(e_b, c["beta"], c["alpha"])
    with loss_wgs(G, wgs):
        o = dict(loss=Out(1), dx=Out(b, d), dp=Out(b, d))
        ws = Workspace(G.lib.gss_loss_workspace_bytes(b, d))
        where = C.c_void_p()
        G._lib.check(G.lib.gss_loss_gather_rows(d, ptr(D["e"]), ptr(rows_d), None, b, ws.ptr, C.byref(where), G.st()))
        assert np.array_equal(bits(ws.floats_at(where.value, b * d).reshape(b, d)), bits(e_b))
        done = C.c_int32(-1)
        G._lib.check(G.lib.gss_loss_step(d, b, c["beta"], c["alpha"], o["loss"].ptr, None, ptr(rows_d), None, None, None, ptr(D["inv_den"]),
                                         ptr(D["p"]), c["c"], o["dx"].ptr, o["dp"].ptr, None, None, None, None, 0, None, ws.ptr, G.st(),
                                         C.byref(done)))
        close_loss(float(o["loss"].host()[0]), ref_loss, "loss")
        written(o["dx"].host(), "dx"), written(o["dp"].host(), "dp")
        ws.check()
        loss, de = Out(1), Out(b, d)
        G._lib.check(G.lib.gss_loss_fwd_bwd(c["n"], d, ptr(D["e"]), ptr(rows_d), b, c["beta"], c["alpha"], loss.ptr, de.ptr, ws.ptr, G.st()))
        assert np.array_equal(bits(loss.host()), bits(o["loss"].host()))
        close(written(de.host(), "dE"), ref_de, T.LOSS_STEP_DE_REL, np.abs(ref_de).max(), "dE")
        ws.check()


# ================================================================ the finish with the input gradient
@pytest.mark.parametrize("regime,d,b,wgs", K.WEIGHT_CASES)
def test_step_with_weights(G, regime, d, b, wgs):
    c = guarded_case(regime, d, b)
    D = device(G, c)
    kept = c["keep"] != 0
    with loss_wgs(G, wgs):
        free = run_step(G, c, D, "member")                     # keep NULL: the unmasked dP rows
        for form, keep in (("ids", False), ("member", True)):
            base = run_step(G, c, D, form, keep=keep)
            assert base["done"] == 0
            for every in (0, 1):
                what = f"{form} keep={keep} dgrad_all={every}"
                w = run_step(G, c, D, form, keep=keep, weights=True, dgrad_all=every)
                assert w["done"] == 1
                # "the same lanes in the same order": the finish is loss_finish_bwd_kernel's, bit for bit
                for k in ("loss", "dx", "dp", "pos"):
                    assert np.array_equal(bits(w[k]), bits(base[k])), f"{what}: {k} differs from the launch without weights"
                ref = K.reference(regime, d, b, form, True, bool(every and keep))
                for k in ("gax", "gam"):
                    close(written(w[k], f"{what} {k}"), ref[k], T.LOSS_STEP_BOUND[k], ref["scale"][k], f"{what} {k}")
                if keep and not every:
                    assert not w["gax"][~kept].any() and not w["gam"][~kept].any()
                # ... and the product is the stand-alone launch's, bit for bit, on the dP this launch multiplied
                dp = w["dp"].copy()
                if keep and every:
                    dp[~kept] = free["dp"][~kept]
                gax, gam = Out(b, d), Out(b, d)
                G._lib.check(G.lib.gss_dense_bwd_input(b, d, ptr(cu(dp)), ptr(D["w1t"]), ptr(D["w2t"]), None, gax.ptr, gam.ptr, G.st()))
                assert np.array_equal(bits(gax.host()), bits(w["gax"])), f"{what}: gax_b is not gss_dense_bwd_input's"
                assert np.array_equal(bits(gam.host()), bits(w["gam"])), f"{what}: gam_b is not gss_dense_bwd_input's"


@pytest.mark.parametrize("d", K.REFUSED_WIDTHS)
def test_weights_at_other_widths_are_refused_by_name(G, d):
    c = K.case("recipe", d, 17)
    D = device(G, c)
    for form, keep in (("ids", False), ("member", True)):
        rc, o, ws = run_step(G, c, D, form, keep=keep, weights=True, dgrad_all=1, want_rc=True)
        assert rc != 0
        msg = G.lib.gss_last_error().decode()
        assert "loss_step" in msg and f"d={d}" in msg, msg
        torch.cuda.synchronize()
        for k in ("loss", "dx", "dp", "gax", "gam"):
            assert o[k].untouched(k), f"a refused call wrote {k}"
        assert (o["pos"].host() == POS_FREE).all()
        assert (ws.buf == WS_BYTE).all().item(), "a refused call wrote the workspace"


# ================================================================ the row-slab form
@pytest.mark.parametrize("regime,d,b,parts", K.SLAB_CASES)
def test_slab_form(G, regime, d, b, parts):
    c = guarded_case(regime, d, b)
    D = device(G, c)
    refs = [M.slab_rank(c["e_b"], c["beta"], c["alpha"], r, parts) for r in range(parts)]
    scale = max(np.abs(x[:-1]).max() for x in refs)
    nbytes = G.lib.gss_loss_workspace_bytes_parts(b, d, parts)
    assert nbytes > 0
    bufs, shares = [], []
    for r in range(parts):
        ws, de_x = Workspace(nbytes), Out(b * d + 1)
        G._lib.check(G.lib.gss_loss_slab_sweep(d, b, c["beta"], c["alpha"], ptr(D["e_b"]), r, parts, ws.ptr, de_x.ptr, G.st()), "gss_loss_slab_sweep")
        x = written(de_x.host(f"de_x of rank {r}"), f"de_x of rank {r}")
        ws.check(f"workspace of rank {r}")
        mine = M.slab_tiles(b, r, parts)
        rows = x[:-1].reshape(b, d)
        assert not rows[~mine].any(), f"rank {r}: rows outside its tiles are exactly zero"
        if not mine.any():
            assert not x.any(), f"rank {r} has no tile: all zeros and a zero loss share"
        else:
            close(rows[mine], refs[r][:-1].reshape(b, d)[mine], T.LOSS_STEP_BOUND["slab"], scale, f"rank {r} rows")
        shares.append(float(x[-1]))
        bufs.append(de_x.t)
    ref_mem = K.reference(regime, d, b, "member")
    close_loss(sum(shares), ref_mem["loss"], "sum of the loss shares")
    # what the all-reduce leaves: the ranks' buffers summed in rank order, in fp32; the finish from that sum
    acc = bufs[0].clone()
    for t in bufs[1:]:
        acc += t
    weights = d in (64, 128, 256)
    got = run_step(G, c, D, "member", keep=True, weights=weights, dgrad_all=1, de_x=acc)
    ref = K.reference(regime, d, b, "member", weights, True)
    check_finish(got, ref, "after the sum")
    assert got["done"] == int(weights) and (bits(got["loss"]) == np.int32(PREFILL)).all()       # (the loss came with de_x)
    if weights:
        for k in ("gax", "gam"):
            close(written(got[k], k), ref[k], T.LOSS_STEP_BOUND[k], ref["scale"][k], f"after the sum {k}")


# ================================================================ the gathers (bit for bit)
def gather_inputs(b, d):
    rng = np.random.RandomState(1000 * b + d)
    n = b + 9                                     # rows of this shard; the id range is [0, 3 n), the shard owns [n, 2 n)
    e, p = rng.randn(n, d).astype(np.float32), rng.randn(n, d).astype(np.float32)
    inv = rng.uniform(0.5, 2.0, n).astype(np.float32)
    node_map = rng.permutation(3 * n).astype(np.int32)
    gid2op = (rng.permutation(3 * n) * 3 + 1).astype(np.int32)
    idx = rng.permutation(3 * n)[:b].astype(np.int32)
    return n, e, p, inv, node_map, gid2op, idx


@pytest.mark.parametrize("b,d", K.GATHER_SHAPES)
def test_gather_rows(G, b, d):
    n, e, _, _, _, _, _ = gather_inputs(b, d)
    rng = np.random.RandomState(b + d)
    rows = rng.permutation(n)[:b].astype(np.int32)
    keep = (rng.rand(b) > 0.4).astype(np.float32)
    e_d, rows_d, keep_d = cu(e), cu(rows), cu(keep)
    for kd, kh in ((None, None), (keep_d, keep)):
        ws = Workspace(G.lib.gss_loss_workspace_bytes(b, d))
        where = C.c_void_p()
        G._lib.check(G.lib.gss_loss_gather_rows(d, ptr(e_d), ptr(rows_d), ptr(kd), b, ws.ptr, C.byref(where), G.st()))
        assert where.value + 4 * b * d == ws.ptr + ws.nbytes             # E_B is the workspace's last part
        assert np.array_equal(bits(ws.floats_at(where.value, b * d).reshape(b, d)), bits(M.gather_rows(e, rows, kh)))
        ws.check()


@pytest.mark.parametrize("b,d", K.GATHER_SHAPES)
def test_gather_rows_mapped_and_batch(G, b, d):
    n, e, p, inv, node_map, gid2op, idx = gather_inputs(b, d)
    e_d, p_d, inv_d, idx_d, nm_d, g2_d = cu(e), cu(p), cu(inv), cu(idx), cu(node_map), cu(gid2op)
    # (node_map, gid2op, lo, nl, e given, keep wanted): a shard in the middle of the id range, the whole range, an empty shard without e
    variants = [(nm, g2, lo, nl, nl > 0, kw) for nm in (None, node_map) for g2 in (None, gid2op) for lo, nl, kw in ((n, n, True), (n + 3, n - 3, False))]
    variants += [(node_map, None, n, 0, False, True), (None, gid2op, 2 * n, 0, False, True)]
    for nm, g2, lo, nl, has_e, want_keep in variants:
        what = f"node_map={nm is not None} gid2op={g2 is not None} lo={lo} nl={nl}"
        # ---- gss_loss_gather_rows_mapped
        ws = Workspace(G.lib.gss_loss_workspace_bytes(b, d))
        pid, rloc, keep = Out(b, dtype=torch.int32), Out(b, dtype=torch.int32), Out(b)
        where = C.c_void_p()
        G._lib.check(G.lib.gss_loss_gather_rows_mapped(d, ptr(e_d) if has_e else None, ptr(idx_d), ptr(nm_d) if nm is not None else None, lo, nl,
                                                       ptr(g2_d) if g2 is not None else None, pid.ptr, rloc.ptr, keep.ptr if want_keep else None, b,
                                                       ws.ptr, C.byref(where), G.st()), what)
        r_eb, r_pid, r_rloc, r_keep = M.gather_rows_mapped(e[:nl] if has_e else None, idx, nm, lo, nl, g2, d)
        assert np.array_equal(bits(ws.floats_at(where.value, b * d).reshape(b, d)), bits(r_eb)), what
        assert np.array_equal(pid.host("pid"), r_pid) and np.array_equal(rloc.host("rloc"), r_rloc), what
        assert np.array_equal(bits(keep.host("keep")), bits(r_keep)) if want_keep else keep.untouched("keep"), what
        assert nl == 0 or (r_rloc.min() >= 0 and r_rloc.max() <= nl - 1)
        ws.check(what)
        # ---- gss_loss_gather_batch with the translation folded in
        out, pid, rloc, keep = Out(b * (2 * d + 1)), Out(b, dtype=torch.int32), Out(b, dtype=torch.int32), Out(b)
        G._lib.check(G.lib.gss_loss_gather_batch(d, ptr(e_d) if has_e else None, ptr(p_d) if has_e else None, ptr(inv_d) if has_e else None, ptr(idx_d),
                                                 ptr(nm_d) if nm is not None else None, lo, nl, ptr(g2_d) if g2 is not None else None, pid.ptr, rloc.ptr,
                                                 keep.ptr if want_keep else None, None, b, out.ptr, G.st()), what)
        r_out, (r_pid, r_rloc, r_keep) = M.gather_batch(e[:nl] if has_e else None, p[:nl] if has_e else None, inv[:nl] if has_e else None, d, idx=idx,
                                                        node_map=nm, lo=lo, nl=nl, gid2op=g2)
        assert np.array_equal(bits(out.host("[E_B | P_B | inv_B]")), bits(r_out)), what
        assert np.array_equal(pid.host("pid"), r_pid) and np.array_equal(rloc.host("rloc"), r_rloc), what
        assert np.array_equal(bits(keep.host("keep")), bits(r_keep)) if want_keep else keep.untouched("keep"), what
    # ---- gss_loss_gather_batch over prepared rows (idx NULL), with and without keep
    rng = np.random.RandomState(b * d)
    rows = rng.permutation(n)[:b].astype(np.int32)
    keepv = (rng.rand(b) > 0.4).astype(np.float32)
    rows_d, keep_d = cu(rows), cu(keepv)
    for kd, kh in ((None, None), (keep_d, keepv)):
        out = Out(b * (2 * d + 1))
        G._lib.check(G.lib.gss_loss_gather_batch(d, ptr(e_d), ptr(p_d), ptr(inv_d), None, None, 0, n, None, None, None, ptr(kd), ptr(rows_d), b,
                                                 out.ptr, G.st()))
        r_out, ids = M.gather_batch(e, p, inv, d, rows=rows, keep=kh)
        assert ids is None and np.array_equal(bits(out.host("[E_B | P_B | inv_B]")), bits(r_out))
        assert np.array_equal(keep_d.cpu().numpy(), keepv)             # the prepared flags are read, not written


# ================================================================ refusals, before any launch
def test_refusals_by_name(G):
    c = K.case("recipe", 64, 17)
    D = device(G, c)
    d, b, n = 64, 17, c["n"]
    o = dict(loss=Out(1), dx=Out(b, d), dp=Out(b, d), gax=Out(b, d), gam=Out(b, d), pos=Out(n + 5, fill=POS_FREE, dtype=torch.int32),
             de_x=Out(b * d + 1), out=Out(b * (2 * d + 1)), pid=Out(b, dtype=torch.int32), rloc=Out(b, dtype=torch.int32), keep=Out(b))
    ws = Workspace(max(G.lib.gss_loss_workspace_bytes(b, d), G.lib.gss_loss_workspace_bytes_parts(b, d, 2)))
    done = C.c_int32(-1)
    where = C.c_void_p()
    st = G.st()

    def step(d=d, b=b, rows=ptr(D["rows"]), pos_ids=None, pos_set=o["pos"].ptr, w=(None, None, None, None), done_ref=C.byref(done)):
        return G.lib.gss_loss_step(d, b, c["beta"], c["alpha"], o["loss"].ptr, ptr(D["e_b"]), rows, pos_ids, pos_set, None, ptr(D["inv_den"]),
                                   ptr(D["p"]), c["c"], o["dx"].ptr, o["dp"].ptr, *w, 0, None, ws.ptr, st, done_ref)

    def slab(d=d, b=b, rank=0, parts=2):
        return G.lib.gss_loss_slab_sweep(d, b, c["beta"], c["alpha"], ptr(D["e_b"]), rank, parts, ws.ptr, o["de_x"].ptr, st)

    def rows_(d=d, b=b):
        return G.lib.gss_loss_gather_rows(d, ptr(D["e"]), ptr(D["rows"]), None, b, ws.ptr, C.byref(where), st)

    def mapped(d=d, b=b, nl=n):
        return G.lib.gss_loss_gather_rows_mapped(d, ptr(D["e"]), ptr(D["rows"]), None, 0, nl, None, o["pid"].ptr, o["rloc"].ptr, o["keep"].ptr, b, ws.ptr,
                                                 C.byref(where), st)

    def batch(d=d, b=b, idx=ptr(D["rows"]), rows=None):
        return G.lib.gss_loss_gather_batch(d, ptr(D["e"]), ptr(D["p"]), ptr(D["inv_den"]), idx, None, 0, n, None, o["pid"].ptr, o["rloc"].ptr,
                                           o["keep"].ptr, rows, b, o["out"].ptr, st)

    w1, w2, ga, gm = ptr(D["w1t"]), ptr(D["w2t"]), o["gax"].ptr, o["gam"].ptr
    refused = [
        (lambda: step(b=0), "loss_step"), (lambda: step(b=-3), "loss_step"), (lambda: step(d=24), "d=24"), (lambda: step(d=1040), "d=1040"),
        (lambda: step(w=(w1, None, ga, gm)), "loss_step: incomplete"), (lambda: step(w=(w1, w2, None, gm)), "loss_step: incomplete"),
        (lambda: step(w=(w1, w2, ga, None)), "loss_step: incomplete"),
        (lambda: step(rows=None), "loss_step: a batch-position map needs its keys"), (lambda: step(done_ref=None), "gss_loss_step"),
        (lambda: slab(rank=2), "loss_step_slab_sweep"), (lambda: slab(rank=-1), "loss_step_slab_sweep"), (lambda: slab(parts=1), "loss_step_slab_sweep"),
        (lambda: slab(rank=0, parts=0), "loss_step_slab_sweep"), (lambda: slab(b=0), "loss_step_slab_sweep"), (lambda: slab(d=8), "d=8"),
        (lambda: rows_(b=0), "loss_gather_rows"), (lambda: rows_(d=20), "d=20"),
        (lambda: mapped(b=0), "loss_gather_rows_mapped"), (lambda: mapped(nl=-1), "loss_gather_rows_mapped"), (lambda: mapped(d=2048), "d=2048"),
        (lambda: batch(b=0), "loss_gather_batch"), (lambda: batch(idx=None, rows=None), "loss_gather_batch: neither"), (lambda: batch(d=0), "d=0"),
    ]
    for call, text in refused:
        assert call() != 0, text
        assert text in G.lib.gss_last_error().decode(), (text, G.lib.gss_last_error().decode())
    torch.cuda.synchronize()
    assert done.value == -1
    for k, v in o.items():
        assert (v.host(k) == POS_FREE).all() if k == "pos" else v.untouched(k), f"a refused call wrote {k}"
    assert (ws.buf == WS_BYTE).all().item()
    # the same arguments, unrefused, run
    assert step() == 0 and slab() == 0 and rows_() == 0 and mapped() == 0 and batch() == 0
    torch.cuda.synchronize()
