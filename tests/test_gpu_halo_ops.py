"""-m gpu: the halo bookkeeping and the batch preparation of a sharded plan, launcher by launcher, against tests/halo_ops_mirror.py
(held to brute force and to the product's shard layout on the CPU in tests/test_halo_ops_mirror.py): gss_bits_compact, gss_bits_clear /
gss_bits_fill, gss_bits_set_list, gss_halo_need_mark, gss_send_slot_bits, gss_pack_rows / gss_unpack_rows, gss_batch_prepare and the same
job inside a forward SpMM launch (gss_spmm_prep_side), gss_scatter_add_rows_ex, and the two forms of a lazy halo exchange composed from
them on one GPU, the copies between ranks done by the mirror's exchange helper.

Everything here is integers, bits and row copies: every assertion is exact equality with the mirror, over the WHOLE buffer -- what the
contract does not name must keep its pre-fill or its random background -- and every output sits between canaries (tests/guarded.py).
What the end-to-end comparison of a lazy-halo plan with a whole-halo plan (tests/test_gpu_shards.py) cannot see shows here: an order both
sides of an exchange get wrong alike, a row or a bit too many, a write behind a list's end, the block scan's second trip.
No test provokes a fault: every launch gets valid arguments."""
import contextlib
import functools

import numpy as np
import pytest

import guarded
import halo_ops_cases as K
import halo_ops_mirror as M
from guarded import PREFILL, Out, Workspace, cu, ptr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

I32 = dict(dtype=torch.int32)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU")
    import gcn_drug_repurposing_amd as pkg
    from gcn_drug_repurposing_amd import _lib, graph

    class NS:
        pass
    ns = NS()
    ns.lib, ns._lib, ns.graph = pkg.load(), _lib, graph
    ns.st = lambda: _lib.current_stream()
    ns.csr = {}
    return ns


def dev_csr(G, a, key):
    if key not in G.csr:
        G.csr[key] = G.graph.DeviceCSR(a.indptr, a.indices, a.data, a.shape[0], a.shape[1], "cuda")
    return G.csr[key]


def iout(values=None, n=None, fill=PREFILL):
    """a guarded int32 / uint32 buffer, pre-filled or holding `values`"""
    o = Out(len(values) if values is not None else n, fill=fill, **I32)
    if values is not None and len(values):
        o.t.copy_(cu(np.ascontiguousarray(values).view(np.int32)))
    return o


def fout(values):
    o = Out(*values.shape)
    if values.size:
        o.t.copy_(cu(values).reshape(-1))
    return o


def words_of(o, what):
    torch.cuda.synchronize()
    return o.host(what).reshape(-1).view(np.uint32)


def same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.flatnonzero(got.reshape(-1).view(np.uint32) != ref.reshape(-1).view(np.uint32))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:8]}: got {got.reshape(-1)[bad[:4]]}, want {ref.reshape(-1)[bad[:4]]}"


def prefill_like(shape, dtype):
    return np.full(shape, PREFILL, np.int32).view(dtype)


def dev_i64(a):
    return cu(np.ascontiguousarray(a, dtype=np.int64))


LIVE = []          # device inputs of the launches of one test: alive until the test is over


@pytest.fixture(autouse=True)
def _release_inputs():
    yield
    LIVE.clear()


def dv64(a):
    return dv(np.ascontiguousarray(a, dtype=np.int64))


def dv(a):
    """the device address of a host array (None stays None)"""
    if a is None:
        return None
    LIVE.append(cu(a))
    return LIVE[-1].data_ptr()


# ================================================================ bits_compact
def run_compact(G, words, P, off, woff, slot_map, add, n_expected, scratch="exact"):
    """-> (list buffer with ONE entry behind the expected ones, out_off); the input words (guard word included) must come back unchanged"""
    woff = np.ascontiguousarray(woff, dtype=np.int64)
    d_words = cu(np.ascontiguousarray(words).view(np.int32))
    d_map = cu(slot_map) if slot_map is not None else None
    d_off, d_woff = dev_i64(off), dev_i64(woff)
    out, out_off = Out(n_expected + 1, **I32), Out(2 * (P + 1), **I32)
    need = G.lib.gss_bits_compact_scratch_bytes(P, woff.ctypes.data)
    nblk = int(((np.diff(woff) + K.COMPACT_BLOCK_WORDS - 1) // K.COMPACT_BLOCK_WORDS).sum())
    assert need == (nblk * 4 + 15) // 16 * 16 + 8 * (nblk + 1)
    ws = Workspace(need) if scratch != "null" else None
    given = {"exact": need, "small": need - 1, "null": 0}[scratch]
    G._lib.check(G.lib.gss_bits_compact(ptr(d_words), P, ptr(d_woff), woff.ctypes.data, ptr(d_off), ptr(d_map), add, out.ptr, out_off.ptr,
                                        ws.ptr if ws else None, given, G.st()), "gss_bits_compact")
    torch.cuda.synchronize()
    if ws is not None:
        ws.check("bits_compact scratch")
        if scratch == "small":         # a scratch too small by one byte is not used at all: the call allocates its own
            assert (ws.buf == guarded.WS_BYTE).all().item(), "bits_compact wrote to a scratch that is too small"
    same_bits(d_words.cpu().numpy(), np.ascontiguousarray(words).view(np.int32), "the bitmap itself")
    return out.host("list"), out_off.host("out_off").view(np.int64)


def check_compact(G, cs, scratch="exact"):
    lst, off = M.bits_compact(cs.words, cs.woff, cs.off, cs.slot_map, cs.add)
    got, got_off = run_compact(G, K.with_guard(cs.words), cs.P, cs.off, cs.woff, cs.slot_map, cs.add, len(lst), scratch)
    assert np.array_equal(got_off, off), (got_off, off)
    same_bits(got[:len(lst)], lst, "list")
    assert got[len(lst)] == np.int32(PREFILL), "an entry behind out_off[P] was written"
    return lst


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("pattern", K.PATTERNS)
@pytest.mark.parametrize("name", list(K.LAYOUTS))
def test_bits_compact_lists_the_set_bits_of_every_range_in_order(G, name, pattern, form):
    cs = K.compact_case(name, pattern, form)
    lst = check_compact(G, cs)
    if name == "all_empty":
        assert len(lst) == 0                      # no block at all: out_off is zeros, the list untouched (checked above)


@pytest.mark.parametrize("scratch", ["null", "small"])
@pytest.mark.parametrize("name", ["all_empty", "empty_middle", "block_edges"])
def test_bits_compact_allocates_when_the_callers_scratch_is_missing_or_short(G, name, scratch):
    check_compact(G, K.compact_case(name, "random", "add"), scratch)


def test_bits_compact_carries_the_scan_into_its_second_trip(G):
    """1026 blocks: the one-workgroup scan of the block counts walks 1024 blocks per trip and carries the running total"""
    cs = K.compact_big()
    lst = check_compact(G, cs)
    assert len(lst) > 60000


# ================================================================ bits_clear, bits_fill, bits_set_list
@pytest.mark.parametrize("op", ["clear", "fill"])
def test_bits_clear_and_fill_touch_exactly_their_range(G, op):
    fn, mirror = (G.lib.gss_bits_clear, M.bits_clear) if op == "clear" else (G.lib.gss_bits_fill, M.bits_fill)
    spans = [(f, l) for f in K.CLEAR_EDGES for l in K.CLEAR_EDGES] + list(K.CLEAR_SPANS)
    assert any(l <= f for f, l in spans) and any(l - f > 8192 for f, l in spans)
    for k, (first, last) in enumerate(spans):
        bg = K.background(M.words_for(max(last, 96)) + 1, k)
        buf = iout(bg)
        G._lib.check(fn(buf.ptr, first, last, G.st()), op)
        same_bits(words_of(buf, f"bits [{first}, {last})"), mirror(bg, first, last), f"{op} [{first}, {last})")


@pytest.mark.parametrize("case", ["none", "one", "word", "repeats", "n257"])
def test_bits_set_list_sets_exactly_the_listed_bits(G, case):
    rng = np.random.RandomState(21)
    ids = {"none": [], "one": [639], "word": list(rng.permutation(32) + 64), "repeats": [5, 5, 37, 5, 608, 37] * 9,
           "n257": list(rng.randint(0, 640, 257))}[case]
    ids = np.asarray(ids, np.int32)
    bg = K.background(21, 6) & np.uint32(0x33333333)
    buf = iout(bg)
    d_ids = cu(ids) if len(ids) else cu(np.zeros(1, np.int32))
    G._lib.check(G.lib.gss_bits_set_list(buf.ptr, ptr(d_ids), len(ids), G.st()), "gss_bits_set_list")
    same_bits(words_of(buf, "bits"), M.bits_set_list(bg, ids), case)


# ================================================================ halo_need_mark, send_slot_bits
@pytest.mark.parametrize("name", list(K.NEED_LAYOUTS))
def test_halo_need_mark_marks_exactly_the_halo_columns_of_the_listed_rows(G, name):
    cs = K.need_case(name)
    csr = dev_csr(G, cs.a, ("need", name))
    d_off, d_woff = dev_i64(cs.off), dev_i64(cs.woff)
    zero = K.with_guard(np.zeros(int(cs.woff[-1]), np.uint32))
    marked = {}
    for key, rows in cs.lists.items():
        buf = iout(zero)
        G._lib.check(G.lib.gss_halo_need_mark(csr.handle, dv(rows), len(rows), cs.n, cs.P, ptr(d_off), ptr(d_woff), buf.ptr, G.st()), key)
        got = words_of(buf, key)
        same_bits(got, M.halo_need_mark(cs.a.indptr, cs.a.indices, rows, cs.n, cs.off, zero), f"{name} {key}")
        M.check_ranges(got[:-1], cs.off, cs.woff)                      # padding bits stay clear
        assert got[-1] == np.uint32(K.GUARD)                             # the guard word behind w_recv_off[P]
        marked[key] = got
    assert not marked["b8_peers"][:-1].any() and marked["b1"][:-1].any() and marked["b1_far"][:-1].any()
    # marks accumulate over what the bitmap holds: nothing is cleared
    buf = iout(marked["b1"])
    rows = cs.lists["b5"]
    G._lib.check(G.lib.gss_halo_need_mark(csr.handle, dv(rows), len(rows), cs.n, cs.P, ptr(d_off), ptr(d_woff), buf.ptr, G.st()), "again")
    same_bits(words_of(buf, "again"), M.halo_need_mark(cs.a.indptr, cs.a.indices, rows, cs.n, cs.off, marked["b1"]), "accumulated")


def test_halo_need_mark_of_a_matrix_without_halo_columns_marks_nothing(G):
    cs = K.need_case("empty_middle", halo=False)
    csr = dev_csr(G, cs.a, ("need", "flat"))
    zero = K.with_guard(np.zeros(int(cs.woff[-1]), np.uint32))
    buf = iout(zero)
    rows = cs.lists["b301"]
    G._lib.check(G.lib.gss_halo_need_mark(csr.handle, dv(rows), len(rows), cs.n, cs.P, dv64(cs.off), dv64(cs.woff), buf.ptr,
                                          G.st()), "flat")
    same_bits(words_of(buf, "flat"), zero, "no halo column")


@pytest.mark.parametrize("counts", [(33, 0, 64, 1), (0, 33, 64, 1), (40, 9000), (0, 0)], ids=str)
def test_send_slot_bits_writes_every_word_of_every_range(G, counts):
    off, woff = K.layout(counts)
    n_words = int(woff[-1])
    rng = np.random.RandomState(31)
    bits = K.background(16, 7)
    send_rows = rng.randint(0, 512, size=max(int(off[-1]), 1)).astype(np.int32)           # rows repeat: one row goes to several peers
    want = M.send_slot_bits(bits, send_rows[:int(off[-1])], off)
    M.check_ranges(want, off, woff)
    for fill in (PREFILL, 0):                       # equal to the mirror from two different pre-fills: every word was written
        buf = iout(n=n_words + 1, fill=fill)
        G._lib.check(G.lib.gss_send_slot_bits(dv(bits.view(np.int32)), dv(send_rows), len(counts), dv64(off), dv64(woff),
                                              n_words, buf.ptr, G.st()), "gss_send_slot_bits")
        got = words_of(buf, "request words")
        same_bits(got[:n_words], want, str(counts))
        assert got[n_words] == np.uint32(fill & 0xFFFFFFFF), "the word behind the last range was written"


# ================================================================ pack_rows, unpack_rows
@pytest.mark.parametrize("n", K.COPY_COUNTS)
@pytest.mark.parametrize("d", K.COPY_WIDTHS)
def test_pack_rows_copies_the_listed_rows_bit_for_bit(G, d, n):
    rng = np.random.RandomState(41 + d + n)
    src = K.odd_floats(rng, 1200, d)
    rows = rng.randint(0, 1200, size=max(n, 1)).astype(np.int32)
    if n >= 17:
        rows[[1, 9, n - 1]] = rows[0]                 # one row to several peers
        rows[2], rows[3] = 0, 1199
    out = Out(n + 1, d)
    G._lib.check(G.lib.gss_pack_rows(d, dv(src), dv(rows), n, out.ptr, G.st()), "gss_pack_rows")
    torch.cuda.synchronize()
    same_bits(out.host("packed rows"), np.concatenate([M.pack_rows(src, rows[:n]), prefill_like((1, d), np.float32)]), f"pack d={d} n={n}")


@pytest.mark.parametrize("n", K.COPY_COUNTS)
@pytest.mark.parametrize("d", K.COPY_WIDTHS)
def test_unpack_rows_writes_exactly_the_listed_rows(G, d, n):
    rng = np.random.RandomState(43 + d + n)
    src = K.odd_floats(rng, max(n, 1), d)
    rows = rng.choice(1100, size=max(n, 1), replace=False).astype(np.int32)
    if n >= 17:
        rows[0], rows[1] = 1099, 0
        rows[2:] = rng.choice(np.arange(1, 1099), size=n - 2, replace=False)
    dst = Out(1100, d)
    G._lib.check(G.lib.gss_unpack_rows(d, dv(src), dv(rows), n, dst.ptr, G.st()), "gss_unpack_rows")
    torch.cuda.synchronize()
    same_bits(dst.host("unpacked rows"), M.unpack_rows(prefill_like((1100, d), np.float32), src[:n], rows[:n]), f"unpack d={d} n={n}")


# ================================================================ batch_prepare, stand-alone and as the SpMM's side job
PREP_CONFIGS = [("window", True, True), ("window", False, False), ("window", True, False), ("window", False, True), ("empty", True, True),
                ("empty", False, False), ("whole", False, False)]
PREP_D = 64


@functools.lru_cache(maxsize=None)
def spmm_operands():
    a = K.prep_matrix()
    rng = np.random.RandomState(51)
    return cu(rng.randn(a.shape[0], PREP_D).astype(np.float32)), cu(rng.randn(a.shape[0], PREP_D).astype(np.float32))


def spmm_reference(G):
    """the carrying launch without its side job: y = A x, m = y (.) h"""
    if "prep_ref" not in G.csr:
        a = K.prep_matrix()
        csr = dev_csr(G, a, "prep")
        x, h = spmm_operands()
        y, m = Out(a.shape[0], PREP_D), Out(a.shape[0], PREP_D)
        G._lib.check(G.lib.gss_spmm(csr.handle, PREP_D, ptr(x), y.ptr, ptr(h), m.ptr, G.st()), "gss_spmm")
        torch.cuda.synchronize()
        G.csr["prep_ref"] = (guarded.written(y.host("y"), "y").copy(), guarded.written(m.host("m"), "m").copy())
    return G.csr["prep_ref"]


def run_prepare(G, cs, dev, leave_out, side):
    """one batch preparation into fresh guarded outputs -> dict of host arrays (None for the output left out)"""
    outs = {"rloc": Out(cs.b, **I32), "pid": Out(cs.b, **I32), "keep": Out(cs.b), "rlist": Out(cs.b, **I32), "pos": Out(cs.n_op, **I32)}
    p = {k: (None if k == leave_out else o.ptr) for k, o in outs.items()}
    if side:
        a = K.prep_matrix()
        x, h = spmm_operands()
        y, m = Out(a.shape[0], PREP_D), Out(a.shape[0], PREP_D)
        G._lib.check(G.lib.gss_spmm_prep_side(dev_csr(G, a, "prep").handle, PREP_D, ptr(x), y.ptr, ptr(h), m.ptr, None, ptr(dev["idx"]), cs.b,
                                              ptr(dev["node_map"]), cs.lo, cs.nl, ptr(dev["gid2op"]), p["rloc"], p["pid"], p["keep"], p["pos"],
                                              p["rlist"], G.st()), "gss_spmm_prep_side")
        torch.cuda.synchronize()
        ref_y, ref_m = spmm_reference(G)
        same_bits(y.host("y"), ref_y, "y of the launch that carries the preparation")
        same_bits(m.host("m"), ref_m, "m of the launch that carries the preparation")
    else:
        G._lib.check(G.lib.gss_batch_prepare(ptr(dev["idx"]), cs.b, ptr(dev["node_map"]), cs.lo, cs.nl, ptr(dev["gid2op"]), p["rloc"], p["pid"],
                                             p["keep"], p["pos"], p["rlist"], G.st()), "gss_batch_prepare")
        torch.cuda.synchronize()
    return {k: o.host(k).copy() for k, o in outs.items()}


@pytest.mark.parametrize("config", PREP_CONFIGS, ids=lambda c: f"{c[0]}-{'map' if c[1] else 'nomap'}-{'gid2op' if c[2] else 'rel'}")
@pytest.mark.parametrize("b", K.PREP_BATCHES)
def test_batch_prepare_alone_and_inside_an_spmm_launch(G, b, config):
    window, mapped, with_gid2op = config
    cs = K.prep_case(b, window, mapped, with_gid2op)
    dev = {k: (cu(getattr(cs, k)) if getattr(cs, k) is not None else None) for k in ("idx", "node_map", "gid2op")}
    want = M.batch_prepare(cs.idx, cs.node_map, cs.lo, cs.nl, cs.gid2op, prefill_like(cs.n_op, np.int32))
    assert (want["pos"] != np.int32(PREFILL)).sum() == (want["pid"] >= 0).sum()             # pos at the op >= 0 entries and nowhere else
    for leave_out in (None, "rloc", "pid", "keep", "rlist"):
        alone = run_prepare(G, cs, dev, leave_out, side=False)
        inside = run_prepare(G, cs, dev, leave_out, side=True)
        for k in want:
            ref = prefill_like(want[k].shape, want[k].dtype) if k == leave_out else want[k]
            same_bits(alone[k], ref, f"gss_batch_prepare {k} (without {leave_out})")
            same_bits(inside[k], ref, f"gss_spmm_prep_side {k} (without {leave_out})")
            same_bits(inside[k], alone[k], f"the two copies of the batch preparation, {k}")


SPMM_DEFAULTS = {"spmm_giant": 32768, "spmm_slices": 0, "spmm_pin": 0}
CARRIERS = {"pin2": {"spmm_slices": 2, "spmm_pin": 1}, "time2": {"spmm_slices": 2, "spmm_pin": 0}, "giant": {"spmm_giant": 64}, "row_bits": {}}


@contextlib.contextmanager
def knobs(G, **kv):
    """set tuning knobs for the body, restore the defaults whatever happens"""
    try:
        for k, v in kv.items():
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), v))
        yield
    finally:
        for k in kv:
            G._lib.check(G.lib.gss_debug_set_option(k.encode(), SPMM_DEFAULTS[k]))


@pytest.mark.parametrize("carrier", list(CARRIERS))
def test_the_side_job_rides_every_form_of_the_carrying_launch(G, carrier):
    """the launch has one workgroup more whatever its grid: feature slices pinned to XCDs (1-D grid, the slice in the workgroup id), slices
    time-separated (the extra workgroup exists once per slice and prepares in the first only), a matrix with a giant row (three passes: the
    preparation rides in the second), a row bitmap (the filtered launch of a lazy step's top layer)"""
    cs = K.prep_case(K.SPMM_THREADS + 1, "window", True, True)
    a = K.prep_matrix()
    x, h = spmm_operands()
    row_bits = None
    if carrier == "row_bits":
        live = np.random.RandomState(52).rand(a.shape[0]) < 0.3
        live[[0, 3, a.shape[0] - 1]] = True
        row_bits = K.with_guard(M.from_bool(live))
    with knobs(G, **CARRIERS[carrier]):
        csr = dev_csr(G, a, ("prep", carrier))          # (a handle caches the giant-row views of the knob it first ran under)
        ref_y, ref_m = Out(a.shape[0], PREP_D), Out(a.shape[0], PREP_D)
        G._lib.check(G.lib.gss_spmm_filtered(csr.handle, PREP_D, ptr(x), ref_y.ptr, ptr(h), ref_m.ptr, None, dv(row_bits.view(np.int32)) if row_bits is not None else None,
                                             None, None, G.st()), "gss_spmm_filtered")
        outs = {"rloc": Out(cs.b, **I32), "pid": Out(cs.b, **I32), "keep": Out(cs.b), "rlist": Out(cs.b, **I32), "pos": Out(cs.n_op, **I32)}
        y, m = Out(a.shape[0], PREP_D), Out(a.shape[0], PREP_D)
        G._lib.check(G.lib.gss_spmm_prep_side(csr.handle, PREP_D, ptr(x), y.ptr, ptr(h), m.ptr, dv(row_bits.view(np.int32)) if row_bits is not None else None,
                                              dv(cs.idx), cs.b, dv(cs.node_map), cs.lo, cs.nl, dv(cs.gid2op), outs["rloc"].ptr, outs["pid"].ptr,
                                              outs["keep"].ptr, outs["pos"].ptr, outs["rlist"].ptr, G.st()), "gss_spmm_prep_side")
        torch.cuda.synchronize()
    same_bits(y.host("y"), ref_y.host("y"), f"y ({carrier})")
    same_bits(m.host("m"), ref_m.host("m"), f"m ({carrier})")
    if carrier == "row_bits":
        skipped = (y.host("y").view(np.int32) == np.int32(PREFILL)).all(1)
        assert np.array_equal(skipped, ~live)
    else:
        guarded.written(y.host("y"), "y")
    want = M.batch_prepare(cs.idx, cs.node_map, cs.lo, cs.nl, cs.gid2op, prefill_like(cs.n_op, np.int32))
    for k in want:
        same_bits(outs[k].host(k), want[k], f"{k} ({carrier})")


# ================================================================ scatter_add_rows_ex
@pytest.mark.parametrize("mode", K.SCATTER_MODES)
@pytest.mark.parametrize("b", [1, 333])
@pytest.mark.parametrize("d", [16, 256])
def test_scatter_add_rows_ex_skips_members_but_resets_their_positions(G, d, b, mode):
    cs = K.scatter_case(d, b, mode)
    pos0 = np.arange(cs.n_pos, dtype=np.int32) + 5
    for with_keep in (True, False):
        for with_pos in (True, False):
            keep = cs.keep if with_keep else None
            dst, pos = fout(cs.dst), iout(pos0)
            G._lib.check(G.lib.gss_scatter_add_rows_ex(d, dv(cs.src), dv(cs.rows), dv(keep) if with_keep else None, b, dst.ptr,
                                                       pos.ptr if with_pos else None, dv(cs.pos_ids) if with_pos else None, G.st()), mode)
            torch.cuda.synchronize()
            want, want_pos = M.scatter_add_rows(cs.dst, cs.src, cs.rows, keep, pos0 if with_pos else None, cs.pos_ids)
            same_bits(dst.host("dst"), want, f"dst ({mode}, keep {with_keep})")          # one addend per row: the fp32 sum is exact
            same_bits(pos.host("pos"), want_pos if with_pos else pos0, f"pos ({mode}, pos_clear {with_pos})")


# ================================================================ the two forms of a lazy exchange, composed on one GPU
EX_D = 16


def operand(s, tag):
    """own rows that say where they come from: (global node id, feature, tag); the boundary rows are pre-filled"""
    x = prefill_like((s.n + s.n_halo, EX_D), np.float32).copy()
    x[:s.n] = ((s.lo + np.arange(s.n))[:, None] * 64 + np.arange(EX_D)[None, :] + tag * 0.25).astype(np.float32)
    return x


def gpu_compact(G, s, words, side):
    """a rank's bits_compact as the plan calls it: requests over the send slots -> own rows; needs over the halo slots -> boundary rows"""
    if side == "send":
        off, woff, slot_map, add = s.send_off, s.wsend_off, (s.send_rows if len(s.send_rows) else np.zeros(1, np.int32)), 0
    else:
        off, woff, slot_map, add = s.recv_off, s.wrecv_off, None, s.n
    n_exp = int(M.to_bool(words[:int(woff[-1])]).sum())
    got, cnt = run_compact(G, words, len(off) - 1, off, woff, slot_map, add, n_exp)
    assert cnt[-1] == n_exp and got[n_exp] == np.int32(PREFILL)
    return got[:n_exp].copy(), cnt.copy()


def gpu_transfer(G, ranks, ops, send, recv):
    """pack on every rank, the copies between the ranks by the mirror, unpack on every rank -> the operands afterwards"""
    sendbuf = []
    for s in ranks:
        lst = send[s.rank][0]
        out = Out(len(lst) + 1, EX_D)
        G._lib.check(G.lib.gss_pack_rows(EX_D, dv(ops[s.rank]), dv(lst) if len(lst) else None, len(lst), out.ptr, G.st()), "pack")
        torch.cuda.synchronize()
        sendbuf.append(out.host("send buffer")[:len(lst)].copy())
    # (exchange_rows refuses a pair of ranks whose counts differ: the sender's list length is the receiver's, per peer)
    recvbuf = M.exchange_rows(sendbuf, [send[s.rank][1] for s in ranks], [np.zeros((len(recv[s.rank][0]), EX_D), np.float32) for s in ranks],
                              [recv[s.rank][1] for s in ranks], EX_D)
    after = []
    for s in ranks:
        lst = recv[s.rank][0]
        dst = fout(ops[s.rank])
        G._lib.check(G.lib.gss_unpack_rows(EX_D, dv(recvbuf[s.rank]) if len(lst) else None, dv(lst) if len(lst) else None, len(lst), dst.ptr,
                                           G.st()), "unpack")
        torch.cuda.synchronize()
        after.append(dst.host("operand").copy())
    return after


def check_arrived(s, before, after, arrived, tag):
    """boundary row n + k holds the owner's row of node remote[k] exactly where `arrived`; every other row is as before"""
    want = before.copy()
    want[s.n:][arrived] = (s.remote[arrived][:, None] * 64 + np.arange(EX_D)[None, :] + tag * 0.25).astype(np.float32)
    same_bits(after, want, f"rank {s.rank}: operand after the transfer")


def test_receiver_driven_exchange_fetches_exactly_the_referenced_rows(G):
    ranks = K.shard_layouts(3)
    rng = np.random.RandomState(61)
    lists = [np.where(rng.rand(7) < 0.2, -1, rng.randint(0, s.n, 7)).astype(np.int32) for s in ranks]
    need = []
    for s in ranks:
        buf = iout(K.with_guard(np.zeros(int(s.wrecv_off[-1]), np.uint32)))
        G._lib.check(G.lib.gss_halo_need_mark(dev_csr(G, s.a.astype(np.float32), ("shard", s.rank)).handle, dv(lists[s.rank]), 7, s.n, 3,
                                              dv64(s.recv_off), dv64(s.wrecv_off), buf.ptr, G.st()), "need")
        need.append(words_of(buf, "need words").copy())
        assert need[-1][-1] == np.uint32(K.GUARD)
    req = M.exchange_words(need, [s.wrecv_off for s in ranks], [K.with_guard(np.zeros(int(s.wsend_off[-1]), np.uint32)) for s in ranks],
                           [s.wsend_off for s in ranks])
    recv = {s.rank: gpu_compact(G, s, need[s.rank], "recv") for s in ranks}
    send = {s.rank: gpu_compact(G, s, req[s.rank], "send") for s in ranks}
    for a in ranks:
        for b in ranks:       # B's send count toward A is A's receive count from B
            assert send[b.rank][1][a.rank + 1] - send[b.rank][1][a.rank] == recv[a.rank][1][b.rank + 1] - recv[a.rank][1][b.rank]
    ops = [operand(s, 1) for s in ranks]
    after = gpu_transfer(G, ranks, ops, send, recv)
    for s in ranks:
        cols = np.unique(np.concatenate([s.a[r].indices for r in lists[s.rank] if r >= 0]))
        referenced = np.zeros(s.n_halo, bool)
        referenced[cols[cols >= s.n] - s.n] = True
        assert 0 < referenced.sum() < s.n_halo
        assert np.array_equal(recv[s.rank][0], s.n + np.flatnonzero(referenced))
        check_arrived(s, ops[s.rank], after[s.rank], referenced, 1)


def test_sender_driven_exchange_sets_exactly_the_arrived_rows_bits(G):
    ranks = K.shard_layouts(3)
    assert any(s.n % 32 for s in ranks)                 # the word that straddles the own rows and the halo is shared
    nz, reqw = [], []
    for s in ranks:
        rows_t = s.n + s.n_halo
        bits = K.background(M.words_for(rows_t), 70 + s.rank)          # own rows: which can be non-zero; halo bits: leftovers of an earlier step
        bits = M.bits_clear(bits, rows_t, len(bits) * 32)
        nz.append(K.with_guard(bits))
        n_words = int(s.wsend_off[-1])
        buf = iout(n=n_words + 1)
        G._lib.check(G.lib.gss_send_slot_bits(dv(nz[-1].view(np.int32)), dv(s.send_rows), 3, dv64(s.send_off), dv64(s.wsend_off),
                                              n_words, buf.ptr, G.st()), "send_slot_bits")
        got = words_of(buf, "request words").copy()
        assert got[n_words] == np.uint32(PREFILL)
        got[n_words] = K.GUARD
        same_bits(got[:n_words], M.send_slot_bits(bits, s.send_rows, s.send_off), f"rank {s.rank}: request words")
        reqw.append(got)
    needw = M.exchange_words(reqw, [s.wsend_off for s in ranks], [K.with_guard(np.zeros(int(s.wrecv_off[-1]), np.uint32)) for s in ranks],
                             [s.wrecv_off for s in ranks])
    send = {s.rank: gpu_compact(G, s, reqw[s.rank], "send") for s in ranks}
    recv = {s.rank: gpu_compact(G, s, needw[s.rank], "recv") for s in ranks}
    ops = [operand(s, 2) for s in ranks]
    after = gpu_transfer(G, ranks, ops, send, recv)
    owner_bit = {}
    for s in ranks:
        own = M.to_bool(nz[s.rank][:-1])[:s.n]
        owner_bit.update({s.lo + r: bool(own[r]) for r in range(s.n)})
    for s in ranks:
        lst = recv[s.rank][0]
        buf = iout(nz[s.rank])
        G._lib.check(G.lib.gss_bits_clear(buf.ptr, s.n, s.n + s.n_halo, G.st()), "bits_clear")
        G._lib.check(G.lib.gss_bits_set_list(buf.ptr, dv(lst) if len(lst) else None, len(lst), G.st()), "bits_set_list")
        got = words_of(buf, "row bits")
        arrived = np.array([owner_bit[int(g)] for g in s.remote], bool)            # the boundary rows whose owner marked them
        assert 0 < arrived.sum() < s.n_halo
        want = M.to_bool(nz[s.rank][:-1])
        want[s.n:s.n + s.n_halo] = arrived
        same_bits(got[:-1], M.from_bool(want, len(got) - 1), f"rank {s.rank}: own bits unchanged, halo bits = the arrived rows")
        assert got[-1] == np.uint32(K.GUARD)
        assert np.array_equal(lst, s.n + np.flatnonzero(arrived))
        check_arrived(s, ops[s.rank], after[s.rank], arrived, 2)
