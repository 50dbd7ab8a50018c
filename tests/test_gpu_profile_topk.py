"""GPU: gss_profile_topk (csrc/profile_topk.hip) for equality against np.argsort(-col[members], kind="stable")[:k] -- indices, value bits
and counts --, through groups, lists, strides and guard bytes, its bit-stability contract and its refusals by name; gss_topk_overlap
against np.intersect1d; diffusion.top_nodes / top_overlap on the three kinds of input.  No tolerance anywhere."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import profile_topk_mirror as T  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import top_nodes, top_overlap  # noqa: E402

pytestmark = pytest.mark.gpu
SENT_I, SENT_V, GUARD = -77, -7.0, 0x5A
KMAX = 1024


def upload(p, ld=None):
    """host [K][N] -> device x [N][ld], profile c in column c, NaN in the columns past K"""
    k, n = p.shape
    x = torch.full((n, ld or k), float("nan"), dtype=torch.float64, device="cuda")
    x[:, :k] = torch.from_numpy(p).cuda().t()
    return x


def i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int32), dtype=torch.int32, device="cuda")


def ptr(t):
    return t if isinstance(t, int) else _lib.ptr(t)


def call(n, x, ld, nc, cols, G, group, k, idx, val, cnt, ws, ws_bytes):
    lib = _lib.load()
    rc = lib.gss_profile_topk(n, ptr(x), ld, nc, ptr(cols), G, ptr(group), k, ptr(idx), ptr(val), ptr(cnt), ptr(ws), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, lib.gss_last_error().decode(errors="replace")


def select(x, nc, k, G=1, group=None, cols=None):
    """the raw entry point with sentinel-filled outputs and guard words behind idx, val, cnt and the workspace
    -> host (idx [nc][G][k], val bits [nc][G][k], cnt [nc][G]); asserts the guards"""
    n, ld = x.shape[0], (x.stride(0) if x.shape[0] > 1 else x.shape[1])
    need = int(_lib.load().gss_profile_topk_workspace_bytes(n, nc, G, k))
    assert need == T.workspace_bytes(n, nc, G, k)
    m = nc * G * k
    idx = torch.full((m + 16,), SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((m + 16,), SENT_V, dtype=torch.float64, device="cuda")
    cnt = torch.full((nc * G + 16,), SENT_I, dtype=torch.int32, device="cuda")
    ws = torch.full((need + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 8 == 0
    rc, msg = call(n, x, ld, nc, None if cols is None else i32(cols), G, None if group is None else i32(group), k, idx, val, cnt, ws, need)
    assert rc == 0, msg
    assert bool((idx[m:] == SENT_I).all()) and bool((val[m:] == SENT_V).all()) and bool((cnt[nc * G:] == SENT_I).all())
    assert bool((ws[need:] == GUARD).all())
    return (idx[:m].view(nc, G, k).cpu().numpy(), val[:m].view(nc, G, k).cpu().numpy().view(np.int64), cnt[:nc * G].view(nc, G).cpu().numpy())


def expected(p, group, G, k=KMAX):
    """the statement for every column of p [K][N] -> (idx [K][G][k], val bits, cnt [K][G])"""
    parts = [T.expected(v, group, G, k) for v in p]
    return tuple(np.stack([q[i] for q in parts]) for i in range(3))


def cut(want, k, cols=None):
    """the statement at a smaller k (and for a column list) out of the one computed at KMAX"""
    idx, val, cnt = (w if cols is None else w[np.asarray(cols)] for w in want)
    idx, val = idx[:, :, :k].copy(), val[:, :, :k].copy()
    flagged = cnt < 0
    idx[flagged], val[flagged] = -1, T.NAN_BITS
    return idx, val, np.where(flagged, -1, np.minimum(cnt, k)).astype(np.int32)


def check(got, want, what):
    for name, a, b in zip(("idx", "val", "cnt"), got, want):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)


@pytest.mark.parametrize("n", T.SIZES)
def test_exact_against_argsort(n):
    p = T.columns(n, 34, 7 * n)
    assert n < 64 or np.isinf(p[2]).any()                                       # +-inf are ordinary extremes
    x = upload(p)
    ks = [k for k in (1, 7, 64, 1024, n + 3) if k <= 1024]                      # n + 3: more places than nodes
    for G, group in ((1, None), (3, T.groups(n, 3, n))):
        want = expected(p, group, G)
        for k in ks:
            check(select(x, 34, k, G, group), cut(want, k), (n, G, k))
        check(select(x, 1, 7, G, group, [3]), cut(want, 7, [3]), (n, G, "one column"))


def test_ties_across_the_kth_place():
    n = 70000                                                                   # the middle run sits at indices with a third 8-bit digit
    v = np.full(n, -1.0)
    v[66000:] = 0.5
    v[::7000] = 2.0
    flat = np.full(n, 0.25)
    p = np.stack([v, flat, -v])
    x = upload(p)
    group = T.groups(n, 2, 5)
    for G, grp in ((1, None), (2, group)):
        want = expected(p, grp, G)
        for k in (5, 10, 11, 64, 1024):
            got = select(x, 3, k, G, grp)
            check(got, cut(want, k), (G, k))
            for g in range(G):                                                  # all equal: the first k nodes of the group
                assert np.array_equal(got[0][1, g], T.members_of(grp, n, g)[:k])


def test_groups():
    n = 3000
    p = T.columns(n, 9, 17)
    x = upload(p)
    g8 = T.groups(n, 8, 3, empty=5)                                             # G = 8, group 5 empty
    small = np.flatnonzero(g8 == 2)[40:]
    g8[small] = -1                                                              # group 2: 40 nodes, fewer than k
    want = expected(p, g8, 8)
    for k in (1, 64, 1024):
        got = select(x, 9, k, 8, g8)
        check(got, cut(want, k), k)
        assert np.all(got[2][:, 5] == 0) and np.all(got[0][:, 5] == -1) and np.all(got[1][:, 5] == T.NAN_BITS)
        assert np.all(got[2][:, 2] == min(k, 40)) and np.all(got[0][:, 2, 40:] == -1)
    only = np.full(n, -1, np.int32)
    only[[5, 17]] = 0                                                           # G = 1 with a group array
    check(select(x, 9, 7, 1, only), expected(p, only, 1, 7), "two members")
    check(select(x, 9, 7, 1, None), expected(p, None, 1, 7), "null group")


def test_nan_flags_its_own_group_only():
    n = 2000
    p = T.columns(n, 6, 23)
    group = T.groups(n, 3, 8)
    p[1, np.flatnonzero(group == 1)[11]] = np.nan                               # column 1: a NaN at a node of group 1
    p[2, np.flatnonzero(group == -1)[3]] = np.nan                               # column 2: a NaN at a node of no group
    p[4, np.flatnonzero(group == 0)[0]] = np.nan
    p[4, np.flatnonzero(group == 2)[5]] = np.nan
    got = select(upload(p), 6, 20, 3, group)
    check(got, expected(p, group, 3, 20), "nan")
    assert got[2].tolist() == [[20, 20, 20], [20, -1, 20], [20, 20, 20], [20, 20, 20], [-1, 20, -1], [20, 20, 20]]
    assert np.all(got[0][1, 1] == -1) and np.all(got[1][1, 1] == T.NAN_BITS)
    flagged = select(upload(p), 6, 20, 1, None)                                 # without groups the NaN of column 2 counts
    assert flagged[2][:, 0].tolist() == [20, -1, -1, 20, -1, 20]


def test_lists_strides_and_the_null_list():
    n, k = 1000, 40
    p = T.columns(n, k, 11)
    group = T.groups(n, 2, 4)
    want = expected(p, group, 2, 33)
    x = upload(p, ld=k + 9)                                                     # NaN in the unused columns of x
    cols = np.concatenate([np.random.RandomState(2).permutation(k), [3, 3, 0, k - 1, 17, 3]])     # permuted, with repeats
    check(select(x, len(cols), 33, 2, group, cols), cut(want, 33, cols), "list")
    check(select(x, k, 33, 2, group), want, "null list")
    check(select(x, 7, 33, 2, group), cut(want, 33, np.arange(7)), "a prefix")
    one = upload(p[:, :1].copy())                                               # n = 1: a single row
    got = select(one, k, 3)
    assert np.all(got[2] == 1) and np.all(got[0][:, 0, 0] == 0) and np.all(got[0][:, 0, 1:] == -1)
    assert np.array_equal(got[1][:, 0, 0], p[:, 0].view(np.int64))


def test_more_columns_than_a_panel():
    n, k = 65, 2 * T.PANEL + 3
    p = T.columns(n, k, 5)
    cols = np.random.RandomState(4).permutation(k)
    check(select(upload(p), k, 5, 1, None, cols), cut(expected(p, None, 1, 5), 5, cols), "panels")


def test_bit_stability():
    n, k = 16385, 300
    p = T.columns(n, k, 13)
    group = T.groups(n, 2, 6)
    x = upload(p)
    whole, again = select(x, k, 20, 2, group), select(x, k, 20, 2, group)
    check(again, whole, "two runs")
    for c in (0, 2, 63, 64, 150, 299):                                          # a column alone == the column inside the 300-column call
        check(select(x, 1, 20, 2, group, [c]), cut(whole, 20, [c]), c)
    check(select(x, 3, 20, 2, group, [299, 2, 299]), cut(whole, 20, [299, 2, 299]), "another position")
    wide = upload(p[[2, 150]], ld=7)                                            # another ld, other neighbours
    check(select(wide, 2, 20, 2, group), cut(whole, 20, [2, 150]), "another matrix")
    check(cut(whole, 20, [1, 2, 7]), expected(p[[1, 2, 7]], group, 2, 20), "the statement")


def test_refusals_by_name():
    n, w, k, G = 8, 6, 3, 2
    x = torch.rand(n, w, dtype=torch.float64, device="cuda")
    group = i32([0, 1, -1, 0, 1, 1, 0, -1])
    idx = torch.full((w, G, k), SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((w, G, k), SENT_V, dtype=torch.float64, device="cuda")
    cnt = torch.full((w, G), SENT_I, dtype=torch.int32, device="cuda")
    need = T.workspace_bytes(n, w, G, k)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    ok = dict(n=n, x=x, ld=w, nc=w, cols=None, G=G, group=group, k=k, idx=idx, val=val, cnt=cnt, ws=ws, ws_bytes=need)
    cases = [(dict(n=0), "n=0"), (dict(n=(1 << 24) + 1), "above the limit of 16777216"),   # refused before any memory of that size is needed
             (dict(k=0), "k=0 is outside [1, 1024]"), (dict(k=1025), "k=1025 is outside [1, 1024]"), (dict(G=0), "G=0 groups is outside [1, 8]"),
             (dict(G=9), "G=9 groups is outside [1, 8]"), (dict(nc=-1), "nc=-1"), (dict(ld=0), "ld=0"), (dict(x=0), "x is null"),
             (dict(idx=0), "idx is null"), (dict(val=0), "val is null"), (dict(cnt=0), "cnt is null"), (dict(ws=0), "workspace is null"),
             (dict(group=None), "group is null (every node in group 0) and G=2 is not 1"), (dict(ld=3), "ld=3 is below nc=6"),
             (dict(ws=ws.data_ptr() + 4), "workspace is not 8-byte aligned"),
             (dict(ws_bytes=need - 1), f"workspace of {need - 1} bytes is below the {need} that n=8, nc=6 need"),
             (dict(nc=3, cols=i32([0, 6, 7])), "cols[1] = 6 is outside [0, ld=6)"), (dict(nc=3, cols=i32([1, 2, -1])), "cols[2] = -1 is outside [0, ld=6)"),
             (dict(group=i32([0, 1, -1, 0, 2, 1, 0, 3])), "group[4] = 2 is outside [-1, G=2)"),
             (dict(group=i32([0, 1, -2, 0, 1, 1, 0, 0])), "group[2] = -2 is outside [-1, G=2)")]
    for change, message in cases:
        rc, msg = call(**dict(ok, **change))
        assert rc == -22 and msg.startswith("profile_topk: ") and message in msg, (message, rc, msg)
    assert bool((idx == SENT_I).all()) and bool((val == SENT_V).all()) and bool((cnt == SENT_I).all())   # no refused call wrote anything
    rc, msg = call(**dict(ok, nc=0, x=0, idx=0, val=0, cnt=0, ws=0, ws_bytes=0))             # nc = 0: a no-op, whatever the pointers
    assert rc == 0, msg
    rc, msg = call(**dict(ok, nc=2, cols=i32([5, 0])))
    assert rc == 0, msg
    want = expected(x.cpu().numpy().T[[5, 0]], group.cpu().numpy(), G, k)
    assert np.array_equal(idx[:2].cpu().numpy(), want[0]) and np.array_equal(cnt[:2].cpu().numpy(), want[2])
    assert np.array_equal(val[:2].cpu().numpy().view(np.int64), want[1]) and bool((idx[2:] == SENT_I).all()) and bool((cnt[2:] == SENT_I).all())
    # lists of more than one 256-thread block of the check: the least offending position is named, cols' before group's, nothing is
    # written, and the status words are armed again by every call
    n, w, L = 70, 8, 300
    x = torch.rand(n, w, dtype=torch.float64, device="cuda")
    h = x.cpu().numpy().T
    rng = np.random.RandomState(3)
    g_cols, g_group = rng.randint(0, w, L), T.groups(n, G, 5)

    def with_bad(v, *entries):
        u = np.array(v)
        for at, e in entries:
            u[at] = e
        return i32(u)
    idx = torch.full((L, G, k), SENT_I, dtype=torch.int32, device="cuda")
    val = torch.full((L, G, k), SENT_V, dtype=torch.float64, device="cuda")
    cnt = torch.full((L, G), SENT_I, dtype=torch.int32, device="cuda")
    need = T.workspace_bytes(n, L, G, k)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    ok = dict(n=n, x=x, ld=w, nc=L, cols=i32(g_cols), G=G, group=i32(g_group), k=k, idx=idx, val=val, cnt=cnt, ws=ws, ws_bytes=need)
    tall = torch.rand(L, w, dtype=torch.float64, device="cuda")                # n = 300, nc = 2: the group list is the longer one
    tall_group = T.groups(L, G, 6)
    tall_case = dict(n=L, x=tall, nc=2, cols=i32([7, 1]), ws_bytes=T.workspace_bytes(L, 2, G, k))
    assert tall_case["ws_bytes"] <= need
    for change, message in ((dict(cols=with_bad(g_cols, (290, 8), (270, -3))), "cols[270] = -3 is outside [0, ld=8)"),
                            (dict(cols=with_bad(g_cols, (290, 8)), group=with_bad(g_group, (5, 2))), "cols[290] = 8 is outside [0, ld=8)"),
                            (dict(group=with_bad(g_group, (69, -2))), "group[69] = -2 is outside [-1, G=2)"),
                            (dict(cols=None, nc=w, group=with_bad(g_group, (69, 2))), "group[69] = 2 is outside [-1, G=2)"),
                            (dict(tall_case, group=with_bad(tall_group, (299, 2))), "group[299] = 2 is outside [-1, G=2)")):
        rc, msg = call(**dict(ok, **change))
        assert rc == -22 and msg.startswith("profile_topk: ") and message in msg, (message, rc, msg)
        assert bool((idx == SENT_I).all()) and bool((val == SENT_V).all()) and bool((cnt == SENT_I).all()), message

    def host(rows):
        return idx[:rows].cpu().numpy(), val[:rows].cpu().numpy().view(np.int64), cnt[:rows].cpu().numpy()
    rc, msg = call(**ok)                                                        # the same buffers, valid lists
    assert rc == 0, msg
    check(host(L), expected(h[g_cols], g_group, G, k), "after the refusals")
    rc, msg = call(**dict(ok, **dict(tall_case, group=i32(tall_group))))
    assert rc == 0, msg
    check(host(2), expected(tall.cpu().numpy().T[[7, 1]], tall_group, G, k), "the longer group list")
    # a null list beside a given one == the explicit list, bit for bit: cols null with a group list, a column list with group null

    def run(**change):
        idx.fill_(SENT_I), val.fill_(SENT_V), cnt.fill_(SENT_I)
        rc, msg = call(**dict(ok, **change))
        assert rc == 0, msg
        return idx.flatten().cpu().numpy(), val.flatten().cpu().numpy().view(np.int64), cnt.flatten().cpu().numpy()

    def first(got, rows, groups):
        return got[0][:rows * groups * k].reshape(rows, groups, k), got[1][:rows * groups * k].reshape(rows, groups, k), got[2][:rows * groups].reshape(rows, groups)
    null = run(cols=None, nc=w)
    check(null, run(cols=i32(np.arange(w)), nc=w), "null cols, whole buffers")
    check(first(null, w, G), expected(h, g_group, G, k), "null cols")
    null = run(group=None, G=1)
    check(null, run(group=i32(np.zeros(n)), G=1), "null group, whole buffers")
    check(first(null, L, 1), expected(h[g_cols], None, 1, k), "null group")

# ---- gss_topk_overlap -------------------------------------------------------------------------------------------------------------------------

def overlap_call(S, G, k, idx, cnt, T_, a, b, shared):
    lib = _lib.load()
    rc = lib.gss_topk_overlap(S, G, k, ptr(idx), ptr(cnt), T_, ptr(a), ptr(b), ptr(shared), _lib.current_stream())
    torch.cuda.synchronize()
    return rc, lib.gss_last_error().decode(errors="replace")


@pytest.mark.parametrize("k", (1, 7, 64, 1000))
def test_overlap_against_intersect1d(k):
    n, S, G = 3000, 12, 3
    p = T.columns(n, S, 41)
    p[5] = -p[4]                                                                # selections 4 and 5 of a uniform column and its negative: disjoint at small k
    group = T.groups(n, G, 2)
    p[7, np.flatnonzero(group == 1)[2]] = np.nan                                # selection 7 is flagged in group 1
    h_idx, _, h_cnt = expected(p, group, G, k)
    x = upload(p)
    m = S * G * k
    idx = torch.full((m + 16,), SENT_I, dtype=torch.int32, device="cuda")
    val = torch.empty(m, dtype=torch.float64, device="cuda")
    cnt = torch.full((S * G + 16,), SENT_I, dtype=torch.int32, device="cuda")
    need = T.workspace_bytes(n, S, G, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc, msg = call(n, x, S, S, None, G, i32(group), k, idx, val, cnt, ws, need)
    assert rc == 0, msg
    assert np.array_equal(idx[:m].view(S, G, k).cpu().numpy(), h_idx) and np.array_equal(cnt[:S * G].view(S, G).cpu().numpy(), h_cnt)
    a = [0, 1, 4, 7, 2, 0, 3, 11, 0, 8]                                         # a pair with itself, a disjoint pair, a flagged side, repeats
    b = [0, 2, 5, 3, 7, 0, 3, 10, 9, 4]
    want = T.expected_overlap(h_idx, h_cnt, a, b)
    assert np.array_equal(want[0], h_cnt[0]) and np.array_equal(want[5], want[0])              # with itself: shared == cnt
    assert want[3, 1] == -1 and want[4, 1] == -1 and want[3, 0] >= 0
    if k <= 64:
        assert want[2, 0] == 0                                                  # disjoint
    shared = torch.full((len(a) * G + 16,), SENT_I, dtype=torch.int32, device="cuda")
    rc, msg = overlap_call(S, G, k, idx, cnt, len(a), i32(a), i32(b), shared)
    assert rc == 0, msg
    assert np.array_equal(shared[:len(a) * G].view(len(a), G).cpu().numpy(), want) and bool((shared[len(a) * G:] == SENT_I).all())
    one = torch.full((G,), SENT_I, dtype=torch.int32, device="cuda")            # an entry depends on its own pair only
    rc, msg = overlap_call(S, G, k, idx, cnt, 1, i32([a[8]]), i32([b[8]]), one)
    assert rc == 0 and np.array_equal(one.cpu().numpy(), want[8]), msg


def test_overlap_refusals_by_name():
    S, G, k = 4, 2, 5
    idx = torch.zeros(S, G, k, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(S, G, dtype=torch.int32, device="cuda")
    shared = torch.full((3, G), SENT_I, dtype=torch.int32, device="cuda")
    ok = dict(S=S, G=G, k=k, idx=idx, cnt=cnt, T_=3, a=i32([0, 1, 2]), b=i32([3, 3, 0]), shared=shared)
    cases = [(dict(S=0), "S=0"), (dict(k=0), "k=0 is outside [1, 1024]"), (dict(k=1025), "k=1025 is outside [1, 1024]"), (dict(G=0), "G=0 groups is outside [1, 8]"),
             (dict(G=9), "G=9 groups is outside [1, 8]"), (dict(T_=-1), "T=-1"), (dict(idx=0), "idx is null"), (dict(cnt=0), "cnt is null"),
             (dict(a=0), "a is null"), (dict(b=0), "b is null"), (dict(shared=0), "shared is null"),
             (dict(a=i32([0, 4, 9])), "a[1] = 4 is outside [0, S=4)"), (dict(b=i32([3, 3, -1])), "b[2] = -1 is outside [0, S=4)")]
    for change, message in cases:
        rc, msg = overlap_call(**dict(ok, **change))
        assert rc == -22 and msg.startswith("topk_overlap: ") and message in msg, (message, rc, msg)
    assert bool((shared == SENT_I).all())
    rc, msg = overlap_call(**dict(ok, T_=0, a=0, b=0, shared=0))
    assert rc == 0, msg
    rc, msg = overlap_call(**ok)
    assert rc == 0 and bool((shared == 0).all()), msg                           # cnt = 0 everywhere: nothing shared
    # lists of more than one 256-thread block of the check: the least offending position is named, a's before b's, nothing is written,
    # and the status words are armed again by every call.  (Neither list may be null here: there is no null-list case.)
    S, L = 8, 300
    rng = np.random.RandomState(3)
    h_idx = np.stack([np.stack([rng.permutation(12)[:k] for _ in range(G)]) for _ in range(S)]).astype(np.int32)
    h_cnt = rng.randint(0, k + 1, size=(S, G)).astype(np.int32)
    h_cnt[3, 1] = -1                                                            # a flagged selection
    for s in range(S):
        for g in range(G):
            h_idx[s, g, max(h_cnt[s, g], 0):] = -1
    idx, cnt = torch.from_numpy(h_idx).cuda(), torch.from_numpy(h_cnt).cuda()
    ga, gb = rng.randint(0, S, L), rng.randint(0, S, L)

    def with_bad(v, *entries):
        u = v.copy()
        for at, e in entries:
            u[at] = e
        return i32(u)
    shared = torch.full((L, G), SENT_I, dtype=torch.int32, device="cuda")
    ok = dict(S=S, G=G, k=k, idx=idx, cnt=cnt, T_=L, a=i32(ga), b=i32(gb), shared=shared)
    for change, message in ((dict(a=with_bad(ga, (290, 8), (270, -3))), "a[270] = -3 is outside [0, S=8)"),
                            (dict(a=with_bad(ga, (290, 8)), b=with_bad(gb, (5, 9))), "a[290] = 8 is outside [0, S=8)"),
                            (dict(b=with_bad(gb, (299, 8))), "b[299] = 8 is outside [0, S=8)")):
        rc, msg = overlap_call(**dict(ok, **change))
        assert rc == -22 and msg.startswith("topk_overlap: ") and message in msg, (message, rc, msg)
        assert bool((shared == SENT_I).all()), message
    rc, msg = overlap_call(**ok)                                                # the same buffers, valid lists
    assert rc == 0, msg
    want = T.expected_overlap(h_idx, h_cnt, ga, gb)
    assert (want == -1).any() and (want > 0).any() and np.array_equal(shared.cpu().numpy(), want)


# ---- diffusion.top_nodes / top_overlap --------------------------------------------------------------------------------------------------------

def test_top_nodes_on_the_three_kinds_of_input():
    n, k = 333, 9
    p = T.columns(n, k, 21)
    group = T.groups(n, 2, 1)
    want = expected(p, group, 2, 20)
    x = upload(p, ld=k + 3)

    def host(res):
        idx, val, cnt = res
        assert idx.is_cuda and idx.dtype == torch.int32 and val.dtype == torch.float64 and cnt.dtype == torch.int32
        return idx.cpu().numpy(), val.cpu().numpy().view(np.int64), cnt.cpu().numpy()
    check(host(top_nodes(x[:, :k], [4, 0, 4], groups=group)), cut(want, 20, [4, 0, 4]), "device tensor")
    check(host(top_nodes(x[:, :k], [4, 0, 4], groups=torch.from_numpy(group).cuda(), n_groups=2)), cut(want, 20, [4, 0, 4]), "device groups")
    check(host(top_nodes(p, groups=group.astype(np.int64))), want, "host array, every profile")
    check(host(top_nodes(p, k=5)), expected(p, None, 1, 5), "no groups")
    named = {"p%d" % j: p[j] for j in range(k)}
    res = top_nodes(named, ["p7", "p1", "p7"], k=20, groups=group, n_groups=2)
    check(host(res), cut(want, 20, [7, 1, 7]), "dict")
    got = top_nodes(x, [], k=3)
    assert got[0].shape == (0, 1, 3) and got[2].shape == (0, 1)
    with pytest.raises(ValueError, match=r"top_nodes: groups\[0\] = 5 is outside \[-1, G=2\)"):
        top_nodes(x[:, :k], groups=torch.full((n,), 5, dtype=torch.int32, device="cuda"), n_groups=2)
    idx, _, cnt = res
    shared = top_overlap(idx, cnt, [0, 0, 1], torch.tensor([2, 1, 1], device="cuda"))
    assert shared.is_cuda and shared.dtype == torch.int32
    assert np.array_equal(shared.cpu().numpy(), T.expected_overlap(*cut(want, 20, [7, 1, 7])[::2], [0, 0, 1], [2, 1, 1]))
    assert np.array_equal(shared[0].cpu().numpy(), cnt[0].cpu().numpy())          # p7 with p7
    assert top_overlap(idx, cnt, [], []).shape == (0, 2)
