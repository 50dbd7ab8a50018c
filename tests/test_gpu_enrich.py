"""GPU: csrc/enrich.hip (gss_profile_order, gss_enrich_lists, gss_enrich_random) through enrich.profile_order / enrichment_scores /
random_enrichment_scores, against the numpy mirror (enrich_mirror.py): equality, no tolerance.

Orders and permutations are integers.  The scores are fp64 whose every operation the header states and the mirror repeats one rounding at a
time (test_enrich_mirror.py holds the mirror to an exact rational walk), so the device's scores equal the mirror's bit for bit, and hence
each other under every regrouping of a call and between the two entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import enrich_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd import enrich as E  # noqa: E402

pytestmark = pytest.mark.gpu

ORDER_COLS = [3, 0, 6, 0, 5, 1, 2, 4]      # out of order, with a repeat
_PROFILES = {}
_ORDERS = {}


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((np.isnan(a) & np.isnan(b)) | (a.view(np.int64) == b.view(np.int64))))


def profiles(m_places):
    """seven profiles over n > m_places nodes and a scattered universe -> (host [n][7], universe, device view [n][7] with a row stride of
    9); made once per size and never written.  Columns: 0 distinct, 1 all equal, 2 heavy ties with +-0.0, 3 with +-inf, 4 subnormals, 5 a NaN
    inside the universe, 6 a NaN outside it only"""
    if m_places not in _PROFILES:
        rng = np.random.RandomState(100 + m_places)
        n = m_places + max(3, m_places // 7)
        universe = np.sort(rng.permutation(n)[:m_places]).astype(np.int32)
        outside = np.setdiff1d(np.arange(n), universe)
        h = np.empty((n, 7))
        h[:, 0] = rng.randn(n)
        h[:, 1] = 0.375
        h[:, 2] = rng.randint(-2, 3, n) * 0.25
        h[rng.rand(n) < 0.5, 2] *= -1.0                                  # -0.0 beside +0.0
        h[:, 3] = rng.randn(n)
        h[rng.rand(n) < 0.2, 3] = np.inf
        h[rng.rand(n) < 0.2, 3] = -np.inf
        h[:, 4] = rng.randint(-40, 41, n) * 5e-324
        h[:, 5] = rng.rand(n)
        h[universe[m_places // 2], 5] = np.nan
        h[:, 6] = rng.rand(n)
        h[outside, 6] = np.nan
        base = torch.zeros(n, 9, dtype=torch.float64, device="cuda")
        view = base[:, :7]
        view.copy_(torch.from_numpy(h))
        _PROFILES[m_places] = (h, universe, view)
    return _PROFILES[m_places]


def scored_order(m_places):
    """an Order of three columns over m_places places -> (Order, pos host [3][M], w host [3][M]): 0 heavy-tailed and distinct, 1 half
    zeros with ties, 2 flagged by a NaN; made once per size"""
    if m_places not in _ORDERS:
        rng = np.random.RandomState(200 + m_places)
        h = np.empty((3, m_places))
        h[0] = np.exp(3 * rng.randn(m_places))
        h[1] = np.round(rng.rand(m_places) * 8) / 8 * (np.arange(m_places) % 2)
        h[2] = rng.rand(m_places)
        h[2, m_places - 1] = np.nan
        order = E.profile_order(h, None, np.arange(m_places))
        pos, w = host(order.pos), host(order.w)
        for j in range(3):
            want_pos, want_w = M.order(h[j], np.arange(m_places))
            assert np.array_equal(pos[j], want_pos) and same_bits(w[j], want_w)
        _ORDERS[m_places] = (order, pos, w)
    return _ORDERS[m_places]


def mirror_scores(pos, w, sets, weighted):
    both = [[M.es_peak(pos[j], w[j], s, weighted) for s in sets] for j in range(len(pos))]
    es = np.array([[b[0] for b in row] for row in both], dtype=np.float64).reshape(len(pos), len(sets))
    peak = np.array([[b[1] for b in row] for row in both], dtype=np.int32).reshape(len(pos), len(sets))
    return es, peak


# ---- gss_profile_order ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m_places", (2, 3, 63, 64, 65, 4097, 20000))
def test_order_equals_the_mirror(m_places):
    h, universe, view = profiles(m_places)
    assert view.stride(0) == 9 and h.shape[0] > m_places
    order = E.profile_order(view, ORDER_COLS, universe)
    pos, w = host(order.pos), host(order.w)
    assert pos.shape == w.shape == (len(ORDER_COLS), m_places)
    for j, c in enumerate(ORDER_COLS):
        want_pos, want_w = M.order(h[:, c], universe)
        assert np.array_equal(pos[j], want_pos), (m_places, c)
        assert same_bits(w[j], want_w), (m_places, c)
    assert (pos[ORDER_COLS.index(5)] == -1).all() and np.isnan(w[ORDER_COLS.index(5)]).all()            # the NaN inside the universe flags
    assert sorted(pos[ORDER_COLS.index(6)].tolist()) == list(range(m_places))                           # the NaN outside changes nothing
    assert pos[ORDER_COLS.index(1)].tolist() == list(range(m_places))                                   # all equal: the places' own order
    assert np.array_equal(pos[1], pos[3]) and same_bits(w[1], w[3])                                      # the repeated column
    alone = E.profile_order(view, [2], universe)                                                         # a column alone: the same bits
    assert torch.equal(alone.pos[0], order.pos[ORDER_COLS.index(2)]) and same_bits(host(alone.w[0]), w[ORDER_COLS.index(2)])
    every = E.profile_order(h.T.copy(), None, universe)                                                  # a host array [K][N], cols = None
    assert torch.equal(every.pos[0], order.pos[1])


# ---- gss_enrich_lists ----------------------------------------------------------------------------------------------------------------

def check_sets(m_places, sets):
    order, pos, w = scored_order(m_places)
    for weighted in (True, False):
        es, peak = E.enrichment_scores(order, sets, weighted)
        want_es, want_peak = mirror_scores(pos, w, sets, weighted)
        assert same_bits(host(es), want_es), (m_places, weighted)
        assert np.array_equal(host(peak), want_peak), (m_places, weighted)
        assert np.isnan(host(es)[2]).all() and (host(peak)[2] == -1).all()                               # the flagged column
    return order, pos, w


def test_list_scores_equal_the_mirror_at_every_size():
    m_places = 2000
    order, pos, w = scored_order(m_places)
    rng = np.random.RandomState(7)
    by_pos = np.argsort(pos[0])
    sets = [rng.permutation(m_places)[:s] for s in (1, 2, 63, 64, 65, 1023, 1024)]
    sets += [[by_pos[0]], [by_pos[-1]], [by_pos[0], by_pos[-1]], list(by_pos[[0, 5, 77, m_places - 1]])]   # the first and the last position
    check_sets(m_places, sets)
    # the exact anchors: the top s, the bottom s, and members that all weigh nothing
    for s in (1, 64, 1024):
        es, peak = E.enrichment_scores(order, [by_pos[:s], by_pos[::-1][:s]], True)
        assert host(es)[0].tolist() == [1.0, -1.0] and host(peak)[0].tolist() == [s - 1, 0]
        es, peak = E.enrichment_scores(order, [by_pos[:s], by_pos[::-1][:s]], False)
        assert host(es)[0].tolist() == [1.0, -1.0] and host(peak)[0].tolist() == [s - 1, 0]
    zeros = np.flatnonzero(w[1] == 0.0)[:40]
    assert len(zeros) == 40
    es, peak = E.enrichment_scores(order, [zeros], True)
    assert np.isnan(host(es)[1, 0]) and host(peak)[1, 0] == -1 and np.isfinite(host(es)[0, 0])
    es, peak = E.enrichment_scores(order, [zeros], False)
    assert np.isfinite(host(es)[1, 0]) and host(peak)[1, 0] >= 0


@pytest.mark.parametrize("m_places", (2, 65, 1025))
def test_list_scores_of_all_but_one_place(m_places):
    rng = np.random.RandomState(m_places)
    sets = [np.delete(np.arange(m_places), k) for k in sorted({0, m_places // 2, m_places - 1})]
    sets += [rng.permutation(m_places)[:m_places - 1], [0], [m_places - 1]]
    check_sets(m_places, sets)


def test_a_set_alone_and_among_others_and_no_set():
    m_places = 1025
    order, pos, w = scored_order(m_places)
    rng = np.random.RandomState(8)
    sets = [rng.permutation(m_places)[:rng.randint(1, 200)] for _ in range(300)]
    every_es, every_peak = E.enrichment_scores(order, sets)
    again_es, again_peak = E.enrichment_scores(order, sets)
    assert same_bits(host(every_es), host(again_es)) and torch.equal(every_peak, again_peak)             # run to run
    for c in (0, 1, 150, 299):
        es, peak = E.enrichment_scores(order, [sets[c]])
        assert same_bits(host(es)[:, 0], host(every_es)[:, c]) and torch.equal(peak[:, 0], every_peak[:, c]), c
        es, peak = E.enrichment_scores(order, [sets[c][::-1]])                                           # the list's order does not matter
        assert same_bits(host(es)[:, 0], host(every_es)[:, c]) and torch.equal(peak[:, 0], every_peak[:, c]), c
    one = E.Order(order.pos[:1].contiguous(), order.w[:1].contiguous(), order.universe)                  # a column alone
    es, peak = E.enrichment_scores(one, sets)
    assert same_bits(host(es)[0], host(every_es)[0]) and torch.equal(peak[0], every_peak[0])
    es, peak = E.enrichment_scores(order, [])                                                            # C = 0
    assert es.shape == (3, 0) and peak.shape == (3, 0)
    lib = _lib.load()
    assert lib.gss_enrich_lists(m_places, 3, order.pos.data_ptr(), order.w.data_ptr(), 1, 0, 0, 0, 0, 0, _lib.current_stream()) == 0
    assert lib.gss_enrich_lists(m_places, 0, 0, 0, 1, 5, 0, 0, 0, 0, _lib.current_stream()) == 0         # nc = 0


# ---- gss_enrich_random ---------------------------------------------------------------------------------------------------------------

def size_lists(m_places):
    top = min(1024, m_places - 1)
    lists = [[1], [m for m in (1, 2, 3) if m <= top], sorted({m for m in (1, 2, 3, 5, 17, 63, 64, 65, 300, 1023, 1024) if m <= top} | {top})]
    return [s for k, s in enumerate(lists) if s not in lists[:k]]


def check_random(m_places, sizes, seed, s0, P, weighted=True):
    order, pos, w = scored_order(m_places)
    es, perm = E.random_enrichment_scores(order, sizes, P, seed=seed, first=s0, perms=True, weighted=weighted)
    es, perm = host(es), host(perm)
    assert es.shape == (3, P, len(sizes)) and perm.shape == (P, sizes[-1])
    for s in range(P):
        assert np.array_equal(perm[s], M.permutation(seed, s0 + s, m_places)[:sizes[-1]]), (m_places, seed, s0 + s)
    for j in range(3):
        want, _ = M.random_scores(pos[j], w[j], sizes, seed, s0, P, weighted)
        assert same_bits(es[j], want), (m_places, sizes, j)
    sets = [perm[s][:m] for s in range(P) for m in sizes]                                                # the lists' entry point on the prefixes
    by_list, _ = E.enrichment_scores(order, sets, weighted)
    assert same_bits(host(by_list).reshape(3, P, len(sizes)), es), (m_places, sizes)
    return es


@pytest.mark.parametrize("m_places", (2, 3, 65, 1000, 2048, 2049, 20000))
def test_random_scores_equal_the_mirror_and_the_lists(m_places):
    for k, sizes in enumerate(size_lists(m_places)):
        check_random(m_places, sizes, seed=(0, 2 ** 63 + 5, 9)[k % 3], s0=(0, 12345, 7)[k % 3], P=3)
    check_random(m_places, size_lists(m_places)[-1], seed=4, s0=2 ** 31 - 2, P=2, weighted=False)         # the last sample numbers, unweighted


@pytest.mark.parametrize("m_places, sizes, seed, sample", ((2049, [1], 0, 1665), (20000, [1, 17, 64], 3, 6)))
def test_a_sample_whose_first_threshold_collects_too_few_keys(m_places, sizes, seed, sample):
    """the selection's second round: on the host, fewer than kmax of the sample's keys lie under the first threshold; the prefix and the
    scores are those of the permutation all the same"""
    assert M.first_threshold_count(seed, sample, m_places, sizes[-1]) < sizes[-1]
    assert M.first_threshold_count(seed, sample + 1, m_places, sizes[-1]) >= sizes[-1]
    check_random(m_places, sizes, seed, sample, P=2)


def test_random_scores_do_not_depend_on_how_a_call_is_cut():
    m_places = 1000
    order, pos, w = scored_order(m_places)
    sizes = [1, 2, 17, 64, 65, 300]
    whole = E.random_enrichment_scores(order, sizes, 7, seed=9, first=40)
    assert same_bits(host(whole), host(E.random_enrichment_scores(order, sizes, 7, seed=9, first=40)))  # run to run
    parts = [E.random_enrichment_scores(order, sizes, c, seed=9, first=40 + f) for f, c in ((0, 3), (3, 4))]
    assert same_bits(host(torch.cat(parts, dim=1)), host(whole))                                         # P = 7 equals 3 + 4 through `first`
    for k, m in enumerate(sizes):                                                                        # a size alone
        alone = E.random_enrichment_scores(order, [m], 7, seed=9, first=40)
        assert same_bits(host(alone)[:, :, 0], host(whole)[:, :, k]), m
    # nc = 1 against the same column among 5
    five = E.Order(order.pos[[1, 0, 2, 0, 1]].contiguous(), order.w[[1, 0, 2, 0, 1]].contiguous(), order.universe)
    among = host(E.random_enrichment_scores(five, sizes, 7, seed=9, first=40))
    for at, j in enumerate((1, 0, 2, 0, 1)):
        one = E.Order(order.pos[j:j + 1].contiguous(), order.w[j:j + 1].contiguous(), order.universe)
        assert same_bits(host(E.random_enrichment_scores(one, sizes, 7, seed=9, first=40))[0], among[at]), at
        assert same_bits(among[at], host(whole)[j])
    assert E.null_scores(order, sizes, 7, seed=9).shape == (3, 7, len(sizes))
    assert same_bits(E.null_scores(order, sizes, 47, seed=9)[:, 40:], host(E.random_enrichment_scores(order, sizes, 7, seed=9, first=40)))


def test_enrichment_equals_its_parts_and_finds_a_planted_set():
    rng = np.random.RandomState(12)
    n = 400
    universe = np.arange(0, n, 2)
    x = rng.rand(n)
    planted = [5, 17, 40, 41, 99, 150]
    x[universe[planted]] += 2.0                                                                          # the set sits at the top
    sets = {"planted": planted, "random": [3, 60, 61, 120, 180, 199], "few": [7, 8]}
    rec, sizes, null = E.enrichment({"a": x}, ["a"], universe, sets, 199, seed=2, return_null=True)
    assert sizes == [2, 6] and null.shape == (1, 199, 2) and [r["set"] for r in rec] == list(sets)
    order = E.profile_order({"a": x}, ["a"], universe)
    assert same_bits(null, host(E.random_enrichment_scores(order, sizes, 199, seed=2)))
    es, peak = (host(t)[0] for t in E.enrichment_scores(order, list(sets.values())))
    want = M.stats(es, peak, list(sets.values()), host(order.pos)[0], sizes, null[0])
    for r, e, pk, m in zip(rec, es, peak, want):
        assert r["es"] == e and r["peak"] == pk and r["profile"] == "a"
        assert all(r[k] == m[k] or (r[k] != r[k] and m[k] != m[k]) for k in m)
    assert rec[0]["es"] == 1.0 and rec[0]["p"] == 1 / (1 + rec[0]["n_same"]) < 0.02 and rec[0]["lead"] == sorted(planted, key=lambda u: -x[universe[u]])
    assert rec[1]["p"] > 0.05


# ---- refusals: by name, outputs untouched ----------------------------------------------------------------------------------------------

def refused(rc, words):
    text = _lib.load().gss_last_error().decode()
    assert rc == -22 and words in text, (rc, text)


def test_profile_order_refusals():
    lib, st = _lib.load(), _lib.current_stream()
    n, m_places = 40, 10
    x = torch.rand(n, 4, dtype=torch.float64, device="cuda")
    uni = torch.arange(0, 20, 2, dtype=torch.int32, device="cuda")
    cols = torch.tensor([1, 3], dtype=torch.int32, device="cuda")
    pos = torch.full((2, m_places), -7, dtype=torch.int32, device="cuda")
    w = torch.full((2, m_places), -7.0, dtype=torch.float64, device="cuda")
    need = lib.gss_profile_order_workspace_bytes(m_places, 2)
    assert need == 256 + 2 * m_places * 8 and lib.gss_profile_order_workspace_bytes(1, 2) == 0 and lib.gss_profile_order_workspace_bytes(65537, 1) == 0
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")

    def call(n=n, x=x, ld=4, nc=2, cols=cols, m=m_places, uni=uni, pos=pos, w=w, ws=ws.data_ptr(), ws_bytes=need):
        return lib.gss_profile_order(n, _lib.ptr(x), ld, nc, _lib.ptr(cols), m, _lib.ptr(uni), _lib.ptr(pos), _lib.ptr(w), ws, ws_bytes, st)

    refused(call(n=0), "profile_order: n=0 rows is outside [1, 16777216]")
    refused(call(n=2 ** 24 + 1), "profile_order: n=16777217 rows is outside [1, 16777216]")
    refused(call(m=1), "profile_order: M=1 places is outside [2, min(n, 65536) = 40]")
    refused(call(m=41), "profile_order: M=41 places is outside [2, min(n, 65536) = 40]")
    refused(call(n=70000, m=65537), "profile_order: M=65537 places is outside [2, min(n, 65536) = 65536]")
    refused(call(nc=-1), "profile_order: nc=-1 columns is outside")
    refused(call(ld=0), "profile_order: ld=0 must be >= 1")
    refused(call(uni=None), "profile_order: universe is null")
    refused(call(ws=0), "profile_order: workspace is null")
    refused(call(ws=ws.data_ptr() + 4), "profile_order: workspace is not 8-byte aligned")
    refused(call(ws_bytes=need - 1), f"profile_order: workspace of {need - 1} bytes is below the {need} that M=10, nc=2 need")
    refused(call(x=None), "profile_order: x is null")
    refused(call(pos=None), "profile_order: pos_out is null")
    refused(call(w=None), "profile_order: w_out is null")
    refused(lib.gss_profile_order(n, x.data_ptr(), 4, 2, cols.data_ptr(), m_places, uni.data_ptr(), pos.data_ptr() + 2, w.data_ptr(), ws.data_ptr(),
                                  need, st), "profile_order: pos_out is not 4-byte aligned")
    refused(lib.gss_profile_order(n, x.data_ptr(), 4, 2, cols.data_ptr(), m_places, uni.data_ptr(), pos.data_ptr(), w.data_ptr() + 4, ws.data_ptr(),
                                  need, st), "profile_order: w_out is not 8-byte aligned")
    refused(call(cols=None, ld=1), "profile_order: ld=1 is below nc=2 (cols is null: columns 0 .. nc - 1)")
    for bad, words in (([0, 2, 4, 6, 40, 42, 44, 46, 48, 50], "universe[4] = 40 is outside [0, n=40)"),
                       ([-1, 2, 4, 6, 8, 10, 12, 14, 16, 18], "universe[0] = -1 is outside [0, n=40)"),
                       ([0, 2, 4, 4, 8, 10, 12, 14, 16, 18], "universe[3] = 4 is not above universe[2] = 4"),
                       ([0, 2, 4, 6, 8, 10, 12, 14, 39, 18], "universe[9] = 18 is not above universe[8] = 39")):
        refused(call(uni=torch.tensor(bad, dtype=torch.int32, device="cuda")), "profile_order: " + words)
    refused(call(cols=torch.tensor([1, 4], dtype=torch.int32, device="cuda")), "profile_order: cols[1] = 4 is outside [0, ld=4)")
    refused(call(cols=torch.tensor([-1, 2], dtype=torch.int32, device="cuda")), "profile_order: cols[0] = -1 is outside [0, ld=4)")
    torch.cuda.synchronize()
    assert (host(pos) == -7).all() and (host(w) == -7.0).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert sorted(host(pos)[0].tolist()) == list(range(m_places))
    with pytest.raises(_lib.GssError, match=r"universe\[1\] = 3 is not above universe\[0\] = 3"):
        E.profile_order(x, [0], [3, 3])
    with pytest.raises(ValueError, match=r"profile_order: column index 4 is outside \[0, 4\)"):
        E.profile_order(x, [4], [1, 3])


def test_enrich_lists_refusals():
    m_places = 65
    order, pos, w = scored_order(m_places)
    for sets, words in (([[1, 2], []], r"enrich_lists: list 1 has 0 places, outside \[1, min\(1024, M - 1\) = 64\]"),
                        ([[1], list(range(65))], r"enrich_lists: list 1 has 65 places, outside \[1, min\(1024, M - 1\) = 64\]"),
                        ([[1, 2, 3], [0, 65, 4]], r"enrich_lists: list 1: idx\[1\] = 65 is outside \[0, M=65\)"),
                        ([[-1, 2]], r"enrich_lists: list 0: idx\[0\] = -1 is outside \[0, M=65\)"),
                        ([[1, 2, 3], [4, 9, 5, 9, 4]], r"enrich_lists: list 1: idx\[4\] = 4 repeats a place of the list"),
                        ([[7, 7], [4, 66]], r"enrich_lists: list 0: idx\[1\] = 7 repeats a place of the list")):
        with pytest.raises(_lib.GssError, match=words):
            E.enrichment_scores(order, sets)
    big, _, _ = scored_order(2000)
    with pytest.raises(_lib.GssError, match=r"enrich_lists: list 0 has 1025 places, outside \[1, min\(1024, M - 1\) = 1024\]"):
        E.enrichment_scores(big, [list(range(1025))])
    lib, st = _lib.load(), _lib.current_stream()
    idx = torch.arange(10, dtype=torch.int32, device="cuda")
    es = torch.full((3, 2), -7.0, dtype=torch.float64, device="cuda")
    peak = torch.full((3, 2), -7, dtype=torch.int32, device="cuda")

    def call(ptr, m=m_places, nc=3, weighted=1, C=2, pos=order.pos, es=es):
        d_ptr = torch.tensor(ptr, dtype=torch.int32, device="cuda")
        return lib.gss_enrich_lists(m, nc, _lib.ptr(pos), order.w.data_ptr(), weighted, C, d_ptr.data_ptr(), idx.data_ptr(), _lib.ptr(es),
                                    peak.data_ptr(), st)

    refused(call([1, 4, 10]), "enrich_lists: ptr[0] = 1 must be 0")
    refused(call([0, 6, 4]), "enrich_lists: ptr[2] = 4 is below ptr[1] = 6")
    refused(call([0, 4, 10], m=1), "enrich_lists: M=1 places is outside [2, 65536]")
    refused(call([0, 4, 10], m=65537), "enrich_lists: M=65537 places is outside [2, 65536]")
    refused(call([0, 4, 10], nc=-1), "enrich_lists: nc=-1 columns must be >= 0")
    refused(call([0, 4, 10], weighted=2), "enrich_lists: weighted=2 must be 0 or 1")
    refused(call([0, 4, 10], C=-1), "enrich_lists: C=-1 lists must be >= 0")
    refused(call([0, 4, 10], pos=None), "enrich_lists: pos is null")
    refused(call([0, 4, 10], es=None), "enrich_lists: es_out is null")
    torch.cuda.synchronize()
    assert (host(es) == -7.0).all() and (host(peak) == -7).all()
    assert call([0, 4, 10]) == 0
    torch.cuda.synchronize()
    assert np.isfinite(host(es)[:2]).all()


def test_enrich_random_refusals():
    order, pos, w = scored_order(65)
    for kw, words in ((dict(sizes=[3, 3]), r"enrich_random: sizes\[1\] = 3 is not above sizes\[0\] = 3"),
                      (dict(sizes=[5, 4]), r"enrich_random: sizes\[1\] = 4 is not above sizes\[0\] = 5"),
                      (dict(sizes=[0]), r"enrich_random: sizes\[0\] = 0 is outside \[1, min\(1024, M - 1\) = 64\]"),
                      (dict(sizes=[65]), r"enrich_random: sizes\[0\] = 65 is outside \[1, min\(1024, M - 1\) = 64\]"),
                      (dict(sizes=[]), r"enrich_random: n_sizes=0 is outside \[1, min\(1024, M - 1\) = 64\]"),
                      (dict(samples=0), r"enrich_random: P=0 samples must be >= 1"),
                      (dict(first=-1), r"enrich_random: samples s0=-1 "),
                      (dict(samples=2, first=2 ** 31 - 1), r"are outside \[0, 2\^31\]")):
        args = dict(sizes=[2], samples=1)
        args.update(kw)
        with pytest.raises(_lib.GssError, match=words):
            E.random_enrichment_scores(order, **args)
    big, _, _ = scored_order(2000)
    with pytest.raises(_lib.GssError, match=r"enrich_random: sizes\[1\] = 1025 is outside \[1, min\(1024, M - 1\) = 1024\]"):
        E.random_enrichment_scores(big, [5, 1025], 1)
    lib, st = _lib.load(), _lib.current_stream()
    sizes = torch.tensor([2, 2], dtype=torch.int32, device="cuda")
    es = torch.full((3, 1, 2), -7.0, dtype=torch.float64, device="cuda")
    perm = torch.full((1, 2), -7, dtype=torch.int32, device="cuda")
    refused(lib.gss_enrich_random(65, 3, order.pos.data_ptr(), order.w.data_ptr(), 1, ctypes.c_uint64(0), 0, 1, 2, sizes.data_ptr(), es.data_ptr(),
                                  perm.data_ptr(), st), "enrich_random: sizes[1] = 2 is not above sizes[0] = 2")
    refused(lib.gss_enrich_random(1, 3, order.pos.data_ptr(), order.w.data_ptr(), 1, ctypes.c_uint64(0), 0, 1, 1, sizes.data_ptr(), es.data_ptr(),
                                  perm.data_ptr(), st), "enrich_random: M=1 places is outside [2, 65536]")
    refused(lib.gss_enrich_random(65, 3, order.pos.data_ptr(), order.w.data_ptr(), 1, ctypes.c_uint64(0), 0, 1, 1, 0, es.data_ptr(),
                                  perm.data_ptr(), st), "enrich_random: sizes is null")
    refused(lib.gss_enrich_random(65, 3, order.pos.data_ptr(), order.w.data_ptr(), 1, ctypes.c_uint64(0), 0, 1, 1, sizes.data_ptr(), 0,
                                  perm.data_ptr(), st), "enrich_random: es_out is null")
    torch.cuda.synchronize()
    assert (host(es) == -7.0).all() and (host(perm) == -7).all()
    with pytest.raises(ValueError, match="order must be what profile_order returned"):
        E.random_enrichment_scores((order.pos, order.w), [2], 1)
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        E.profile_order(np.zeros((1, 4)), None, [0, 1], device="cpu")
