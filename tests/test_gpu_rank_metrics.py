"""GPU: csrc/rank_metrics.hip (gss_rank_metrics_rows) against its host mirror (rank_metrics_mirror.py), gss_auc_rows and sklearn.
For every case: auc bit-equal to gss_auc_rows on the same inputs; hits bit-equal to the mirror; ap bit-equal to the mirror's statement of
the kernel's order of additions (M.ap_ordered) and within (P + 3) 2^-53 relative of the mirror's exactly rounded value (any order of
summing P positive, correctly rounded terms, plus the final division); ap within 1e-12
absolute of sklearn.metrics.average_precision_score where C <= 1,661 (test_gpu_auc.py's tolerance for the same library; the derived
4 C 2^-53 is 7.4e-13 at that width).  Then order independence, one-class rows, nk = 0 and the refusals by name."""
import os
import sys

import numpy as np
import pytest
import torch
from sklearn.metrics import average_precision_score

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_metrics_mirror as M  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_COLS = 16384


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def device_metrics(scores, rows, ks, workspace_bytes=None):
    """scores [R, C] fp64 host, rows: per row the positive columns, ks: cut-offs -> (rc, auc, ap, hits [R, nk], n_pos, n_neg, error text)"""
    lib = _lib.load()
    s = np.ascontiguousarray(scores, dtype=np.float64)
    ptr, col = M.csr(rows)
    col = np.concatenate([col, np.zeros(1, np.int32)])
    dev = torch.device("cuda")
    d_s, d_ptr, d_col = (torch.from_numpy(a).to(dev) for a in (s, ptr, col))
    R, Cn = s.shape
    nk = len(ks)
    h_ks = np.asarray(list(ks) + [0], dtype=np.int32)
    auc = torch.empty(R, dtype=torch.float64, device=dev)
    ap = torch.empty(R, dtype=torch.float64, device=dev)
    hits = torch.full((R, max(nk, 1)), -7.0, dtype=torch.float64, device=dev)
    n_pos = torch.empty(R, dtype=torch.int32, device=dev)
    n_neg = torch.empty(R, dtype=torch.int32, device=dev)
    need = lib.gss_rank_metrics_workspace_bytes(R, Cn)
    assert need == 8 * R * Cn
    nbytes = need if workspace_bytes is None else workspace_bytes
    ws = torch.empty(max(need, 8) // 8, dtype=torch.int64, device=dev)
    rc = lib.gss_rank_metrics_rows(R, Cn, _lib.ptr(d_s), Cn, _lib.ptr(d_ptr), _lib.ptr(d_col), nk, h_ks.ctypes.data, _lib.ptr(auc),
                                   _lib.ptr(ap), _lib.ptr(hits), _lib.ptr(n_pos), _lib.ptr(n_neg), _lib.ptr(ws), nbytes,
                                   _lib.current_stream())
    msg = lib.gss_last_error().decode(errors="replace")
    return rc, auc.cpu().numpy(), ap.cpu().numpy(), hits.cpu().numpy()[:, :nk], n_pos.cpu().numpy(), n_neg.cpu().numpy(), msg


def device_aucs(scores, rows):
    lib = _lib.load()
    s = np.ascontiguousarray(scores, dtype=np.float64)
    ptr, col = M.csr(rows)
    col = np.concatenate([col, np.zeros(1, np.int32)])
    d_s, d_ptr, d_col = (torch.from_numpy(a).cuda() for a in (s, ptr, col))
    R, Cn = s.shape
    auc = torch.empty(R, dtype=torch.float64, device="cuda")
    cnt = torch.empty(2 * R, dtype=torch.int32, device="cuda")
    rc = lib.gss_auc_rows(R, Cn, _lib.ptr(d_s), Cn, _lib.ptr(d_ptr), _lib.ptr(d_col), _lib.ptr(auc), _lib.ptr(cnt), _lib.ptr(cnt[R:]),
                          _lib.current_stream())
    assert rc == 0, lib.gss_last_error()
    return auc.cpu().numpy()


def seeded_rows(rng, R, Cn, max_pos):
    return [np.sort(rng.choice(Cn, rng.randint(1, max_pos + 1), replace=False)) for _ in range(R)]


def check(scores, rows, ks):
    """the comparisons of the module docstring -> the device outputs"""
    scores = np.asarray(scores, np.float64)
    rc, auc, ap, hits, n_pos, n_neg, msg = device_metrics(scores, rows, ks)
    assert rc == 0, msg
    C = scores.shape[1]
    ptr, col = M.csr(rows)
    m_auc, m_ap, m_hits, m_pos, m_neg = M.mirror_metrics(scores, ptr, col, ks)
    assert np.array_equal(n_pos, m_pos) and np.array_equal(n_neg, m_neg)
    assert np.array_equal(_bits(auc), _bits(device_aucs(scores, rows)))
    assert np.array_equal(_bits(auc), _bits(m_auc))
    assert hits.shape == m_hits.shape and np.array_equal(_bits(hits), _bits(m_hits)), (hits[hits != m_hits], m_hits[hits != m_hits])
    worst = 0.0
    for r, cols in enumerate(rows):
        P = len(cols)
        bound = (P + 3) * 2.0 ** -53 * m_ap[r]
        worst = max(worst, abs(ap[r] - m_ap[r]) / bound)
        assert abs(ap[r] - m_ap[r]) <= bound, (r, P, ap[r], m_ap[r])
        mask = np.zeros(C, bool)
        mask[cols] = True
        ordered = M.ap_ordered_row(scores[r], mask)
        assert _bits(ap[r:r + 1])[0] == _bits([ordered])[0], (r, P, ap[r], ordered)
        if C <= 1661:
            y = np.zeros(C, int)
            y[cols] = 1
            want = average_precision_score(y, scores[r])
            assert abs(ap[r] - want) <= 1e-12, (r, ap[r], want)
    print(f"C={C}: worst |ap - mirror| / ((P + 3) 2^-53 ap) = {worst:.3f}")
    return auc, ap, hits, n_pos, n_neg


def heavy_ties(rng, R, C):
    """test_gpu_auc.py's test_heavy_ties_and_signed_zeros generator: a handful of levels, mixed signed zeros"""
    s = np.round(rng.randn(R, C), 0) * 0.5
    s[s == 0] = np.where(rng.rand(int((s == 0).sum())) < 0.5, -0.0, 0.0)
    assert np.any(np.signbit(s) & (s == 0)) and np.any(~np.signbit(s) & (s == 0))
    return s


def test_two_columns_tied_and_untied():
    check(np.array([[0.3, 0.3], [1.0, -1.0], [1.0, -1.0], [0.0, -0.0]]), [[0], [1], [0], [1]], (1, 2, 3))


@pytest.mark.parametrize("C", [64, 65])
def test_across_the_minimum_pad(C):
    rng = np.random.RandomState(C)
    s = np.concatenate([rng.randn(6, C), np.round(rng.randn(6, C), 0)])
    rows = seeded_rows(rng, 11, C, C - 1) + [list(range(C - 1))]
    check(s, rows, (1, 5, 63, 64, 65, 66))


def test_heavy_ties_and_signed_zeros_with_cuts_inside_and_at_the_end_of_groups():
    rng = np.random.RandomState(1)
    s = heavy_ties(rng, 64, 1661)
    rows = seeded_rows(rng, 64, 1661, 40)
    ks = (1, 10, 50, 1661, 5000)
    # the cases the cut-offs are there for, found on the inputs themselves: a cut inside a tie group, a cut on a group's last member
    inside = last = 0
    for r in range(64):
        mask = np.zeros(1661, bool)
        mask[rows[r]] = True
        for k in ks[:3]:
            _, _, slots, g = M.hits_parts(s[r], mask, k)
            inside += slots < g
            last += slots == g and g > 1
    k_last = int((s[7] >= 0.5).sum())                           # row 7, the sixth cut: the last member of the group at 0.5
    ks = ks + (k_last,)
    mask = np.zeros(1661, bool)
    mask[rows[7]] = True
    parts = M.hits_parts(s[7], mask, k_last)
    assert parts[2] == parts[3] > 1 and inside > 0
    auc, ap, hits, n_pos, _ = check(s, rows, ks)
    assert np.array_equal(hits[:, 3], n_pos.astype(np.float64)) and np.array_equal(_bits(hits[:, 3]), _bits(hits[:, 4]))   # k = C and k > C
    print(f"cuts inside a group: {inside}, on a group's last member: {last + 1}")


@pytest.mark.parametrize("C", M.RANK_IDENTITY_WIDTHS)
def test_the_three_entry_points_share_one_ordering(C):
    """gss_profile_rank on the transposed scores, the identity of M.auc_from_ranks on its ranks: the bits of auc from gss_auc_rows and from
    gss_rank_metrics_rows.  Each kernel is otherwise compared with its own mirror only"""
    s, rows = M.tied_rows(C)
    R = len(rows)
    lib = _lib.load()
    x = torch.from_numpy(s).cuda().t().contiguous()                            # [C, R]: row r of the scores is profile column r
    ranks = torch.empty(C, R, dtype=torch.float64, device="cuda")
    need = int(lib.gss_profile_rank_workspace_bytes(C, R))
    ws = torch.empty((need + 7) // 8, dtype=torch.int64, device="cuda")
    rc = lib.gss_profile_rank(C, _lib.ptr(x), R, R, None, _lib.ptr(ranks), R, _lib.ptr(ws), need, _lib.current_stream())
    assert rc == 0, lib.gss_last_error()
    torch.cuda.synchronize()
    ranks = ranks.cpu().numpy()
    got = np.array([M.auc_from_ranks(ranks[:, r], rows[r]) for r in range(R)])
    rc, auc, *_, msg = device_metrics(s, rows, ())
    assert rc == 0, msg
    assert np.array_equal(_bits(got), _bits(device_aucs(s, rows))) and np.array_equal(_bits(got), _bits(auc)), (got, auc)


def test_single_positive_and_single_negative():
    rng = np.random.RandomState(2)
    s = rng.randn(8, 1661)
    s[1] = np.round(s[1], 0)
    s[5] = np.round(s[5], 0)
    rows = [[5]] * 4 + [[c for c in range(1661) if c != k] for k in (0, 7, 1000, 1660)]
    check(s, rows, (1, 50, 1660, 1661))


def test_msi_width():
    rng = np.random.RandomState(3)
    check(rng.randn(96, 1661), seeded_rows(rng, 96, 1661, 30), (10, 50))


def test_the_column_limit_and_a_row_of_mostly_positives():
    rng = np.random.RandomState(3)
    s = np.round(rng.randn(7, MAX_COLS), 3)
    rows = seeded_rows(rng, 6, MAX_COLS, 4000) + [np.sort(rng.choice(MAX_COLS, 12000, replace=False))]
    s[5] = np.round(s[5], 1)
    assert len(rows[6]) == 12000
    check(s, rows, (1, 50, 4000, 16383, 16384, 20000, 12000, 8192))


def test_permuted_columns_and_lists_give_bitwise_equal_results():
    rng = np.random.RandomState(5)
    s = np.round(rng.randn(32, 1661), 1)
    rows = seeded_rows(rng, 32, 1661, 50)
    ks = (1, 10, 50, 400)
    a = check(s, rows, ks)
    perm = rng.permutation(1661)
    inv = np.argsort(perm)
    moved = [np.asarray([inv[c] for c in r]) for r in rows]
    for lists in ([m[::-1] for m in moved], [rng.permutation(m) for m in moved]):
        rc, *b, msg = device_metrics(s[:, perm], lists, ks)
        assert rc == 0, msg
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    rc, *again, msg = device_metrics(s, rows, ks)                # run to run
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, again))


def test_one_class_rows_are_nan_with_their_counts():
    s = np.random.RandomState(4).randn(3, 10)
    rc, auc, ap, hits, n_pos, n_neg, msg = device_metrics(s, [[], list(range(10)), [2, 3]], (1, 3))
    assert rc == 0, msg
    assert np.isnan(auc[:2]).all() and np.isnan(ap[:2]).all() and np.isnan(hits[:2]).all()
    assert not np.isnan(auc[2]) and not np.isnan(ap[2]) and not np.isnan(hits[2]).any()
    assert list(n_pos) == [0, 10, 2] and list(n_neg) == [10, 0, 8]
    rc, auc, ap, hits, n_pos, n_neg, msg = device_metrics(np.zeros((1, 1)), [[]], (1,))    # C = 1
    assert rc == 0 and np.isnan(auc[0]) and np.isnan(ap[0]) and np.isnan(hits[0, 0]) and (n_pos[0], n_neg[0]) == (0, 1)


def test_no_cut_offs_writes_auc_and_ap_alone():
    rng = np.random.RandomState(8)
    s = np.round(rng.randn(5, 200), 1)
    rows = seeded_rows(rng, 5, 200, 20)
    auc, ap, hits, _, _ = check(s, rows, ())
    assert hits.shape == (5, 0)
    lib = _lib.load()
    ptr, col = M.csr(rows)
    d_s, d_ptr, d_col = (torch.from_numpy(a).cuda() for a in (s, ptr, col))
    out = torch.empty(10, dtype=torch.float64, device="cuda")
    cnt = torch.empty(10, dtype=torch.int32, device="cuda")
    ws = torch.empty(5 * 200, dtype=torch.int64, device="cuda")
    rc = lib.gss_rank_metrics_rows(5, 200, _lib.ptr(d_s), 200, _lib.ptr(d_ptr), _lib.ptr(d_col), 0, None, _lib.ptr(out), _lib.ptr(out[5:]), None,
                                   _lib.ptr(cnt), _lib.ptr(cnt[5:]), _lib.ptr(ws), 8 * 5 * 200, _lib.current_stream())      # null ks and hits
    assert rc == 0, lib.gss_last_error()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:5]), _bits(auc)) and np.array_equal(_bits(got[5:]), _bits(ap))


def test_refusals_by_name():
    s = np.random.RandomState(6).randn(3, 20)
    ok = [[0], [1], [2]]
    for bad in (np.nan, np.inf, -np.inf):
        t = s.copy()
        t[1, 7] = bad
        rc, *_, msg = device_metrics(t, ok, (5,))
        assert rc == -22 and msg.startswith("rank_metrics_rows:") and "NaN or infinite" in msg and "row 1, column 7" in msg, msg
    rc, *_, msg = device_metrics(s, [[0], [20], [1]], (5,))
    assert rc == -22 and "rank_metrics_rows: row 1: pos_col 20 is outside [0, 20)" in msg, msg
    rc, *_, msg = device_metrics(s, [[0], [-1], [1]], (5,))
    assert rc == -22 and "outside" in msg, msg
    rc, *_, msg = device_metrics(s, [[0, 4, 4], [1], [2]], (5,))
    assert rc == -22 and "rank_metrics_rows: row 0: pos_col 4 is repeated" in msg, msg
    rc, *_, msg = device_metrics(s, ok, tuple(range(1, 10)))
    assert rc == -22 and "rank_metrics_rows: nk=9 cut-offs is outside 0..8" in msg, msg
    rc, *_, msg = device_metrics(s, ok, (5, 0))
    assert rc == -22 and "rank_metrics_rows: cut-off 1 is k=0" in msg and ">= 1" in msg, msg
    rc, *_, msg = device_metrics(s, ok, (5,), workspace_bytes=8 * 3 * 20 - 8)
    assert rc == -22 and "rank_metrics_rows: the workspace has 472 bytes" in msg and "= 480" in msg, msg
    lib = _lib.load()
    d_s = torch.from_numpy(s).cuda()
    d_ptr = torch.tensor([0, 2, 1, 3], dtype=torch.int32, device="cuda")          # decreasing between rows 1 and 2
    d_col = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    out = torch.empty(9, dtype=torch.float64, device="cuda")
    cnt = torch.empty(6, dtype=torch.int32, device="cuda")
    ws = torch.empty(60, dtype=torch.int64, device="cuda")
    ks = np.asarray([5], np.int32)
    rc = lib.gss_rank_metrics_rows(3, 20, _lib.ptr(d_s), 20, _lib.ptr(d_ptr), _lib.ptr(d_col), 1, ks.ctypes.data, _lib.ptr(out), _lib.ptr(out[3:]),
                                   _lib.ptr(out[6:]), _lib.ptr(cnt), _lib.ptr(cnt[3:]), _lib.ptr(ws), 480, _lib.current_stream())
    assert rc == -22 and b"rank_metrics_rows: row 1: pos_ptr is not a CSR row pointer" in lib.gss_last_error(), lib.gss_last_error()
    buf = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = lib.gss_rank_metrics_rows(1, MAX_COLS + 1, _lib.ptr(buf), MAX_COLS + 1, _lib.ptr(buf), _lib.ptr(buf), 1, ks.ctypes.data, _lib.ptr(buf),
                                   _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), 64, _lib.current_stream())
    assert rc == -22 and b"rank_metrics_rows: C=16385" in lib.gss_last_error() and b"above the limit of 16384" in lib.gss_last_error()
