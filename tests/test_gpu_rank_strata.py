"""GPU: csrc/rank_strata.hip (gss_rank_metrics_strata) against gss_rank_metrics_rows on each stratum gathered into a row of its own, and
against the host mirror (rank_strata_mirror.py).  For every stratum: auc, hits and the counts bit-equal to the mirror; ap bit-equal to
the mirror's statement of the kernel's order of additions (M.ap_ordered on the gathered sub-problem) and within
(|Q| + 3) 2^-53 relative of the mirror's exactly rounded value (test_gpu_rank_metrics.py's derived bound: any order of summing |Q| positive,
correctly rounded terms, plus the final division); and for up to 24 strata per test every output word bit-equal to what
gss_rank_metrics_rows writes for the gathered sub-problem (R = 1).  A stratum with all of its row's positives has the row's words.  Then
the structure cases, order independence, the sentinels behind the outputs and the device-side refusals by name."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rank_metrics_mirror as M  # noqa: E402
import rank_strata_mirror as RS  # noqa: E402
from gcn_drug_repurposing_amd import _lib  # noqa: E402
from test_gpu_rank_metrics import _bits, device_metrics, heavy_ties  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_COLS = 16384
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)        # |Q_s| across the sort's minimum pad and the workgroup's thread count
GUARD = 3                                                 # sentinel words behind every per-stratum output


def device_strata(scores, ptr, col, sp, qp, qc, ks, ld=None, workspace_bytes=None):
    """scores [R, C] fp64 host and the four CSR arrays as given (not checked here) -> (rc, auc, ap, hits [S, nk], s_pos, s_neg, n_pos, n_neg,
    error text); the words behind auc, ap, hits and s_pos must come back as they went in"""
    lib = _lib.load()
    s = np.ascontiguousarray(scores, dtype=np.float64)
    R, Cn = s.shape
    ld = Cn if ld is None else ld
    if ld > Cn:
        s = np.concatenate([s, np.full((R, ld - Cn), np.nan)], axis=1)           # nothing behind a row's C columns is read
    dev = torch.device("cuda")
    up = lambda a: torch.from_numpy(np.concatenate([np.asarray(a, np.int32), np.zeros(1, np.int32)])).to(dev)   # noqa: E731
    d_s, d_ptr, d_col, d_sp, d_qp, d_qc = torch.from_numpy(s).to(dev), up(ptr), up(col), up(sp), up(qp), up(qc)
    S, nk = len(qp) - 1, len(ks)
    h_ks = np.asarray(list(ks) + [0], dtype=np.int32)
    auc = torch.full((S + GUARD,), -7.0, dtype=torch.float64, device=dev)
    ap = torch.full((S + GUARD,), -7.0, dtype=torch.float64, device=dev)
    hits = torch.full((S * nk + GUARD,), -7.0, dtype=torch.float64, device=dev)
    s_pos = torch.full((S + GUARD,), -77, dtype=torch.int32, device=dev)
    s_neg = torch.full((S + GUARD,), -77, dtype=torch.int32, device=dev)
    n_pos = torch.full((R,), -77, dtype=torch.int32, device=dev)
    n_neg = torch.full((R,), -77, dtype=torch.int32, device=dev)
    need = lib.gss_rank_strata_workspace_bytes(len(qc))
    assert need == 8 * len(qc)
    ws = torch.empty(max(len(qc), 1), dtype=torch.int64, device=dev)
    rc = lib.gss_rank_metrics_strata(R, Cn, _lib.ptr(d_s), ld, _lib.ptr(d_ptr), _lib.ptr(d_col), S, _lib.ptr(d_sp), _lib.ptr(d_qp), _lib.ptr(d_qc), nk,
                                     h_ks.ctypes.data, _lib.ptr(auc), _lib.ptr(ap), _lib.ptr(hits), _lib.ptr(s_pos), _lib.ptr(s_neg), _lib.ptr(n_pos),
                                     _lib.ptr(n_neg), _lib.ptr(ws), need if workspace_bytes is None else workspace_bytes, _lib.current_stream())
    msg = lib.gss_last_error().decode(errors="replace")
    auc, ap, hits, s_pos, s_neg = (t.cpu().numpy() for t in (auc, ap, hits, s_pos, s_neg))
    assert np.all(auc[S:] == -7.0) and np.all(ap[S:] == -7.0) and np.all(hits[S * nk:] == -7.0) and np.all(s_pos[S:] == -77) and np.all(s_neg[S:] == -77)
    return rc, auc[:S], ap[:S], hits[:S * nk].reshape(S, nk), s_pos[:S], s_neg[:S], n_pos.cpu().numpy(), n_neg.cpu().numpy(), msg


def run(scores, rows, strata, ks, **kw):
    ptr, col = M.csr(rows)
    return device_strata(scores, ptr, col, *RS.strata_csr(strata), ks, **kw)


def check(scores, rows, strata, ks, gather=24, **kw):
    """the comparisons of the module docstring -> the device outputs (auc, ap, hits, s_pos, s_neg, n_pos, n_neg)"""
    scores = np.asarray(scores, np.float64)
    rc, auc, ap, hits, s_pos, s_neg, n_pos, n_neg, msg = run(scores, rows, strata, ks, **kw)
    assert rc == 0, msg
    ptr, col = M.csr(rows)
    sp, qp, qc = RS.strata_csr(strata)
    m_auc, m_ap, m_hits, m_spos, m_pos, m_neg = RS.mirror_strata(scores, ptr, col, sp, qp, qc, ks)
    owner = [r for r in range(len(rows)) for _ in strata[r]]
    assert np.array_equal(n_pos, m_pos) and np.array_equal(n_neg, m_neg) and np.array_equal(s_pos, m_spos)
    assert np.array_equal(s_neg, m_neg[owner]) if len(owner) else len(s_neg) == 0
    assert np.array_equal(_bits(auc), _bits(m_auc)), (auc, m_auc)
    assert hits.shape == m_hits.shape and np.array_equal(_bits(hits), _bits(m_hits)), (hits[hits != m_hits], m_hits[hits != m_hits])
    worst = 0.0
    for s in range(len(owner)):
        if np.isnan(m_ap[s]):
            assert _bits(ap[s:s + 1])[0] == _bits(m_ap[s:s + 1])[0] and (s_pos[s] == 0 or s_neg[s] == 0)
            continue
        bound = (int(s_pos[s]) + 3) * 2.0 ** -53 * m_ap[s]
        print(f"stratum {s}: |Q| = {s_pos[s]}, N = {s_neg[s]}, ap = {ap[s]!r}, mirror {m_ap[s]!r}, bound {bound:.3e}")
        worst = max(worst, abs(ap[s] - m_ap[s]) / bound)
        assert abs(ap[s] - m_ap[s]) <= bound, (s, s_pos[s], ap[s], m_ap[s])
        x, cols = RS.gathered(scores[owner[s]], rows[owner[s]], qc[qp[s]:qp[s + 1]])
        mask = np.zeros(len(x), bool)
        mask[cols] = True
        ordered = M.ap_ordered_row(x, mask)
        assert _bits(ap[s:s + 1])[0] == _bits([ordered])[0], (s, s_pos[s], ap[s], ordered)
    print(f"C={scores.shape[1]}: worst |ap - mirror| / ((|Q| + 3) 2^-53 ap) = {worst:.3f}")
    # the gathered sub-problems through the rows' kernel: the ranked strata, spread evenly when there are more than `gather`
    ranked = [s for s in range(len(owner)) if s_pos[s] > 0 and s_neg[s] > 0]
    chosen = ranked if len(ranked) <= gather else [ranked[i] for i in np.unique(np.linspace(0, len(ranked) - 1, gather).astype(int))]
    assert len(chosen) <= 24
    for s in chosen:
        r = owner[s]
        x, cols = RS.gathered(scores[r], rows[r], qc[qp[s]:qp[s + 1]])
        rc, g_auc, g_ap, g_hits, g_pos, g_neg, msg = device_metrics(x[None, :], [cols], ks)
        assert rc == 0, msg
        got = (auc[s:s + 1], ap[s:s + 1], hits[s:s + 1], s_pos[s:s + 1], s_neg[s:s + 1])
        for a, b in zip(got, (g_auc, g_ap, g_hits, g_pos, g_neg)):
            assert a.tobytes() == b.tobytes(), (s, a, b)
    return auc, ap, hits, s_pos, s_neg, n_pos, n_neg


def whole_rows_agree(scores, rows, strata, ks, out):
    """every stratum that holds all of its row's positives has the words gss_rank_metrics_rows writes for the row"""
    rc, r_auc, r_ap, r_hits, r_pos, r_neg, msg = device_metrics(scores, rows, ks)
    assert rc == 0, msg
    auc, ap, hits, s_pos, s_neg, n_pos, n_neg = out
    assert np.array_equal(n_pos, r_pos) and np.array_equal(n_neg, r_neg)
    s, seen = 0, 0
    for r, row in enumerate(strata):
        for q in row:
            if sorted(int(c) for c in q) == sorted(int(c) for c in rows[r]):
                for a, b in ((auc[s], r_auc[r]), (ap[s], r_ap[r]), (hits[s], r_hits[r])):
                    assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (r, s)
                seen += 1
            s += 1
    assert seen > 0


def seeded_strata(rng, p):
    """strata of one row's positives p: all of them, one, none, and two overlapping random subsets"""
    p = np.asarray(p)
    half = len(p) // 2 + 1
    return [list(rng.permutation(p)), [int(p[rng.randint(len(p))])], [], list(rng.permutation(p)[:half]), list(rng.permutation(p)[:half])]


@pytest.mark.parametrize("C", [2, 3, 64, 65, 257, 1661])
def test_widths_with_heavy_ties_and_signed_zeros(C):
    rng = np.random.RandomState(C)
    R = 8
    s = heavy_ties(rng, R, max(C, 8))[:, :C]
    if C <= 3:
        s[0, :2], s[1, :2] = (0.0, -0.0), (-0.0, 0.5)
    else:
        s[4:] = rng.randn(4, C)                                                     # and rows without ties
    rows = [np.sort(rng.choice(C, rng.randint(1, max(2, min(C - 1, 40) + 1)), replace=False)) for _ in range(R)]
    rows[R - 1] = np.arange(C - 1)                                                   # a single negative
    strata = [seeded_strata(rng, p) for p in rows]
    ks = (1, 2, 50, C - 1, C, C + 1) if C > 3 else (1, 2, 3)
    out = check(s, rows, strata, ks)
    whole_rows_agree(s, rows, strata, ks, out)


def test_stratum_sizes_across_the_pad_and_the_thread_count():
    rng = np.random.RandomState(7)
    s = np.concatenate([heavy_ties(rng, 1, 1661), np.round(rng.randn(1, 1661), 1), rng.randn(1, 1661)])
    rows = [np.sort(rng.choice(1661, 600, replace=False)) for _ in range(3)]
    strata = [[list(rng.permutation(p)[:n]) for n in SIZES] for p in rows]
    strata[2] = strata[2][6:] + [list(rows[2])]                                      # the untied row: the sizes above a wave, and every positive
    ks = (1, 10, 50, 300, 1100, 1661)
    out = check(s, rows, strata, ks)                                                 # 9 + 9 + 5 ranked strata: all through the rows' kernel
    assert sorted(set(int(n) for n in out[3])) == sorted(SIZES + (600,))
    whole_rows_agree(s, rows, strata, ks, out)


def test_the_column_limit():
    rng = np.random.RandomState(3)
    s = np.round(rng.randn(2, MAX_COLS), 2)
    s[1] = np.round(s[1], 1)
    s[s == 0] = np.where(rng.rand(int((s == 0).sum())) < 0.5, -0.0, 0.0)
    rows = [np.sort(rng.choice(MAX_COLS, 1000, replace=False)), np.sort(rng.choice(MAX_COLS, 12000, replace=False))]
    strata = [[list(rows[0]), list(rng.permutation(rows[0])[:513]), [int(rows[0][0])], list(rng.permutation(rows[0])[:257])],
              [list(rng.permutation(rows[1])), list(rng.permutation(rows[1])[:8193]), [], list(rng.permutation(rows[1])[:64])]]
    ks = (1, 50, 4000, 16383, 16384, 20000, 12000, 8192)
    out = check(s, rows, strata, ks)
    whole_rows_agree(s, rows, strata, ks, out)


def test_structure_overlap_empty_strata_rows_without_strata_one_class_rows_and_a_wide_ld():
    rng = np.random.RandomState(9)
    C = 65
    s = heavy_ties(rng, 7, C)
    rows = [[3, 9, 64, 0], [5], [], list(range(C)), [7, 8, 9, 10, 11], [1, 2], [60, 61, 62, 63, 64]]
    strata = [[[3, 9], [9, 64], [9], [0, 64, 9, 3]],            # overlapping
              [],                                               # a ranked row without strata
              [[], []],                                         # no positive: only empty strata are possible
              [[4, 5, 6], list(range(C)), []],                  # no negative: NaN with the counts
              [[], [11], []],                                   # empty strata around a ranked one
              [],
              [[64], [60, 61, 62, 63, 64]]]
    ks = (1, 3, 61, 70)
    for ld in (C, C + 7):
        auc, ap, hits, s_pos, s_neg, n_pos, n_neg = check(s, rows, strata, ks, ld=ld)
        assert list(n_pos) == [4, 1, 0, C, 5, 2, 5] and list(s_pos) == [2, 2, 1, 4, 0, 0, 3, C, 0, 0, 1, 0, 1, 5]
        assert list(s_neg) == [C - 4] * 4 + [C] * 2 + [0] * 3 + [C - 5] * 3 + [C - 5] * 2
        nan = [4, 5, 6, 7, 8, 9, 11]
        assert np.isnan(auc[nan]).all() and np.isnan(ap[nan]).all() and np.isnan(hits[nan]).all()
        rest = [k for k in range(14) if k not in nan]
        assert not np.isnan(auc[rest]).any() and not np.isnan(ap[rest]).any() and not np.isnan(hits[rest]).any()
    whole_rows_agree(s, rows, strata, ks, (auc, ap, hits, s_pos, s_neg, n_pos, n_neg))
    # no cut-offs: auc and ap alone, hits untouched (device_strata's sentinels)
    rc, auc0, ap0, hits0, *_, msg = run(s, rows, strata, ())
    assert rc == 0 and hits0.shape == (14, 0) and auc0.tobytes() == auc.tobytes() and ap0.tobytes() == ap.tobytes(), msg


def test_permuted_lists_strata_and_columns_change_no_bit():
    rng = np.random.RandomState(5)
    C, R = 257, 6
    s = np.round(rng.randn(R, C), 1)
    rows = [np.sort(rng.choice(C, rng.randint(2, 70), replace=False)) for _ in range(R)]
    strata = [seeded_strata(rng, p) + [list(rng.permutation(p)[:3])] for p in rows]
    ks = (1, 10, 50, 200)
    base = check(s, rows, strata, ks, gather=12)
    perm = rng.permutation(C)
    inv = np.argsort(perm)
    order = [rng.permutation(len(row)) for row in strata]                            # the order of a row's strata
    offset = np.cumsum([0] + [len(row) for row in strata])
    back = np.concatenate([offset[r] + np.argsort(order[r]) for r in range(R)])      # stratum s of the base run is stratum back[s] of the moved one
    moved_rows = [inv[rng.permutation(p)] for p in rows]
    moved = [[[int(inv[c]) for c in rng.permutation(strata[r][j])] if strata[r][j] else [] for j in order[r]] for r in range(R)]
    rc, *got, msg = run(s[:, perm], moved_rows, moved, ks)
    assert rc == 0, msg
    for x, y in zip(base[:5], got[:5]):
        assert x.tobytes() == y[back].tobytes()
    assert base[5].tobytes() == got[5].tobytes() and base[6].tobytes() == got[6].tobytes()
    rc, *again, msg = run(s, rows, strata, ks)                                       # run to run
    assert all(x.tobytes() == y.tobytes() for x, y in zip(base, again))


def test_device_side_refusals_by_name():
    s = np.random.RandomState(6).randn(3, 20)
    ptr, col = M.csr([[0, 4, 7], [1], [2, 3]])
    sp, qp, qc = RS.strata_csr([[[0, 4], [7]], [[1]], [[3, 2]]])
    ks = (5,)

    def refused(words, scores=s, ptr=ptr, col=col, sp=sp, qp=qp, qc=qc, **kw):
        rc, *_, msg = device_strata(scores, ptr, col, sp, qp, qc, ks, **kw)
        assert rc == -22 and msg.startswith("rank_metrics_strata: ") and words in msg, msg

    rc, *_, msg = device_strata(s, ptr, col, sp, qp, qc, ks)
    assert rc == 0, msg
    i32 = lambda *a: np.asarray(a, np.int32)   # noqa: E731
    # what gss_rank_metrics_rows refuses, in its words
    for bad in (np.nan, np.inf, -np.inf):
        t = s.copy()
        t[1, 7] = bad
        refused("row 1, column 7: the score is NaN or infinite", scores=t)
    refused("row 2: pos_col 20 is outside [0, 20)", col=i32(0, 4, 7, 1, 2, 20))
    refused("row 0: pos_col 4 is repeated", col=i32(0, 4, 4, 1, 2, 3))
    refused("row 1: pos_ptr is not a CSR row pointer", ptr=i32(0, 4, 3, 6))
    # the strata's two pointers
    refused("row 1: str_ptr is not a row pointer over [0, 4]", sp=i32(0, 3, 2, 4))
    refused("row 0: str_ptr is not a row pointer over [0, 4]", sp=i32(1, 2, 3, 4))
    refused("row 2: str_ptr is not a row pointer over [0, 4] (0 first, non-decreasing, 4 last; 3 here)", sp=i32(0, 2, 3, 3))
    refused("row 2: str_ptr is not a row pointer over [0, 4]", sp=i32(0, 2, 3, 9))
    refused("row 0, stratum 1: sub_ptr is not a row pointer over the strata", qp=i32(0, 3, 2, 4, 6))
    refused("row 0, stratum 0: sub_ptr is not a row pointer over the strata", qp=i32(1, 2, 3, 4, 6))
    refused("row 1, stratum 2: sub_ptr is not a row pointer over the strata", qp=i32(0, 2, 2, 4, 6), qc=i32(0, 4, 1, 1, 3, 2))   # 2 of 1 positive
    refused("row 0, stratum 1: sub_ptr is not a row pointer over the strata", qp=i32(0, 2, 100, 4, 6))                            # beyond sub_ptr[S]
    # a stratum's columns
    refused("row 0, stratum 1: sub_col 5 is not a positive of the row", qc=i32(0, 4, 5, 1, 3, 2))
    refused("row 2, stratum 3: sub_col 1 is not a positive of the row", qc=i32(0, 4, 7, 1, 3, 1))                                 # another row's positive
    refused("row 1, stratum 2: sub_col 20 is not a positive of the row", qc=i32(0, 4, 7, 20, 3, 2))
    refused("row 1, stratum 2: sub_col -1 is not a positive of the row", qc=i32(0, 4, 7, -1, 3, 2))
    refused("row 0, stratum 0: sub_col 4 is repeated", qp=i32(0, 3, 4, 5, 7), qc=i32(4, 0, 4, 7, 1, 3, 2))
    refused("the workspace has 40 bytes, gss_rank_strata_workspace_bytes(6) = 48", workspace_bytes=40)
