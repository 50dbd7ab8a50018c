"""GPU: the batched ROC-AUC kernel (csrc/auc.hip, gss_auc_rows) against sklearn.metrics.roc_auc_score on seeded score matrices: ties,
mixed signed zeros, single positives / negatives, one-class rows, the column limit, the refusals by name and order independence."""
import numpy as np
import pytest
import torch
from sklearn.metrics import roc_auc_score

from gcn_drug_repurposing_amd import _lib

pytestmark = pytest.mark.gpu

MAX_COLS = 16384


def device_aucs(scores, rows):
    """scores [R, C] fp64 host, rows: per row the positive column indices -> (rc, auc, n_pos, n_neg, error text)"""
    lib = _lib.load()
    s = np.ascontiguousarray(scores, dtype=np.float64)
    ptr = np.zeros(len(rows) + 1, np.int32)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.zeros(1, np.int32)])
    dev = torch.device("cuda")
    d_s, d_ptr, d_col = (torch.from_numpy(a).to(dev) for a in (s, ptr, col))
    R, Cn = s.shape
    auc = torch.empty(R, dtype=torch.float64, device=dev)
    n_pos = torch.empty(R, dtype=torch.int32, device=dev)
    n_neg = torch.empty(R, dtype=torch.int32, device=dev)
    rc = lib.gss_auc_rows(R, Cn, _lib.ptr(d_s), Cn, _lib.ptr(d_ptr), _lib.ptr(d_col), _lib.ptr(auc), _lib.ptr(n_pos), _lib.ptr(n_neg),
                          _lib.current_stream())
    return rc, auc.cpu().numpy(), n_pos.cpu().numpy(), n_neg.cpu().numpy(), lib.gss_last_error().decode(errors="replace")


def seeded_rows(rng, R, Cn, max_pos):
    return [np.sort(rng.choice(Cn, rng.randint(1, max_pos + 1), replace=False)) for _ in range(R)]


def check_against_sklearn(scores, rows):
    rc, auc, n_pos, n_neg, msg = device_aucs(scores, rows)
    assert rc == 0, msg
    for r, cols in enumerate(rows):
        y = np.zeros(scores.shape[1], int)
        y[cols] = 1
        assert n_pos[r] == len(cols) and n_neg[r] == scores.shape[1] - len(cols)
        assert abs(auc[r] - roc_auc_score(y, scores[r])) <= 1e-12, (r, auc[r], roc_auc_score(y, scores[r]))
    return auc


def test_heavy_ties_and_signed_zeros():
    rng = np.random.RandomState(1)
    s = np.round(rng.randn(64, 1661), 0) * 0.5                 # a handful of levels: large tie groups
    s[s == 0] = np.where(rng.rand(int((s == 0).sum())) < 0.5, -0.0, 0.0)
    assert np.any(np.signbit(s) & (s == 0)) and np.any(~np.signbit(s) & (s == 0))
    check_against_sklearn(s, seeded_rows(rng, 64, 1661, 40))


def test_single_positive_single_negative_and_small_widths():
    rng = np.random.RandomState(2)
    s = rng.randn(8, 1661)
    rows = [[5]] * 4 + [[c for c in range(1661) if c != k] for k in (0, 7, 1000, 1660)]
    check_against_sklearn(s, rows)
    check_against_sklearn(np.array([[0.3, 0.3], [1.0, -1.0]]), [[0], [1]])


def test_msi_width_and_the_column_limit():
    rng = np.random.RandomState(3)
    check_against_sklearn(rng.randn(840, 1661), seeded_rows(rng, 840, 1661, 30))
    s = np.round(rng.randn(6, MAX_COLS), 3)
    check_against_sklearn(s, seeded_rows(rng, 6, MAX_COLS, 4000))


def test_one_class_rows_are_nan_with_their_counts():
    s = np.random.RandomState(4).randn(3, 10)
    rc, auc, n_pos, n_neg, msg = device_aucs(s, [[], list(range(10)), [2, 3]])
    assert rc == 0, msg
    assert np.isnan(auc[0]) and np.isnan(auc[1]) and not np.isnan(auc[2])
    assert list(n_pos) == [0, 10, 2] and list(n_neg) == [10, 0, 8]
    rc, auc, n_pos, n_neg, msg = device_aucs(np.zeros((1, 1)), [[]])    # C = 1
    assert rc == 0 and np.isnan(auc[0]) and (n_pos[0], n_neg[0]) == (0, 1)


def test_permuted_columns_give_bitwise_equal_results():
    rng = np.random.RandomState(5)
    s = np.round(rng.randn(32, 1661), 1)
    rows = seeded_rows(rng, 32, 1661, 50)
    a = check_against_sklearn(s, rows)
    perm = rng.permutation(1661)
    inv = np.argsort(perm)
    b = check_against_sklearn(s[:, perm], [np.asarray([inv[c] for c in r])[::-1] for r in rows])
    assert a.tobytes() == b.tobytes()
    assert device_aucs(s, rows)[1].tobytes() == a.tobytes()


def test_refusals_by_name():
    s = np.random.RandomState(6).randn(3, 20)
    for bad in (np.nan, np.inf, -np.inf):
        t = s.copy()
        t[1, 7] = bad
        rc, _, _, _, msg = device_aucs(t, [[0], [1], [2]])
        assert rc == -22 and "NaN or infinite" in msg and "row 1, column 7" in msg, msg
    rc, _, _, _, msg = device_aucs(s, [[0], [20], [1]])
    assert rc == -22 and "pos_col 20 is outside [0, 20)" in msg, msg
    rc, _, _, _, msg = device_aucs(s, [[0], [-1], [1]])
    assert rc == -22 and "outside" in msg, msg
    rc, _, _, _, msg = device_aucs(s, [[0, 4, 4], [1], [2]])
    assert rc == -22 and "row 0: pos_col 4 is repeated" in msg, msg
    lib = _lib.load()
    d_s = torch.from_numpy(s).cuda()
    d_ptr = torch.tensor([0, 2, 1, 3], dtype=torch.int32, device="cuda")          # decreasing between rows 1 and 2
    d_col = torch.tensor([0, 1, 2], dtype=torch.int32, device="cuda")
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    cnt = torch.empty(6, dtype=torch.int32, device="cuda")
    rc = lib.gss_auc_rows(3, 20, _lib.ptr(d_s), 20, _lib.ptr(d_ptr), _lib.ptr(d_col), _lib.ptr(out), _lib.ptr(cnt), _lib.ptr(cnt[3:]),
                          _lib.current_stream())
    assert rc == -22 and b"row 1: pos_ptr is not a CSR row pointer" in lib.gss_last_error(), lib.gss_last_error()
    buf = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = lib.gss_auc_rows(1, MAX_COLS + 1, _lib.ptr(buf), MAX_COLS + 1, _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf), _lib.ptr(buf),
                          _lib.ptr(buf), _lib.current_stream())
    assert rc == -22 and b"above the limit of 16384" in lib.gss_last_error()
