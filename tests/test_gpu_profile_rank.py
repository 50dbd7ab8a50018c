"""GPU: gss_profile_rank (csrc/profile_rank.hip) bit for bit against scipy.stats.rankdata, through lists, strides and guard words, its
bit-stability contract and its refusals by name; diffusion.rank_profiles on the three kinds of input."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.stats import rankdata

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import profile_rank_mirror as R  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import rank_profiles  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
GUARD = 0x5A


def upload(p, ld=None):
    """host [K][N] -> device x [N][ld], profile c in column c, NaN in the columns past K"""
    k, n = p.shape
    x = torch.full((n, ld or k), float("nan"), dtype=torch.float64, device="cuda")
    x[:, :k] = torch.from_numpy(p).cuda().t()
    return x


def i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int32), dtype=torch.int32, device="cuda")


def call(n, x, ld, nc, cols, r, ld_r, ws, ws_bytes):
    lib = _lib.load()
    rc = lib.gss_profile_rank(n, x if isinstance(x, int) else _lib.ptr(x), ld, nc, _lib.ptr(cols), r if isinstance(r, int) else _lib.ptr(r), ld_r,
                              ws if isinstance(ws, int) else _lib.ptr(ws), ws_bytes, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, lib.gss_last_error().decode(errors="replace")


def ranks(x, nc, cols=None, ld_r=None):
    """the raw entry point with guard words behind r and behind the workspace -> host r [n][ld_r]; asserts the guards and the spare columns"""
    n, ld = x.shape[0], (x.stride(0) if x.shape[0] > 1 else x.shape[1])
    ld_r = ld_r or nc
    need = int(_lib.load().gss_profile_rank_workspace_bytes(n, nc))
    assert need == R.workspace_bytes(n, nc)
    r = torch.full((n * ld_r + 16,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.full((need + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 8 == 0
    rc, msg = call(n, x, ld, nc, None if cols is None else i32(cols), r, ld_r, ws, need)
    assert rc == 0, msg
    assert bool((r[n * ld_r:] == SENTINEL).all()) and bool((ws[need:] == GUARD).all())
    out = r[:n * ld_r].view(n, ld_r).cpu().numpy()
    assert np.all(out[:, nc:] == SENTINEL)                                     # columns j >= nc of r are not touched
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("n", R.SIZES)
def test_exact_against_rankdata(n):
    p = R.columns(n, 34, 7 * n)
    p[5, n // 3] = np.nan                                                       # a column with one NaN: all NaN out
    assert np.isinf(p[2]).any()                                                 # +-inf are ordinary extremes
    want = rankdata(p, axis=1).T                                                # once per n; every call below is a slice of it
    assert np.isnan(want[:, 5]).all() and not np.isnan(np.delete(want, 5, axis=1)).any()
    x = upload(p)
    for nc in (1, 17, 33):
        got = ranks(x, nc)
        assert np.array_equal(got, want[:, :nc], equal_nan=True), (n, nc)
    for c in (1, 2, 3, 5):                                                      # nc = 1 with each kind of column, and the NaN one
        assert np.array_equal(ranks(x, 1, [c]), want[:, [c]], equal_nan=True), (n, c)


def test_lists_strides_and_guards():
    n, k = 1000, 40
    p = R.columns(n, k, 11)
    want = rankdata(p, axis=1).T
    x = upload(p, ld=k + 9)                                                     # NaN in the unused columns of x
    rng = np.random.RandomState(2)
    cols = np.concatenate([rng.permutation(k), [3, 3, 0, k - 1, 17, 3]])        # permuted, with repeats
    assert np.array_equal(ranks(x, len(cols), cols, ld_r=len(cols) + 5)[:, :len(cols)], want[:, cols])
    assert np.array_equal(ranks(x, k, None, ld_r=k + 3)[:, :k], want)           # the null list
    assert np.array_equal(ranks(x, 7, None), want[:, :7])
    one = upload(p[:, :1].copy())                                               # n = 1: a single row
    assert np.array_equal(ranks(one, k), np.ones((1, k)))


def test_more_columns_than_a_panel():
    n, k = 65, 2 * R.PANEL + 3
    p = R.columns(n, k, 5)
    want = rankdata(p, axis=1).T
    cols = np.random.RandomState(4).permutation(k)
    assert np.array_equal(ranks(upload(p), k, cols), want[:, cols])


def test_bit_stability():
    n, k = 32769, 300
    p = R.columns(n, k, 13)
    x = upload(p)
    whole, again = ranks(x, k), ranks(x, k)
    assert np.array_equal(bits(whole), bits(again))                             # two runs
    for c in (0, 2, 63, 64, 150, 299):                                          # a column alone == the column inside the 300-column call
        assert np.array_equal(bits(ranks(x, 1, [c]))[:, 0], bits(whole)[:, c]), c
    back = ranks(x, 3, [299, 2, 299])                                           # another position in the list
    assert np.array_equal(bits(back), bits(whole)[:, [299, 2, 299]])
    for c in (1, 2, 7):
        assert np.array_equal(whole[:, c], rankdata(p[c]))


def test_refusals_by_name():
    n, k = 8, 6
    x = torch.rand(n, k, dtype=torch.float64, device="cuda")
    r = torch.full((n, k), SENTINEL, dtype=torch.float64, device="cuda")
    need = R.workspace_bytes(n, k)
    ws = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    off = ws.data_ptr() + 4
    cases = [((0, x, k, k, None, r, k, ws, need), "n=0"),
             (((1 << 24) + 1, x, k, k, None, r, k, ws, need), "quadratic in n / chunk"),          # refused before any memory of that size is needed
             ((n, x, k, -1, None, r, k, ws, need), "nc=-1"),
             ((n, x, 0, k, None, r, k, ws, need), "ld=0"),
             ((n, x, k, k, None, r, k - 1, ws, need), "ld_r=5 is below nc=6"),
             ((n, 0, k, k, None, r, k, ws, need), "x is null"),
             ((n, x, k, k, None, 0, k, ws, need), "r is null"),
             ((n, x, k, k, None, r, k, 0, need), "workspace is null"),
             ((n, x, 3, k, None, r, k, ws, need), "ld=3 is below nc=6"),
             ((n, x, k, k, None, r, k, off, need), "workspace is not 8-byte aligned"),
             ((n, x, k, k, None, r, k, ws, need - 1), f"workspace of {need - 1} bytes is below the {need} that n=8, nc=6 need"),
             ((n, x, k, 3, i32([0, 6, 7]), r, k, ws, R.workspace_bytes(n, 3)), "cols[1] = 6 is outside [0, ld=6)"),
             ((n, x, k, 3, i32([1, 2, -1]), r, k, ws, R.workspace_bytes(n, 3)), "cols[2] = -1 is outside [0, ld=6)")]
    for args, message in cases:
        rc, msg = call(*args)
        assert rc == -22 and msg.startswith("profile_rank: ") and message in msg, (message, rc, msg)
    assert bool((r == SENTINEL).all())                                          # no refused call wrote anything
    rc, msg = call(n, x, k, 0, None, 0, 0, 0, 0)                                # nc = 0: a no-op, whatever the pointers
    assert rc == 0, msg
    rc, msg = call(n, x, k, 2, i32([5, 0]), r, k, ws, need)
    assert rc == 0, msg
    assert np.array_equal(r[:, :2].cpu().numpy(), rankdata(x.cpu().numpy()[:, [5, 0]], axis=0)) and bool((r[:, 2:] == SENTINEL).all())
    # a list of more than one 256-thread block of the check: the least offending position is named, nothing is written, and the status
    # words are armed again by every call.  (One list: there is no second list to report behind it.)
    n, ld, L = 70, 8, 300
    x = torch.rand(n, ld, dtype=torch.float64, device="cuda")
    want = rankdata(x.cpu().numpy(), axis=0)
    g = np.random.RandomState(3).randint(0, ld, L)
    bad = g.copy()
    bad[290], bad[270] = 8, -3
    r = torch.full((n, L), SENTINEL, dtype=torch.float64, device="cuda")
    need = R.workspace_bytes(n, L)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    rc, msg = call(n, x, ld, L, i32(bad), r, L, ws, need)
    assert rc == -22 and msg.startswith("profile_rank: ") and "cols[270] = -3 is outside [0, ld=8)" in msg, (rc, msg)
    bad[270] = 0
    rc, msg = call(n, x, ld, L, i32(bad), r, L, ws, need)
    assert rc == -22 and "cols[290] = 8 is outside [0, ld=8)" in msg, (rc, msg)
    assert bool((r == SENTINEL).all())
    rc, msg = call(n, x, ld, L, i32(g), r, L, ws, need)                        # the same buffers, a valid list
    assert rc == 0, msg
    assert np.array_equal(r.cpu().numpy(), want[:, g])
    rc, msg = call(n, x, ld, ld, None, r, L, ws, need)                         # the null list == the explicit 0 .. ld - 1, bit for bit
    assert rc == 0, msg
    null = r[:, :ld].clone()
    rc, msg = call(n, x, ld, ld, i32(np.arange(ld)), r, L, ws, need)
    assert rc == 0 and torch.equal(r[:, :ld].view(torch.int64), null.view(torch.int64)) and np.array_equal(null.cpu().numpy(), want), msg


def test_rank_profiles_on_the_three_kinds_of_input():
    n, k = 333, 9
    p = R.columns(n, k, 21)
    want = rankdata(p, axis=1).T
    x = upload(p, ld=k + 3)
    got = rank_profiles(x[:, :k], [4, 0, 4])
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and got.shape == (n, 3)
    assert np.array_equal(got.cpu().numpy(), want[:, [4, 0, 4]])
    assert np.array_equal(rank_profiles(p).cpu().numpy(), want)                                  # host [K][N], every profile
    named = {"p%d" % j: p[j] for j in range(k)}
    assert np.array_equal(rank_profiles(named, ["p7", "p1", "p7"]).cpu().numpy(), want[:, [7, 1, 7]])
    assert rank_profiles(x, []).shape == (n, 0)
    with pytest.raises(ValueError, match="rank_profiles: column index 9 is outside"):
        rank_profiles(p, [9])
    with pytest.raises(ValueError, match="rank_profiles: column 'q' has no profile"):
        rank_profiles(named, ["q"])
    with pytest.raises(ValueError, match="cols must name"):
        rank_profiles(named)
