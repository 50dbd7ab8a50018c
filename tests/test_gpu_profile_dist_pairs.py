"""GPU: gss_profile_dist_pairs (csrc/profile_dist.hip) -- the distance of listed column pairs -- against scipy per pair within the derived
bounds of profile_dist_mirror.py (the ones test_gpu_profile_dist.py holds the matrix kernel to), against the diagonal of gss_profile_dist
within twice those bounds (both sides are within one bound of scipy), its bit-level contract (the order of every sum depends on n alone),
the NaN cases, guard words behind out and behind the workspace on every call, and its refusals by name."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.distance import cdist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import profile_dist_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import compare_profile_pairs, compare_profiles  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 8          # fp64 words behind out and behind the workspace
SENTINEL = -7.25


def i32(v):
    return torch.tensor(np.asarray(v, dtype=np.int32), dtype=torch.int32, device="cuda")


def call(n, x, ld, T, ca, cb, metric, out, ws, ws_bytes):
    lib = _lib.load()
    rc = lib.gss_profile_dist_pairs(n, _lib.ptr(x), ld, T, _lib.ptr(ca), _lib.ptr(cb), metric, _lib.ptr(out), _lib.ptr(ws), ws_bytes,
                                    _lib.current_stream())
    torch.cuda.synchronize()
    return rc, lib.gss_last_error().decode(errors="replace")


def pairs(x, ca, cb, metric):
    """the raw entry point on device x [n][ld] with guard words behind out and behind the workspace -> host [T]"""
    n, ld, T = x.shape[0], x.shape[1], len(ca)
    need = _lib.load().gss_profile_dist_pairs_workspace_bytes(n, T)
    assert need % 8 == 0 and need >= 8 * 3 * T * -(-n // 32)
    out = torch.full((T + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.full((need // 8 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    rc, msg = call(n, x, ld, T, i32(ca), i32(cb), M.METRICS.index(metric), out, ws, need)
    assert rc == 0, msg
    assert bool((out[T:] == SENTINEL).all()) and bool((ws[need // 8:] == SENTINEL).all()), (metric, n, T)
    return out[:T].cpu().numpy()


def device_matrix(p, extra):
    """host profiles [k][n] -> device x [n][k + extra], the columns past k poisoned with NaN"""
    k, n = p.shape
    x = torch.full((n, k + extra), float("nan"), dtype=torch.float64, device="cuda")
    x[:, :k] = torch.from_numpy(p).cuda().t()
    return x


def pair_list(k, T, seed):
    """adjacent pairs in both orders and at both parities (2 j, 2 j + 1 share 16 bytes; 2 j + 1, 2 j + 2 do not), a column with itself,
    repeated pairs and scattered ones"""
    rng = np.random.RandomState(seed)
    fixed = [(0, 1), (3, 2), (1, 2), (4, 3), (5, 5), (0, 1), (k - 1, 0), (k - 2, k - 1)]
    ca = [a for a, _ in fixed] + list(rng.randint(0, k, size=max(0, T - len(fixed))))
    cb = [b for _, b in fixed] + list(rng.randint(0, k, size=max(0, T - len(fixed))))
    order = rng.permutation(max(T, len(fixed)))[:T] if T >= len(fixed) else np.arange(T)
    return np.asarray(ca)[order], np.asarray(cb)[order]


def scipy_pairs(p, ca, cb, metric):
    with np.errstate(invalid="ignore", divide="ignore"):
        return cdist(p, p, metric)[ca, cb] if len(ca) else np.zeros(0)


def within_twice_the_bound(got, full, metric, n):
    """the pair kernel against the matrix kernel's value of the same pair: each is within one bound of scipy, so they are within two of
    each other (relative to scipy's value for the difference class; the matrix kernel's stands in for it, which moves the bound by a factor
    1 + 4 gamma: the 1.0001)"""
    assert np.array_equal(np.isnan(got), np.isnan(full)), metric
    ok = ~np.isnan(full)
    err = np.abs(got[ok] - full[ok])
    bound = 2.0001 * M.diff_rel_bound(n) * np.abs(full[ok]) if metric in M.DIFF_CLASS else 2.0 * M.dot_abs_bound(n)
    assert np.all(err <= bound), (metric, n, float(np.max(err)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("n", [1, 7, 255, 257, 1000])
@pytest.mark.parametrize("T", [0, 1, 3, 130])
def test_pairs_against_scipy_and_the_matrix_kernel(n, T):
    k = 12
    p = M.synthetic(1000 * n + T, k, n, lognormal=(n == 1000))
    M.check_spread(p)
    ca, cb = pair_list(k, T, n + T)
    for extra in (4, 5):                                  # ld = 16: 16-byte loads for the aligned neighbours; ld = 17: none
        x = device_matrix(p, extra)
        for m in M.METRICS:
            got = pairs(x, ca, cb, m)
            worst = M.compare(got, scipy_pairs(p, ca, cb, m), m, n)
            if T:
                full = compare_profiles(x, ca, cb, m).cpu().numpy().diagonal()
                within_twice_the_bound(got, full, m, n)
            print(m, n, T, x.shape[1], "worst / bound", worst)


def test_bit_level_contract():
    k, n, T = 40, 1000, 300
    p = M.synthetic(3, k, n)
    x = device_matrix(p, 2)
    ca, cb = pair_list(k, T, 9)
    perm = np.random.RandomState(4).permutation(T)
    for m in M.METRICS:
        ab = pairs(x, ca, cb, m)
        assert not np.isnan(ab).any()
        assert np.array_equal(bits(ab), bits(pairs(x, ca, cb, m))), m                               # two runs
        assert np.array_equal(bits(ab)[perm], bits(pairs(x, ca[perm], cb[perm], m))), m              # a permuted list permutes the output
        assert np.array_equal(bits(ab), bits(pairs(x, cb, ca, m))), m                               # out(a, b) == out(b, a)
        for t in (0, 63, 64, 255, 256, 299):                                                        # a pair alone == inside the list
            assert bits(pairs(x, ca[t:t + 1], cb[t:t + 1], m))[0] == bits(ab)[t], (m, t)
        same = ca == cb
        assert same.any()
        first = {}
        for t in range(T):                                                                          # a repeated pair repeats its bits
            assert first.setdefault((ca[t], cb[t]), bits(ab)[t]) == bits(ab)[t], (m, t)
        if m in M.DIFF_CLASS:
            own = pairs(x, np.arange(k), np.arange(k), m)
            assert np.array_equal(own, np.zeros(k)) and not np.signbit(own).any(), m


def test_the_16_byte_load_changes_no_bit():
    """the same profiles at an even and an odd ld (the odd one takes no 16-byte load) and at an 8-byte-aligned base"""
    k, n = 10, 257
    p = M.synthetic(8, k, n)
    ca, cb = pair_list(k, 40, 2)
    even, odd = device_matrix(p, 2), device_matrix(p, 3)
    shifted = torch.full((n * 12 + 1,), float("nan"), dtype=torch.float64, device="cuda")[1:].view(n, 12)
    shifted[:, :k] = even[:, :k]
    assert even.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 8
    for m in M.METRICS:
        want = bits(pairs(even, ca, cb, m))
        assert np.array_equal(want, bits(pairs(odd, ca, cb, m))), m
        assert np.array_equal(want, bits(pairs(shifted, ca, cb, m))), m


def test_nan_cases_and_canberra_zero_terms():
    fx = M.fixture()
    x = device_matrix(M.DEGENERATE, 3)
    ca, cb = np.repeat(np.arange(4), 4), np.tile(np.arange(4), 4)
    for m in M.METRICS:
        got = pairs(x, ca, cb, m)
        M.compare(got.reshape(4, 4), fx["deg_" + m], m, 4)
        if m in ("cosine", "correlation"):
            assert np.isnan(got.reshape(4, 4)[1]).all()                     # the zero vector
        if m == "correlation":
            assert np.isnan(got.reshape(4, 4)[2]).all()                     # the constant vector
    assert pairs(x, [1], [1], "canberra")[0] == 0.0                          # every term 0 / 0


def test_the_python_entry_point_takes_host_and_device_profiles():
    k, n = 9, 203
    p = M.synthetic(21, k, n)
    x = device_matrix(p, 7)
    ca, cb = pair_list(k, 20, 6)
    for m in M.METRICS:
        on_device = compare_profile_pairs(x, ca, cb, m)
        assert on_device.is_cuda and on_device.dtype == torch.float64 and on_device.shape == (20,)
        M.compare(on_device.cpu().numpy(), scipy_pairs(p, ca, cb, m), m, n)
        M.compare(compare_profile_pairs(p, ca, cb, m).cpu().numpy(), scipy_pairs(p, ca, cb, m), m, n)
    assert compare_profile_pairs(x, [], [], "cosine").shape == (0,)
    with pytest.raises(ValueError, match="col_a lists 2 profiles and col_b 1"):
        compare_profile_pairs(x, [0, 1], [2], "cosine")
    with pytest.raises(ValueError, match="col_b index 16 is outside"):
        compare_profile_pairs(x, [0], [16], "cosine")
    with pytest.raises(ValueError, match="'chebyshev' is unknown"):
        compare_profile_pairs(x, [0], [1], "chebyshev")


def test_refusals_by_name():
    lib = _lib.load()
    x = torch.rand(8, 6, dtype=torch.float64, device="cuda")
    need = lib.gss_profile_dist_pairs_workspace_bytes(8, 3)
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    ws = torch.zeros(need // 8 + 1, dtype=torch.float64, device="cuda")
    a, b = i32([0, 1, 2]), i32([3, 4, 5])
    cases = [((0, x, 6, 3, a, b, 0, out, ws, need), "n=0"),
             ((8, x, 6, -1, a, b, 0, out, ws, need), "T=-1"),
             ((8, x, 6, (1 << 21) + 1, a, b, 0, out, ws, need), "T=2097153 pairs must be in [0, 2097152]"),
             ((8, x, 6, 3, a, b, 5, out, ws, need), "metric 5 is unknown"),
             ((8, x, 6, 3, a, b, -1, out, ws, need), "metric -1 is unknown"),
             ((8, x, 0, 3, a, b, 0, out, ws, need), "ld=0"),
             ((8, None, 6, 3, a, b, 0, out, ws, need), "x is null"),
             ((8, x, 6, 3, None, b, 0, out, ws, need), "col_a is null"),
             ((8, x, 6, 3, a, None, 0, out, ws, need), "col_b is null"),
             ((8, x, 6, 3, a, b, 0, None, ws, need), "out is null"),
             ((8, x, 6, 3, a, b, 0, out, None, need), "workspace is null"),
             ((8, x, 6, 3, a, b, 0, out, ws, need - 8), f"workspace of {need - 8} bytes is below the {need}"),
             ((8, x, 6, 3, i32([0, 6, 7]), b, 3, out, ws, need), "col_a[1] = 6 is outside [0, ld=6)"),
             ((8, x, 6, 3, a, i32([1, 2, -1]), 4, out, ws, need), "col_b[2] = -1 is outside [0, ld=6)")]
    for args, message in cases:
        rc, msg = call(*args)
        assert rc == -22 and message in msg, (message, rc, msg)
    assert bool((out == 0).all())                                            # no refused call wrote a distance
    misaligned = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")[4:]
    rc, msg = call(8, x, 6, 3, a, b, 0, out, misaligned, need)
    assert rc == -22 and "workspace is not 8-byte aligned" in msg, msg
    assert lib.gss_profile_dist_pairs_workspace_bytes(0, 3) == 0 and lib.gss_profile_dist_pairs_workspace_bytes(8, -1) == 0
    rc, msg = call(8, None, 6, 0, None, None, 0, None, None, 0)              # T = 0: a no-op that looks at no pointer
    assert rc == 0, msg
    rc, msg = call(8, x, 6, 3, a, b, 0, out, ws, need)
    assert rc == 0, msg
    M.compare(out.cpu().numpy(), scipy_pairs(x.cpu().numpy().T, [0, 1, 2], [3, 4, 5], "cityblock"), "cityblock", 8)
    # lists of more than one 256-thread block of the check: the least offending position is named, col_a's before col_b's, nothing is
    # written, and the status words are armed again by every call.  (Neither list may be null here: there is no null-list case.)
    n, ld, L = 70, 8, 300
    x = torch.rand(n, ld, dtype=torch.float64, device="cuda")
    rng = np.random.RandomState(3)
    ga, gb = rng.randint(0, ld, L), rng.randint(0, ld, L)

    def with_bad(v, *entries):
        w = v.copy()
        for at, e in entries:
            w[at] = e
        return i32(w)
    need = lib.gss_profile_dist_pairs_workspace_bytes(n, L)
    out = torch.full((L,), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.zeros(need // 8, dtype=torch.float64, device="cuda")
    for ca, cb, message in ((with_bad(ga, (290, 8), (270, -3)), i32(gb), "col_a[270] = -3 is outside [0, ld=8)"),
                            (with_bad(ga, (290, 8)), with_bad(gb, (5, 9)), "col_a[290] = 8 is outside [0, ld=8)"),
                            (i32(ga), with_bad(gb, (299, 8)), "col_b[299] = 8 is outside [0, ld=8)")):
        rc, msg = call(n, x, ld, L, ca, cb, 0, out, ws, need)
        assert rc == -22 and msg.startswith("profile_dist_pairs: ") and message in msg, (message, rc, msg)
        assert bool((out == SENTINEL).all()), message
    rc, msg = call(n, x, ld, L, i32(ga), i32(gb), 0, out, ws, need)          # the same buffers, valid lists
    assert rc == 0, msg
    M.compare(out.cpu().numpy(), scipy_pairs(x.cpu().numpy().T, ga, gb, "cityblock"), "cityblock", n)
