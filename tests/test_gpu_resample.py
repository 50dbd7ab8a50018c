"""GPU: csrc/resample.hip (gss_resample_stats), called directly on guarded outputs and through resample.resample_stats / paired_test, against
the numpy mirror (resample_mirror.py).

Bits: the draw and the sign are integer arithmetic, the sorted multiset is the mirror's np.sort, the median is np.median's arithmetic and the
mean's order of additions is stated in include/gssgcn.h and restated term by term in the mirror (ordered_sum): the device's statistics equal
the mirror's bit for bit, up to the sign of a zero (order_key folds -0.0 into +0.0; both sides are compared after x + 0.0), and hence each
other under every regrouping of a call.
Accuracy: a sum of n terms added in any order is within gamma(n - 1) * sum |v| of the exact sum, gamma(k) = k u / (1 - k u), u = 2^-53; the
mean is held to math.fsum(values) / n within that over n.
Every direct call writes into a buffer between canary words (guarded.Out), checked after the call; a refused call leaves it untouched."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import guarded as G  # noqa: E402
import resample_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd import resample as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES_N = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 16384)
_SERIES = {}


def series(n):
    """three series of n values with both signs, ties and both zeros -> (host, device); made once per n and never written"""
    if n not in _SERIES:
        rng = np.random.RandomState(2000 + n)
        h = rng.randn(3, n)
        if n >= 63:
            h[1, ::7] = h[1, 3]          # ties
            h[2, 5], h[2, 11] = 0.0, -0.0
        _SERIES[n] = (h, torch.from_numpy(h).cuda())
    return _SERIES[n]


def call(v, ld, S, n, mode, seed, first, count, words=None):
    """gss_resample_stats on the device tensor v with a guarded output -> (rc, the error text, the output)"""
    out = G.Out(2 * (count * S * 2 if words is None else words), dtype=torch.int32)
    lib = _lib.load()
    rc = lib.gss_resample_stats(v.data_ptr(), ld, S, n, mode, seed, first, count, out.ptr, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, lib.gss_last_error().decode(), out


def stats(v, mode, seed, count, first=0, ld=None):
    """a call that must succeed -> host fp64 [count][S][2], the canaries around it checked"""
    S, n = v.shape
    rc, msg, out = call(v, v.stride(0) if ld is None else ld, S, n, mode, seed, first, count)
    assert rc == 0, msg
    return np.ascontiguousarray(out.host("out")).view(np.float64).reshape(count, S, 2)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64) + 0.0, np.asarray(b, np.float64) + 0.0      # the sign of a zero is not defined
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the mirror, shape by shape ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES_N)
def test_statistics_equal_the_mirror(n):
    h, d = series(n)
    count = 2 if n == 16384 else 5
    for S in (1, 3):
        for mode, first, seed in ((0, 0, 0), (1, 0, 7), (1, 12345, 2 ** 63 + 5), (2, 0, 7), (2, 2 ** 31 - count, 3)):
            c = 1 if mode == 0 else count
            got = stats(d[:S], mode, seed, c, first)
            want = M.resample_stats(h[:S], mode, seed, c, first)
            assert same_bits(got, want), (n, S, mode, first, np.argwhere((got + 0.0).view(np.uint64) != (want + 0.0).view(np.uint64))[:4])
    if n > 1:      # np.median itself, and the mean within the any-order bound of fsum
        got = stats(d[:1], 1, 7, 1)[0, 0]
        values = M.gathered(h[0], 1, 7, 0)
        assert got[1] == np.median(values)
        share = abs(got[0] - math.fsum(values) / n) / M.mean_bound(values)
        print(f"n={n} |mean - fsum / n| / bound = {share:.3g}")
        assert share <= 1.0


def test_signed_zeros():
    h = np.array([[0.0, -0.0, -0.0, 0.0], [-0.0, 1.0, -1.0, 0.0]])
    d = torch.from_numpy(h).cuda()
    for mode in (0, 1, 2):
        got = stats(d, mode, 1, 1 if mode == 0 else 9)
        assert same_bits(got, M.resample_stats(h, mode, 1, len(got)))
        assert np.all(got[:, 0] == 0.0)


def test_ties_and_magnitudes():
    rng = np.random.RandomState(31)
    ties = rng.choice([0.0, 0.5, 1.0], 300)
    wide = rng.choice([-1.0, 1.0], 300) * 10.0 ** rng.uniform(-300, 300, 300)
    wide[:4] = [1e-300, -1e-300, 1e300, -1e300]
    h = np.stack([ties, wide])
    assert np.isfinite(h).all() and np.abs(wide).sum() < 1e305
    d = torch.from_numpy(h).cuda()
    for mode, count in ((0, 1), (1, 20), (2, 20)):
        got = stats(d, mode, 5, count)
        assert same_bits(got, M.resample_stats(h, mode, 5, count)), mode
        for r in range(count):
            for s in range(2):
                values = M.gathered(h[s], mode, 5, r)
                assert got[r, s, 1] == np.median(values)
                bound = M.mean_bound(values)
                print(f"mode={mode} r={r} s={s} |mean - fsum / n| = {abs(got[r, s, 0] - math.fsum(values) / 300):.3g}, bound {bound:.3g}")
                assert abs(got[r, s, 0] - math.fsum(values) / 300) <= bound
    assert len(set(stats(d, 1, 5, 20)[:, 0, 1])) <= 3      # a median of ties is one of the tied values (or their midpoint: n is even)
    assert set(stats(d, 1, 5, 20)[:, 0, 1]) <= {0.0, 0.25, 0.5, 0.75, 1.0}


# ---- bit-equality under regrouping -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (65, 1025))
def test_replicates_do_not_depend_on_how_a_call_is_cut(n):
    h, d = series(n)
    for mode in (1, 2):
        whole = stats(d, mode, 9, 64)
        assert same_bits(whole, stats(d, mode, 9, 64))                                                  # run to run
        parts = np.concatenate([stats(d, mode, 9, 10, 0), stats(d, mode, 9, 54, 10)])
        assert np.array_equal(parts.view(np.uint64), whole.view(np.uint64))                             # replicates in two calls
        for s in range(3):                                                                              # a series alone
            alone = stats(d[s:s + 1], mode, 9, 64)
            assert np.array_equal(alone[:, 0].view(np.uint64), np.ascontiguousarray(whole[:, s]).view(np.uint64)), (mode, s)
        padded = torch.full((3, n + 5), float("nan"), dtype=torch.float64, device="cuda")               # ld > n, the padding poisoned
        padded[:, :n] = d
        assert np.array_equal(stats(padded[:, :n], mode, 9, 64, ld=n + 5).view(np.uint64), whole.view(np.uint64))
    assert same_bits(stats(d[:, :n], 0, 0, 1), M.resample_stats(h, 0, 0, 1))


def test_the_wrapper_chunks_and_uploads(monkeypatch):
    h, d = series(65)
    whole = R.resample_stats(d, "bootstrap", 9, 64)
    assert whole.shape == (64, 3, 2) and whole.dtype == np.float64
    assert np.array_equal(whole.view(np.uint64), stats(d, 1, 9, 64).view(np.uint64))
    monkeypatch.setattr(R, "CHUNK_BYTES", 16 * 3 * 7)                                                   # 7 replicates per call
    assert np.array_equal(R.resample_stats(h, 1, 9, 64).view(np.uint64), whole.view(np.uint64))         # a host array, in ten calls
    assert np.array_equal(R.resample_stats(h, 1, 9, 14, first=50).view(np.uint64), whole[50:].view(np.uint64))
    assert np.array_equal(R.resample_stats(h[1], 2, 9, 3)[:, 0].view(np.uint64), np.ascontiguousarray(stats(d, 2, 9, 3)[:, 1]).view(np.uint64))
    assert R.resample_stats(d, 1, 9, 0).shape == (0, 3, 2)
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        R.resample_stats(h, 1, 9, 4, device="cpu")
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        R.resample_stats(torch.from_numpy(h), 1, 9, 4)


def test_plain_is_a_sign_flip_without_a_flip():
    h, d = series(3)
    seed = 0
    b = next(b for b in range(200) if not M.flips(seed, b, 3).any())      # the mirror says: replicate b negates nothing
    assert np.array_equal(stats(d, 2, seed, 1, first=b).view(np.uint64), stats(d, 0, 0, 1).view(np.uint64))
    c = next(b for b in range(200) if M.flips(seed, b, 3).all())          # and replicate c everything: at n = 3 the additions mirror each other
    assert same_bits(stats(d, 2, seed, 1, first=c), -stats(d, 0, 0, 1))


# ---- the paired test -------------------------------------------------------------------------------------------------------------------

def test_paired_p_value_is_the_mirrors_count():
    rng = np.random.RandomState(12)
    b = rng.rand(12)
    a = b + 0.1 + rng.rand(12)
    diff = a - b
    assert np.all(diff > 0)
    flips, seed = 2000, 2
    null = M.resample_stats(diff, M.SIGN_FLIP, seed, flips)[:, 0]
    observed = M.resample_stats(diff, M.PLAIN, 0, 1)[0, 0]
    rec = R.paired_test(a, b, 500, flips, seed)
    for k, stat in enumerate(R.STATS):
        c = int(np.count_nonzero(np.abs(null[:, k]) >= abs(observed[k])))
        assert c >= 1                  # the seed was chosen so that two replicates flip every sign: the count is not trivially zero
        assert rec[stat]["p"] == (1 + c) / (flips + 1), (stat, c)
        assert rec[stat]["observed"] == observed[k]
    assert (rec["wins"], rec["losses"], rec["ties"], rec["n"]) == (12, 0, 0, 12)
    boot = M.resample_stats(np.stack([a, b, diff]), M.BOOTSTRAP, seed, 500)
    for i, key in enumerate(("a", "b")):
        assert (rec[key]["mean"]["lo"], rec[key]["mean"]["hi"]) == R.percentile_interval(boot[:, i, 0], 0.95)
    assert (rec["median"]["lo"], rec["median"]["hi"]) == R.percentile_interval(boot[:, 2, 1], 0.95)
    assert rec["mean"]["se"] == float(np.std(boot[:, 2, 0], ddof=1))
    zero = R.paired_test(a, a, 50, 99, 1)
    assert zero["mean"]["p"] == zero["median"]["p"] == 1.0 and zero["ties"] == 12


# ---- refusals: each by name, the output untouched --------------------------------------------------------------------------------------

def test_refusals_by_name():
    h, d = series(65)
    big = torch.zeros(1, dtype=torch.float64, device="cuda")      # n = 0 and n = 16385 are refused before anything is read
    for args, words in (((big, 1, 1, 0, 1, 0, 0, 2), "resample_stats: n=0 is outside [1, 16384]"),
                        ((big, 16385, 1, 16385, 1, 0, 0, 2), "resample_stats: n=16385 is outside [1, 16384]"),
                        ((d, 64, 3, 65, 1, 0, 0, 2), "resample_stats: ld=64 is below n=65"),
                        ((d, 65, 0, 65, 1, 0, 0, 2), "resample_stats: S=0 series must be >= 1"),
                        ((d, 65, 3, 65, 3, 0, 0, 2), "resample_stats: mode=3 is unknown"),
                        ((d, 65, 3, 65, -1, 0, 0, 2), "resample_stats: mode=-1 is unknown"),
                        ((d, 65, 3, 65, 0, 0, 0, 2), "resample_stats: mode 0 (plain) has one replicate: first=0, count=2"),
                        ((d, 65, 3, 65, 0, 0, 1, 1), "resample_stats: mode 0 (plain) has one replicate: first=1, count=1"),
                        ((d, 65, 3, 65, 1, 0, 0, -1), "resample_stats: count=-1 replicates must be >= 0"),
                        ((d, 65, 3, 65, 1, 0, -1, 2), "resample_stats: replicates first=-1, count=2 reach outside [0, 2^31]"),
                        ((d, 65, 3, 65, 2, 0, 2 ** 31 - 1, 2), "resample_stats: replicates first=2147483647, count=2 reach outside [0, 2^31]")):
        rc, msg, out = call(*args, words=12)
        assert rc == -22 and words in msg, (args[1:], rc, msg)
        assert out.untouched(), words
    for bad, s, j in ((np.nan, 2, 40), (np.inf, 0, 64), (-np.inf, 1, 0)):
        v = h.copy()
        v[s, j] = bad
        if s < 2:
            v[2, 3] = np.nan       # the first in (series, position) order is the one named
        for mode in (0, 1, 2):
            rc, msg, out = call(torch.from_numpy(v).cuda(), 65, 3, 65, mode, 0, 0, 1)
            assert rc == -22 and f"resample_stats: series {s}, position {j}: the value is NaN or infinite" in msg, (rc, msg)
            assert out.untouched()
    with pytest.raises(_lib.GssError, match=r"series 0, position 1: the value is NaN or infinite"):
        R.bootstrap_summary({"x": [0.5, float("nan"), 1.0]}, 10, 0)
    rc, msg, out = call(d, 65, 3, 65, 1, 0, 5, 0, words=12)      # count = 0 succeeds and writes nothing
    assert rc == 0 and out.untouched()
