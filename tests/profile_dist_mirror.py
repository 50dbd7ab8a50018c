"""Shared by test_profile_dist.py (CPU) and test_gpu_profile_dist.py: csrc/profile_dist.hip's arithmetic in numpy (every sum runs over the
rows 0 .. N - 1 in that order), the fixture of tests/golden/make_profile_dist_fixture.py, the derived tolerances and seeded profiles."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
METRICS = ("cityblock", "euclidean", "canberra", "cosine", "correlation")
DIFF_CLASS = METRICS[:3]
DEGENERATE = np.array([[0, 0, 1, 2], [0, 0, 0, 0], [1, 1, 1, 1], [.5, 0, 1, 2]], dtype=np.float64)

# Tolerances, derived and not measured.  Device and scipy both sum N terms in fp64 in some order; with u = 2^-53 and
# gamma_k = k u / (1 - k u) each side is within gamma_(N + 8) of the exact value (the 8 covers the subtraction, addition, division and
# square root of a term).  So
#   cityblock, euclidean, canberra (sums of non-negative terms):  |device - scipy| <= 4 gamma_(N + 8) * scipy   (twice the two-sided bound):
#     5.3e-14 relative at N = 111, 1.3e-11 at N = 29,960;
#   cosine, correlation (a quotient bounded by 1, by Cauchy-Schwarz): |device - scipy| <= 8 gamma_(N + 8) absolute; the extra factor 2 covers
#     the three sums of the quotient.  An error of a column mean shifts the centred vector by a constant, which enters the dot product and
#     the norm only at second order, so the bound needs no more than mean(|a|) <= 100 std(a), which check_spread asserts on the inputs.
U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


def diff_rel_bound(n):
    return 4.0 * gamma(n + 8)


def dot_abs_bound(n):
    return 8.0 * gamma(n + 8)


def fixture():
    z = np.load(os.path.join(HERE, "golden", "profile_dist_msi_small.npz"))
    return {k: z[k] for k in z.files}


def reference_profiles():
    """-> (names [21], profiles [21][111]) of tests/golden/diffusion_msi_small.npz, the fixture's row / column order"""
    z = np.load(os.path.join(HERE, "golden", "diffusion_msi_small.npz"))
    return [str(s) for s in z["starts"]], np.asarray(z["profiles"], dtype=np.float64)


def mirror(a, b, metric):
    """a [na][N], b [nb][N] -> [na][nb]: sequential sums in row order, the kernels' formulas"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]))
    with np.errstate(invalid="ignore", divide="ignore"):
        if metric in DIFF_CLASS:
            for k in range(n):
                x, y = a[:, k, None], b[None, :, k]
                if metric == "cityblock":
                    acc += np.abs(x - y)
                elif metric == "euclidean":
                    acc += (x - y) * (x - y)
                else:
                    den = np.abs(x) + np.abs(y)
                    acc += np.where(den > 0, np.abs(x - y) / np.where(den > 0, den, 1.0), 0.0)
            return np.sqrt(acc) if metric == "euclidean" else acc
        if metric not in ("cosine", "correlation"):
            raise ValueError(metric)
        if metric == "correlation":
            def centre(v):
                s = np.zeros(v.shape[0])
                for k in range(n):
                    s += v[:, k]
                return v - (s / n)[:, None]
            a, b = centre(a), centre(b)
        na2, nb2 = np.zeros(a.shape[0]), np.zeros(b.shape[0])
        for k in range(n):
            acc += a[:, k, None] * b[None, :, k]
            na2 += a[:, k] * a[:, k]
            nb2 += b[:, k] * b[:, k]
        cs = acc / (np.sqrt(na2)[:, None] * np.sqrt(nb2)[None, :])
        cs = np.where(np.abs(cs) > 1.0, np.copysign(1.0, cs), cs)
        return 1.0 - cs


def check_spread(profiles):
    """the condition of the dot-class bound on the inputs: mean(|a|) <= 100 std(a) for every profile that is not constant"""
    p = np.asarray(profiles, np.float64)
    std = p.std(axis=1)
    live = std > 0
    assert np.all(np.abs(p[live]).mean(axis=1) <= 100.0 * std[live])


def compare(got, want, metric, n):
    """asserts the NaN positions equal and the finite entries within the derived bound -> the measured maximum in units of the bound"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (metric, np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    err = np.abs(got[ok] - want[ok])
    if metric in DIFF_CLASS:
        bound = diff_rel_bound(n) * np.abs(want[ok])
        worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    else:
        worst = float(err.max() / dot_abs_bound(n))
    assert worst <= 1.0, (metric, n, worst)
    return worst


def synthetic(seed, k, n, lognormal=False):
    """k seeded profiles of n entries: non-negative, one tenth of the entries exactly zero (Canberra's rule), normalised to sum 1"""
    rng = np.random.RandomState(seed)
    p = rng.lognormal(0.0, 2.0, size=(k, n)) if lognormal else rng.rand(k, n)
    p[rng.rand(k, n) < 0.1] = 0.0
    s = p.sum(axis=1, keepdims=True)
    return p / np.where(s > 0, s, 1.0)


def nearest(dist, row_ids, col_ids, top):
    """the host selection compare_profiles.py makes: per row the `top` nearest columns, ties by column position, a row's own id never
    listed -> [(row id, rank from 1, column id, distance)]"""
    out = []
    for i, r in enumerate(row_ids):
        order = [j for j in np.argsort(dist[i], kind="stable") if col_ids[j] != r][:top]
        out += [(r, k + 1, col_ids[j], float(dist[i][j])) for k, j in enumerate(order)]
    return out
