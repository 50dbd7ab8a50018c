"""GPU: csrc/matrix_mantel.hip (gss_matrix_cross_sums) through mantel.cross_sums / observed_cross_sum / mantel, against the numpy mirror
(mantel_mirror.py).

Permutations are integers: equal to the mirror's np.lexsort((i, key)) exactly.
Bits: the kernel's order of additions is stated in include/gssgcn.h and restated term by term in the mirror (ordered_cross_sum) on signed
matrices; the device's sums equal it bit for bit, and hence each other under every cut of a call and every row stride.
Accuracy at the largest size, where the term-by-term mirror is slow: a sum of K signed terms added in any order is within gamma(K) * sum
|terms| of the exact sum, gamma(k) = k u / (1 - k u), u = 2^-53.
r: the correlation of the pair values as scipy computes it, within 2 gamma(4 K) -- the mean, the norm and the cross-sum each contribute at
most gamma_K on values of magnitude <= 1, on either side of the comparison."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mantel_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import _lib  # noqa: E402
from gcn_drug_repurposing_amd import mantel as MT  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES_N = (2, 3, 5, 64, 65, 66, 129, 257)
_MATRICES = {}


def matrices(n):
    """two signed symmetric matrices of n rows with zero diagonals -> (host a, host b, device a, device b); made once per n, never written"""
    if n not in _MATRICES:
        rng = np.random.RandomState(2000 + n)
        pair = []
        for _ in range(2):
            h = np.triu(rng.randn(n, n), 1)
            pair.append(h + h.T)
        _MATRICES[n] = (pair[0], pair[1], torch.from_numpy(pair[0]).cuda(), torch.from_numpy(pair[1]).cuda())
    return _MATRICES[n]


def host(t):
    return t.cpu().numpy()


def bits(x):
    return np.atleast_1d(np.asarray(x, dtype=np.float64)).view(np.uint64)


def same(x, y):
    """equal bit for bit"""
    return np.array_equal(bits(x), bits(y))


# ---- bits and permutations against the mirror ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES_N)
def test_sums_and_permutations_equal_the_mirror(n):
    ha, hb, da, db = matrices(n)
    seed = 2 ** 63 + 11
    plain = host(MT.observed_cross_sum(da, db))
    assert plain.shape == (1,) and same(plain, M.ordered_cross_sum(ha, hb))
    sums, perm = MT.cross_sums(da, db, 3, seed=seed, perms=True)
    sums, perm = host(sums), host(perm)
    assert sums.shape == (3,) and perm.shape == (3, n) and perm.dtype == np.int32
    for s in range(3):
        want = M.permutation(seed, s, n)
        assert np.array_equal(perm[s], want), (n, s)
        assert same(sums[s], M.ordered_cross_sum(ha, hb, want)), (n, s, sums[s])
    later = host(MT.cross_sums(da, db, 1, seed=seed, first=12345))
    assert same(later, M.ordered_cross_sum(ha, hb, M.permutation(seed, 12345, n)))


def test_outputs_end_where_they_should():
    """count replicates write count sums and count * n permutation entries, and nothing behind them"""
    n, count = 66, 5
    _, _, da, db = matrices(n)
    out = torch.full((count + 8,), -7.0, dtype=torch.float64, device="cuda")
    perm = torch.full((count * n + 64,), -7, dtype=torch.int32, device="cuda")
    lib = _lib.load()
    _lib.check(lib.gss_matrix_cross_sums(n, da.data_ptr(), n, db.data_ptr(), n, 1, 3, 2, count, out.data_ptr(), perm.data_ptr(), _lib.current_stream()))
    sums, perm = host(out), host(perm)
    assert np.all(sums[count:] == -7.0) and np.all(perm[count * n:] == -7)
    assert same(sums[:count], host(MT.cross_sums(da, db, count, seed=3, first=2)))
    assert np.array_equal(perm[:count * n].reshape(count, n), np.stack([M.permutation(3, 2 + s, n) for s in range(count)]))
    ident = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.gss_matrix_cross_sums(n, da.data_ptr(), n, db.data_ptr(), n, 0, 3, 0, 1, out.data_ptr(), ident.data_ptr(), _lib.current_stream()))
    assert np.array_equal(host(ident)[:n], np.arange(n)) and np.all(host(ident)[n:] == -7)
    assert same(host(out)[:1], host(MT.observed_cross_sum(da, db))) and same(host(out)[1:], sums[1:])


@pytest.mark.parametrize("n", (65, 257))
def test_sums_do_not_depend_on_how_a_call_is_cut(n):
    _, _, da, db = matrices(n)
    whole = host(MT.cross_sums(da, db, 10, seed=9))
    cut = np.concatenate([host(MT.cross_sums(da, db, 3, seed=9)), host(MT.cross_sums(da, db, 7, seed=9, first=3))])
    single = np.concatenate([host(MT.cross_sums(da, db, 1, seed=9, first=s)) for s in range(10)])
    assert same(whole, cut) and same(whole, single)
    assert len(set(bits(whole).tolist())) == 10


@pytest.mark.parametrize("n", (5, 129))
def test_row_strides_do_not_change_the_bits(n):
    ha, hb, da, db = matrices(n)
    wide_a = torch.full((n, n + 3), 99.0, dtype=torch.float64, device="cuda")
    wide_b = torch.full((n, 2 * n + 1), -99.0, dtype=torch.float64, device="cuda")
    wide_a[:, :n], wide_b[:, :n] = da, db
    va, vb = wide_a[:, :n], wide_b[:, :n]
    assert va.stride(0) == n + 3 and vb.stride(0) == 2 * n + 1
    assert same(host(MT.cross_sums(va, vb, 4, seed=1)), host(MT.cross_sums(da, db, 4, seed=1)))
    assert same(host(MT.observed_cross_sum(va, vb)), host(MT.observed_cross_sum(da, db)))
    assert same(host(MT.observed_cross_sum(ha, hb)), host(MT.observed_cross_sum(da, db)))      # host arrays are uploaded


def test_the_largest_size_against_numpy():
    n, seed = 4096, 4
    K = n * (n - 1) // 2
    assert K == 8386560
    ha, hb, da, db = matrices(n)
    sums, perm = MT.cross_sums(da, db, 2, seed=seed, perms=True)
    sums, perm = host(sums), host(perm)
    low = np.tril(ha, -1)
    for s in range(2):
        assert np.array_equal(perm[s], M.permutation(seed, s, n))
        terms = low * hb[perm[s]][:, perm[s]]
        want, scale = float(np.sum(terms)), float(np.sum(np.abs(terms)))
        print(f"n={n} s={s} |got - numpy| / bound = {abs(sums[s] - want) / (M.gamma(K) * scale):.3g}")
        assert abs(sums[s] - want) <= M.gamma(K) * scale, (s, sums[s], want)
    plain = float(host(MT.observed_cross_sum(da, db))[0])
    terms = low * hb
    assert abs(plain - float(np.sum(terms))) <= M.gamma(K) * float(np.sum(np.abs(terms)))
    del _MATRICES[n]


# ---- mantel() ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (4, 12))
@pytest.mark.parametrize("method", MT.METHODS)
def test_a_matrix_against_itself(n, method):
    """r = 1, and the replicates that tie it are exactly the identity permutations: the same additions give the same bits"""
    ha, _, da, _ = matrices(n) if n == 12 else matrices(5)
    ha, da = ha[:n, :n], da[:n, :n].contiguous()
    S, seed, K = 200, 6, n * (n - 1) // 2
    rec, null = MT.mantel(da, da, method=method, permutations=S, seed=seed, return_null=True)
    identities = sum(1 for s in range(S) if np.array_equal(M.permutation(seed, s, n), np.arange(n)))
    assert (identities > 0) == (n == 4)
    assert rec["n"] == n and rec["n_pairs"] == K and abs(rec["r"] - 1) <= M.gamma(K)
    assert rec["p_greater"] == (1 + identities) / (S + 1) and int(np.count_nonzero(null == rec["r"])) == identities


@pytest.mark.parametrize("method", MT.METHODS)
def test_mantel_equals_its_parts(method):
    import scipy.stats
    n, S, seed = 12, 200, 8
    ha, hb, da, db = matrices(n)
    labels = [f"D{i}" for i in range(n)]
    rec, null = MT.mantel(da, db, method=method, permutations=S, seed=seed, labels=labels, return_null=True)
    assert MT.mantel(ha, hb, method=method, permutations=S, seed=seed) == rec                                  # host arrays, no null asked for
    K = n * (n - 1) // 2
    iu = np.triu_indices(n, 1)
    want = (scipy.stats.spearmanr if method == "spearman" else scipy.stats.pearsonr)(ha[iu], hb[iu])[0]
    assert abs(rec["r"] - want) <= 2 * M.gamma(4 * K), (rec["r"], want)
    # the kernel on the standardised matrices, bit for bit
    sa, sb = host(MT.standardise_pairs(da, method)), host(MT.standardise_pairs(db, method))
    for h, m in ((ha, sa), (hb, sb)):
        assert np.array_equal(m, m.T) and not m.diagonal().any() and np.max(np.abs(m - M.standardised(h, method))) <= M.gamma(4 * K)
    assert same(rec["r"], M.ordered_cross_sum(sa, sb))
    assert null.shape == (S,) and all(same(null[s], M.ordered_cross_sum(sa, sb, M.permutation(seed, s, n))) for s in range(S))
    # the statistics with the host statements of the definition
    nm, ns = float(np.mean(null)), float(np.std(null, ddof=0))
    assert rec == {"n": n, "n_pairs": K, "r": rec["r"], "null_mean": nm, "null_std": ns, "z": (rec["r"] - nm) / ns,
                   "p_greater": (1 + sum(1 for t in null if t >= rec["r"])) / (S + 1),
                   "p_two_sided": (1 + sum(1 for t in null if abs(t) >= abs(rec["r"]))) / (S + 1)}
    assert abs(nm) < 5 / np.sqrt(K) and 0 < ns < 1                   # a null of correlations: centred near 0


def test_spearman_ranks_the_ties():
    """rounded matrices: the pair values tie, the ranks are average ranks"""
    import scipy.stats
    n = 12
    ha, hb, _, _ = matrices(n)
    ra, rb = np.round(ha), np.round(2 * hb) / 2
    iu = np.triu_indices(n, 1)
    assert len(set(ra[iu])) < len(ra[iu])
    rec = MT.mantel(ra, rb, method="spearman", permutations=20, seed=1)
    assert abs(rec["r"] - scipy.stats.spearmanr(ra[iu], rb[iu])[0]) <= 2 * M.gamma(4 * len(iu[0]))
    _, v = MT.pair_values(torch.from_numpy(ra).cuda())
    assert np.array_equal(host(MT.pair_ranks(v)), scipy.stats.rankdata(ra[iu]))


# ---- refusals of the Python layer ----------------------------------------------------------------------------------------------------

def test_python_refusals():
    ha, hb, da, db = matrices(5)
    labels = ["DA", "DB", "DC", "DD", "DE"]
    skew = ha.copy()
    skew[3, 1] += 1e-9
    with pytest.raises(ValueError, match="mantel: b is not symmetric"):
        MT.mantel(da, skew, permutations=5)
    with pytest.raises(ValueError, match="cross_sums: a is not symmetric"):
        MT.cross_sums(skew, db, 5)
    hole = hb.copy()
    hole[2, 4] = hole[4, 2] = np.nan
    with pytest.raises(ValueError, match="'DC' is NaN"):
        MT.mantel(da, hole, permutations=5, labels=labels)
    with pytest.raises(ValueError, match="'row 2' is NaN"):
        MT.observed_cross_sum(hole, db)
    with pytest.raises(ValueError, match="n=2 drugs give 1 pair"):
        MT.mantel(ha[:2, :2], hb[:2, :2], permutations=5)
    flat = np.full((5, 5), 0.5)
    np.fill_diagonal(flat, 0.0)
    for method in MT.METHODS:
        with pytest.raises(ValueError, match="pair values of b are constant"):
            MT.mantel(da, flat, method=method, permutations=5)
    with pytest.raises(ValueError, match="a is 5 x 5 and b 3 x 3"):
        MT.cross_sums(da, hb[:3, :3], 5)
    with pytest.raises(_lib.GssError, match="n=4097 is outside"):
        MT.cross_sums(np.zeros((4097, 4097)), np.zeros((4097, 4097)), 1)
