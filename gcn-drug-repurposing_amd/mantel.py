"""Mantel's test between two drug x drug matrices: is the correlation of their n (n - 1) / 2 pair values larger than relabelling the drugs of
one matrix leaves it?  The pairs share drugs, so they are not independent and the p-value of a plain correlation test is wrong; the null
here is the correlation under S seeded permutations of one matrix's rows and columns.  It answers the multiscale interactome's question
about the Connectivity Map signatures (signatures.py, drug_signatures.py), and compares any two matrices over the same drugs: two profile
metrics, a chemical or a side-effect similarity.

Both matrices are standardised once (standardise_pairs: the upper-triangle values, or their average-tie ranks for Spearman, centred and
scaled to unit norm); after that the cross-product sum over the pairs IS the correlation r, and because a relabelling keeps the multiset
of pair values -- and so the mean and the norm -- the permuted cross-product sums are the null's r_s with no further work.  The sums are a
HIP kernel (csrc/matrix_mantel.hip, gss_matrix_cross_sums; no CPU fallback): one workgroup per permutation, in a fixed order of additions,
so that r and every r_s are bit-reproducible and a permutation equal to the identity ties r exactly.  What comes back is [S] sums; mean,
standard deviation, z and the two empirical p-values over them are host numpy."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._nulls import chunked_null, square_matrix

MAX_N = 4096                  # gss_matrix_cross_sums sorts a replicate's permutation in LDS
METHODS = ("pearson", "spearman")


# ---- the kernel ----------------------------------------------------------------------------------------------------------------------

def _symmetric(m, who, name, labels=None):
    """square_matrix plus exact symmetry: the kernel reads both triangles of the permuted matrix"""
    import torch
    d = square_matrix(m, who, labels)
    if not torch.equal(d, d.T):
        raise ValueError(f"{who}: {name} is not symmetric (it must equal its transpose exactly)")
    return d


def _pair(a, b, who, labels=None):
    da, db = _symmetric(a, who, "a", labels), _symmetric(b, who, "b", labels)
    if da.shape != db.shape:
        raise ValueError(f"{who}: a is {da.shape[0]} x {da.shape[0]} and b {db.shape[0]} x {db.shape[0]}")
    if da.device != db.device:
        raise ValueError(f"{who}: a is on {da.device} and b on {db.device}")
    return da, db


def _cross_sums(da, db, mode, seed, first, count, perms):
    import torch
    n = da.shape[0]
    with torch.cuda.device(da.device):
        out = torch.empty(max(count, 0), dtype=torch.float64, device=da.device)
        perm = torch.empty(max(count, 0), n, dtype=torch.int32, device=da.device) if perms else None
        _lib.check(_lib.load().gss_matrix_cross_sums(n, da.data_ptr(), _lib.row_stride(da), db.data_ptr(), _lib.row_stride(db), mode,
                                                     _lib.seed64(seed), int(first), count, out.data_ptr(), _lib.ptr(perm), _lib.current_stream()),
                   "gss_matrix_cross_sums")
    return (out, perm) if perms else out


def cross_sums(a, b, samples, seed=0, first=0, perms=False, labels=None):
    """the permuted cross-product sums of two symmetric matrices -> device tensor fp64 [samples]: entry s - first = the sum over i < j of
    a[j][i] * b[pi_s(j)][pi_s(i)] for permutation number s = first .. first + samples - 1 of the n rows (gss_matrix_cross_sums: rows sorted
    by the counter-based key of (seed, s, row), a pure function of its arguments -- a call equals the same replicates in any split through
    `first`).  a, b: square device fp64 tensors, used in place (a row stride above n is honoured), or host arrays, uploaded; 2 <= n <= 4096.
    A NaN is refused with the row's label (labels[i], else its number), a matrix that is not exactly symmetric by name.  perms=True also
    returns the permutations, device int32 [samples][n].  No CPU fallback."""
    da, db = _pair(a, b, "cross_sums", labels)
    return _cross_sums(da, db, 1, seed, first, int(samples), perms)


def observed_cross_sum(a, b, labels=None):
    """the same sum under the identity, with the additions of the null -> device tensor fp64 [1] (mode 0 of gss_matrix_cross_sums)"""
    da, db = _pair(a, b, "observed_cross_sum", labels)
    return _cross_sums(da, db, 0, 0, 0, 1, False)


def null_cross_sums(a, b, samples, seed=0):
    """cross_sums brought to the host -> fp64 [samples], in calls of at most NULL_CHUNK_BYTES of sums each"""
    return chunked_null(lambda count, first: cross_sums(a, b, count, seed, first), samples, 8)


# ---- the standardisation (device) ----------------------------------------------------------------------------------------------------

def check_method(method, who="mantel"):
    if method not in METHODS:
        raise ValueError(f"{who}: method {method!r} is unknown; choose one of {', '.join(METHODS)}")


def pair_values(d):
    """the K = n (n - 1) / 2 values d[i][j], i < j, row after row, of a device matrix -> (device int64 [2][K] of (i, j), device fp64 [K])"""
    import torch
    n = d.shape[0]
    iu = torch.triu_indices(n, n, 1, device=d.device)
    return iu, d[iu[0], iu[1]].contiguous()


def pair_ranks(v):
    """scipy.stats.rankdata(v, method="average") of a device fp64 vector, exactly -> device fp64 [K] (diffusion.rank_profiles)"""
    from .diffusion import rank_profiles
    return rank_profiles(v.view(-1, 1), None, device=v.device)[:, 0].contiguous()


def standardise_pairs(d, method, labels=None, name="d"):
    """a symmetric matrix -> the symmetric device fp64 matrix [n][n] with a zero diagonal whose K upper-triangle values are those of d
    (method "pearson") or their average-tie ranks ("spearman"), centred and scaled to unit Euclidean norm.  The cross-product sum of two
    such matrices over the pairs is the correlation of their pair values.  Constant values (a zero norm) are refused."""
    import torch
    check_method(method, "standardise_pairs")
    d = _symmetric(d, "standardise_pairs", name, labels)
    n = d.shape[0]
    if n < 2:
        raise ValueError(f"standardise_pairs: {name} has {n} row: there is no pair")
    iu, v = pair_values(d)
    if bool(v.min() == v.max()):
        raise ValueError(f"standardise_pairs: the {v.numel()} pair values of {name} are constant: they have no correlation with anything")
    if method == "spearman":
        v = pair_ranks(v)
    v = v - v.mean()
    v = v / torch.sqrt((v * v).sum())
    out = torch.zeros(n, n, dtype=torch.float64, device=d.device)
    out[iu[0], iu[1]] = v
    out[iu[1], iu[0]] = v
    return out


# ---- the statistics (host) -----------------------------------------------------------------------------------------------------------

def mantel_stats(r, null):
    """the observed r against the null's r_s [S]: null_mean and null_std = np.mean and np.std (ddof 0), z = (r - null_mean) / null_std (nan
    when the std is 0), p_greater = (1 + #{s: r_s >= r}) / (S + 1) and p_two_sided = (1 + #{s: |r_s| >= |r|}) / (S + 1), counted on the sums
    themselves -> a dict"""
    r, null = float(r), np.asarray(null, dtype=np.float64).reshape(-1)
    nm, ns = float(np.mean(null)), float(np.std(null))
    return {"r": r, "null_mean": nm, "null_std": ns, "z": (r - nm) / ns if ns > 0 else float("nan"),
            "p_greater": (1 + int(np.count_nonzero(null >= r))) / (len(null) + 1),
            "p_two_sided": (1 + int(np.count_nonzero(np.abs(null) >= abs(r)))) / (len(null) + 1)}


def mantel(a, b, method="spearman", permutations=10000, seed=0, labels=None, return_null=False):
    """Mantel's test of two symmetric matrices over the same n >= 3 drugs -> {"n", "n_pairs", "r", "null_mean", "null_std", "z",
    "p_greater", "p_two_sided"} (mantel_stats): r = the Pearson correlation of the n (n - 1) / 2 pair values, or of their average-tie ranks
    (method "spearman"), as mode 0 of the kernel adds it; the null = the same sum under `permutations` seeded relabellings of b.  a, b and
    labels as in cross_sums.  return_null=True: -> (the dict, the null r_s [permutations] on the host).  No CPU fallback."""
    check_method(method)
    S = int(permutations)
    if S < 1:
        raise ValueError(f"mantel: permutations={permutations} must be at least 1")
    da, db = _pair(a, b, "mantel", labels)
    n = da.shape[0]
    if n < 3:
        raise ValueError(f"mantel: n={n} drugs give {n * (n - 1) // 2} pair: a correlation needs at least 3 drugs")
    if n > MAX_N:
        raise ValueError(f"mantel: n={n} is above {MAX_N}, the most a permutation is drawn over")
    sa, sb = standardise_pairs(da, method, labels, "a"), standardise_pairs(db, method, labels, "b")
    r = float(_cross_sums(sa, sb, 0, 0, 0, 1, False)[0])
    null = null_cross_sums(sa, sb, S, seed)
    rec = {"n": n, "n_pairs": n * (n - 1) // 2, **mantel_stats(r, null)}
    return (rec, null) if return_null else rec
