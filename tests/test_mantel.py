"""CPU: the host half of Mantel's test between two drug x drug matrices (mantel.py, signatures.py) and the mirror the GPU tests hold the
kernel to (mantel_mirror.py): the entry point's place in the header, the library and the binding with its argument-only refusals, the
mirror's correlation against scipy, the signature table's parsing on the head of the reference's table, the p-value arithmetic on hand-made
nulls, and the program's refusals."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mantel_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import mantel as MT  # noqa: E402
from gcn_drug_repurposing_amd import signatures as SG  # noqa: E402
from gcn_drug_repurposing_amd.predict import PredictError  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "bcm_signatures_head.tsv")


def symmetric(n, seed, decimals=None):
    """a seeded signed symmetric matrix with a zero diagonal; rounded to `decimals`, its pair values tie"""
    a = np.random.RandomState(seed).randn(n, n)
    a = np.round(a, decimals) if decimals is not None else a
    a = np.triu(a, 1)
    return a + a.T


# ---- the entry point in the header, the library and the binding ----------------------------------------------------------------------

def test_abi_25_carries_the_cross_sums():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    lib = pkg.load()
    header = open(os.path.join(ROOT, "include", "gssgcn.h")).read()
    assert pkg._lib.ABI_VERSION == lib.gss_abi_version() == 25 and "#define GSS_ABI_VERSION 25 " in header
    assert re.search(r"\bint gss_matrix_cross_sums\(int32_t n, const double \*a, int64_t lda, const double \*b, int64_t ldb, int32_t mode, uint64_t seed, "
                     r"int64_t first,\s+int64_t count, double \*out, int32_t \*perm_out, void \*stream\);", header)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    assert " T gss_matrix_cross_sums\n" in out
    restype, argtypes = pkg._lib.SIGNATURES["gss_matrix_cross_sums"]
    assert restype is C.c_int and [C.sizeof(t) for t in argtypes] == [4, 8, 8, 8, 8, 4, 8, 8, 8, 8, 8, 8] and argtypes[6] is C.c_uint64
    assert lib.gss_matrix_cross_sums.argtypes == argtypes
    rng_h = open(os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc", "counter_rng.h")).read()
    assert f"kRngMantelPerm = {M.TAG_MANTEL_PERM}," in rng_h and M.TAG_MANTEL_PERM == 12
    # the refusals that need no device: the arguments alone (n, a, lda, b, ldb, mode, seed, first, count, out, perm_out, stream); a pointer
    # that is not null is never read before the last refusal
    some = 8
    for args, words in (((1, 0, 5, 0, 5, 1, 0, 0, 1, 0, 0, 0), "n=1 is outside [2, 4096]"), ((4097, 0, 4097, 0, 4097, 1, 0, 0, 1, 0, 0, 0), "n=4097 is outside"),
                        ((5, 0, 4, 0, 5, 1, 0, 0, 1, 0, 0, 0), "lda=4 is below n=5"), ((5, 0, 5, 0, 4, 1, 0, 0, 1, 0, 0, 0), "ldb=4 is below n=5"),
                        ((5, 0, 5, 0, 5, 2, 0, 0, 1, 0, 0, 0), "mode=2 is unknown"), ((5, 0, 5, 0, 5, -1, 0, 0, 1, 0, 0, 0), "mode=-1 is unknown"),
                        ((5, 0, 5, 0, 5, 0, 0, 0, 2, 0, 0, 0), "mode 0 (plain) has one replicate"),
                        ((5, 0, 5, 0, 5, 0, 0, 0, 0, 0, 0, 0), "mode 0 (plain) has one replicate"),
                        ((5, 0, 5, 0, 5, 1, 0, 0, -1, 0, 0, 0), "count=-1 replicates must be >= 0"),
                        ((5, 0, 5, 0, 5, 1, 0, -1, 1, 0, 0, 0), "reach outside [0, 2^31]"), ((5, 0, 5, 0, 5, 1, 0, 2 ** 31, 1, 0, 0, 0), "reach outside [0, 2^31]"),
                        ((5, 0, 5, 0, 5, 1, 0, 2 ** 31 - 3, 4, 0, 0, 0), "reach outside [0, 2^31]"),
                        ((5, 0, 5, some, 5, 1, 0, 0, 1, some, 0, 0), "a is null"), ((5, some, 5, 0, 5, 1, 0, 0, 1, some, 0, 0), "b is null"),
                        ((5, some, 5, some, 5, 1, 0, 0, 1, 0, 0, 0), "out is null")):
        assert lib.gss_matrix_cross_sums(*args) == -22 and words in lib.gss_last_error().decode(), words
    assert lib.gss_matrix_cross_sums(5, 0, 5, 0, 5, 1, 0, 7, 0, 0, 0, 0) == 0      # count = 0: nothing to do, nothing read


def test_sort_pairs_is_stated_once():
    """class_cohesion.hip and matrix_mantel.hip share rank_keys.h's sort_pairs"""
    csrc = os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc")
    defined = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and re.search(r"\bvoid sort_pairs\(", open(os.path.join(csrc, f)).read())]
    assert defined == ["rank_keys.h"]
    for f in ("class_cohesion.hip", "matrix_mantel.hip"):
        assert "sort_pairs<" in open(os.path.join(csrc, f)).read()


# ---- the mirror ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (2, 3, 65, 130))
def test_mirror_permutation_and_sum(n):
    A, B = symmetric(n, n), symmetric(n, n + 100)
    K = n * (n - 1) // 2
    for s in range(3):
        pi = M.permutation(5, s, n)
        assert sorted(pi) == list(range(n))
        got, exact = M.ordered_cross_sum(A, B, pi), M.fsum_cross_sum(A, B, pi)
        scale = sum(float(np.sum(np.abs(M.row_terms(A, B, pi, j)))) for j in range(1, n))
        assert abs(got - exact) <= M.gamma(K) * scale
    assert M.ordered_cross_sum(A, B) == M.ordered_cross_sum(A, B, np.arange(n))
    if n > 3:
        assert not np.array_equal(M.permutation(5, 0, n), M.permutation(5, 1, n)) and not np.array_equal(M.permutation(5, 0, n), M.permutation(6, 0, n))


def test_mirror_row_sum_is_the_stated_order():
    t = np.random.RandomState(2).randn(150)
    p = [0.0] * 64
    for i, x in enumerate(t):
        p[i % 64] = p[i % 64] + x                       # lane-strided, ascending, from +0.0
    for o in (32, 16, 8, 4, 2, 1):
        p = [p[l] + p[l ^ o] for l in range(64)]
    assert M.ordered_row_sum(t) == p[0]
    assert M.ordered_row_sum(np.array([-0.0])) == 0.0 and math.copysign(1.0, M.ordered_row_sum(np.array([-0.0]))) == 1.0


@pytest.mark.parametrize("n", (3, 12, 63))
@pytest.mark.parametrize("method", MT.METHODS)
def test_mirror_correlation_is_scipys(n, method):
    """standardise, then add the cross products = the correlation of the upper triangles.  The bound is derived: the mean, the norm and the
    cross-sum each contribute at most gamma_K on values of magnitude <= 1, on either side of the comparison"""
    import scipy.stats
    K = n * (n - 1) // 2
    iu = np.triu_indices(n, 1)
    for A, B in ((symmetric(n, 1), symmetric(n, 2)), (symmetric(n, 3, decimals=0), symmetric(n, 4, decimals=1)), (symmetric(n, 5), symmetric(n, 5))):
        if np.ptp(A[iu]) == 0 or np.ptp(B[iu]) == 0:
            continue                                     # constant pair values have no correlation (n = 3, rounded)
        want = (scipy.stats.spearmanr if method == "spearman" else scipy.stats.pearsonr)(A[iu], B[iu])[0]
        got = M.correlation(A, B, method)
        assert abs(got - want) <= 2 * M.gamma(4 * K), (n, method, got, want)
    assert np.array_equal(M.average_ranks(np.array([3.0, 1.0, 3.0, 2.0, 3.0])), scipy.stats.rankdata([3.0, 1.0, 3.0, 2.0, 3.0]))
    S = M.standardised(symmetric(n, 3, decimals=0) if n > 3 else symmetric(n, 1), method)
    assert np.array_equal(S, S.T) and not S.diagonal().any() and abs(float(np.sum(S[iu] ** 2)) - 1) <= M.gamma(2 * K)


# ---- the signature table -------------------------------------------------------------------------------------------------------------

def test_read_signatures_on_the_head_of_the_reference_table():
    drugs, names, genes, table = SG.read_signatures(FIXTURE)
    lines = [l.rstrip("\n").split("\t") for l in open(FIXTURE, encoding="utf-8")]
    assert lines[0][:6] == ["drug", "drug_name", "sig_id", "cell", "dose", "time"] and len(lines) == 6
    assert drugs == [l[0] for l in lines[1:]] and drugs[:3] == ["DB00970", "DB01243", "DB00242"]
    assert names == {l[0]: l[1] for l in lines[1:]} and names["DB00970"] == "dactinomycin"
    assert genes == lines[0][6:] and genes[:4] == ["2597", "1677", "81544", "3611"] and len(genes) == 16
    assert table.shape == (5, 16) and table.dtype == np.float64
    assert np.array_equal(table, np.array([[float(c) for c in l[6:]] for l in lines[1:]]))
    assert table[0, 0] == 0.114158146 and table[1, 0] == 0.0 and table[0, 3] == 3.5280883


def write_table(path, head, rows):
    path.write_text("\t".join(head) + "\n" + "".join("\t".join(r) + "\n" for r in rows))
    return str(path)


def test_read_signatures_refusals_and_replicates(tmp_path):
    head = ["drug", "drug_name", "cell", "11", "7", "gene9"]
    rows = [["D1", "one", "A", "1.0", "2.0", "x"], ["D2", "two", "A", "-1.5", "0.25", "x"], ["D1", "one", "B", "3.0", "1.0", "x"]]
    with pytest.raises(PredictError, match="column 'drug' is missing"):
        SG.read_signatures(write_table(tmp_path / "a.tsv", ["id"] + head[1:], rows))
    with pytest.raises(PredictError, match="no gene column"):
        SG.read_signatures(write_table(tmp_path / "b.tsv", ["drug", "drug_name", "cell", "g1", "g2", "gene9"], rows))
    with pytest.raises(PredictError, match="drug 'D2', gene 7: 'n/a' is not a number"):
        SG.read_signatures(write_table(tmp_path / "c.tsv", head, [rows[0], ["D2", "two", "A", "-1.5", "n/a", "x"]]))
    with pytest.raises(PredictError, match="drug 'D2', gene 11: '' is not a number"):
        SG.read_signatures(write_table(tmp_path / "d.tsv", head, [rows[0], ["D2", "two", "A", "", "1", "x"]]))
    with pytest.raises(PredictError, match="drug 'D1' has 2 rows"):
        SG.read_signatures(write_table(tmp_path / "e.tsv", head, rows))
    drugs, names, genes, table = SG.read_signatures(str(tmp_path / "e.tsv"), "mean")
    assert drugs == ["D1", "D2"] and names == {"D1": "one", "D2": "two"} and genes == ["11", "7"]
    assert np.array_equal(table, np.array([[2.0, 1.5], [-1.5, 0.25]]))
    drugs, names, _, _ = SG.read_signatures(write_table(tmp_path / "f.tsv", ["drug", "5"], [["D3", "1"], ["D4", "2"]]))
    assert drugs == ["D3", "D4"] and names == {"D3": "", "D4": ""}                      # drug_name is optional


def test_pool_is_the_tables_drugs_with_a_profile_in_node_order():
    g = types.SimpleNamespace(adj={n: {} for n in ("D4", "D3", "D2", "D1", "P1")})      # D9 is no node
    pool, no_node, no_profile = SG.pool_of(["D1", "D9", "D2", "D3", "D4"], ["P1", "D4", "D3", "D2", "D1"], {"D1": None, "D3": None, "D4": None}, g)
    assert pool == ["D4", "D3", "D1"] and no_node == ["D9"] and no_profile == ["D2"]


# ---- the statistics ------------------------------------------------------------------------------------------------------------------

def test_statistics_on_hand_made_nulls():
    null = np.array([-0.5, -0.25, 0.0, 0.25, 0.25, 0.5, 0.75, -0.75])
    rec = MT.mantel_stats(0.25, null)
    assert rec["r"] == 0.25 and rec["p_greater"] == (1 + 4) / 9 and rec["p_two_sided"] == (1 + 7) / 9          # ties count
    assert rec["null_mean"] == float(np.mean(null)) and rec["null_std"] == float(np.std(null, ddof=0))
    assert rec["z"] == (0.25 - float(np.mean(null))) / float(np.std(null, ddof=0))
    rec = MT.mantel_stats(-0.6, null)
    assert rec["p_greater"] == (1 + 7) / 9 and rec["p_two_sided"] == (1 + 2) / 9                               # |r_s| >= 0.6: 0.75 and -0.75
    rec = MT.mantel_stats(2.0, null)
    assert rec["p_greater"] == rec["p_two_sided"] == 1 / 9                                                     # never below 1 / (S + 1)
    flat = MT.mantel_stats(0.3, np.full(5, 0.1))
    assert flat["null_std"] == 0.0 and math.isnan(flat["z"]) and flat["p_greater"] == 1 / 6
    assert MT.mantel_stats(0.1, np.full(5, 0.1))["p_greater"] == 1.0


def test_python_refusals_before_the_gpu():
    with pytest.raises(ValueError, match="method 'kendall' is unknown"):
        MT.mantel(np.zeros((3, 3)), np.zeros((3, 3)), method="kendall")
    with pytest.raises(ValueError, match="permutations=0 must be at least 1"):
        MT.mantel(np.zeros((3, 3)), np.zeros((3, 3)), permutations=0)
    with pytest.raises(ValueError, match="must be square"):
        MT.cross_sums(np.zeros((3, 4)), np.zeros((3, 3)), 1)


# ---- the program ---------------------------------------------------------------------------------------------------------------------

def test_program_refusals_exit_2_with_one_line(tmp_path, capsys):
    for argv, words in ((["--method", "kendall"], "--method 'kendall' is unknown"), (["--metric", "hamming"], "--metric 'hamming' is unknown"),
                        (["--signature-metric", "hamming"], "--signature-metric 'hamming' is unknown"),
                        (["--permutations", "0"], "--permutations 0 must be at least 1"), (["--replicates", "median"], "--replicates 'median' is unknown"),
                        (["-c", str(tmp_path / "none.json")], "none.json")):
        with pytest.raises(SystemExit) as e:
            SG.main(["--signatures", FIXTURE] + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and err.startswith("drug_signatures: ") and err.count("\n") == 1 and words in err


def test_summary_line():
    rec = {"n": 10, "n_pairs": 45, "r": 0.5, "z": 2.25, "p_greater": 0.125, "p_two_sided": 0.25}
    assert SG.summary_line(rec, 8, "spearman", 200, 3, "pairs.tsv") == ("signatures: 10 drugs, 45 pairs, 8 genes: spearman r = 0.5, z = 2.25, "
                                                                         "p = 0.125 (two-sided 0.25; 200 permutations, seed 3): pairs.tsv")
