"""CPU: the host half of the ATC class coherence (classes.py) and the mirror the GPU tests hold the kernels to (class_cohesion_mirror.py):
the table's parsing (multi-code drugs, unknown drugs, drugs without a profile, --min-size), z / p / Benjamini-Hochberg q against direct
numpy statements on a hand-made null, the program's refusals that need no GPU, and the uniformity of the mirror's random sets."""
import math
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import class_cohesion_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import classes as K  # noqa: E402
from gcn_drug_repurposing_amd.predict import PredictError  # noqa: E402

TABLE_HEAD = ["db_id", "atc_code"] + [c for k in (4, 3, 2, 1) for c in (f"level_{k}", f"level_{k}_name")]


def write_table(path, rows, head=TABLE_HEAD):
    path.write_text("\t".join(head) + "\n" + "".join("\t".join(r) + "\n" for r in rows))
    return str(path)


def atc_row(drug, code):
    """a row as the reference's table has it: the code's prefixes of 5, 4, 3 and 1 characters, named after themselves"""
    cells = [drug, code]
    for width in (5, 4, 3, 1):
        cells += [code[:width], "name of " + code[:width]]
    return cells


ROWS = [atc_row("D1", "A01AA01"), atc_row("D2", "A01AB02"), atc_row("D3", "A02BA01"), atc_row("D1", "B01AC06"),      # D1 carries two codes
        atc_row("D4", "B01AC04"), atc_row("D9", "A01AA07"), atc_row("D5", "B02AA01"), atc_row("D2", "A01AB09"),      # D2 twice in A01AB
        atc_row("D6", "C01AA01")]


def test_table_parsing_counts_a_drug_once_per_class(tmp_path):
    drugs, table = K.read_classes(write_table(tmp_path / "t.tsv", ROWS), [1, 2])
    assert drugs == ["D1", "D2", "D3", "D4", "D9", "D5", "D6"]
    assert table[1] == {"A": ["name of A", ["D1", "D2", "D3", "D9"]], "B": ["name of B", ["D1", "D4", "D5"]], "C": ["name of C", ["D6"]]}
    assert table[2]["A01"] == ["name of A01", ["D1", "D2", "D9"]] and table[2]["B01"][1] == ["D1", "D4"]
    assert set(table[2]) == {"A01", "A02", "B01", "B02", "C01"}


def test_pool_classes_and_the_skipped_drugs(tmp_path):
    drugs, table = K.read_classes(write_table(tmp_path / "t.tsv", ROWS), [1, 2])
    g = types.SimpleNamespace(adj={n: {} for n in ("D6", "D5", "D4", "D3", "D2", "D1", "P1")})      # D9 is no node
    nodelist = ["P1", "D6", "D5", "D4", "D3", "D2", "D1"]
    profiles = {n: None for n in ("D1", "D2", "D3", "D4", "D6")}                                      # D5 has no profile
    pool, classes, no_node, no_profile = K.pool_and_classes(drugs, table, nodelist, profiles, g, 2)
    assert pool == ["D6", "D4", "D3", "D2", "D1"] and no_node == ["D9"] and no_profile == ["D5"]     # node order
    assert classes == [(1, "A", "name of A", [2, 3, 4]), (1, "B", "name of B", [1, 4]), (2, "A01", "name of A01", [3, 4]),
                       (2, "B01", "name of B01", [1, 4])]                                            # C, A02, B02, C01 are singletons
    assert [c[1] for c in K.pool_and_classes(drugs, table, nodelist, profiles, g, 3)[1]] == ["A"]
    # a drug whose only class is dropped stays in the pool: the pool is the drugs with a profile and a code
    assert "D6" in pool


def test_table_refusals(tmp_path):
    with pytest.raises(PredictError, match="column 'level_3' is missing"):
        K.read_classes(write_table(tmp_path / "a.tsv", [r[:4] + r[6:] for r in ROWS], TABLE_HEAD[:4] + TABLE_HEAD[6:]), [3])
    with pytest.raises(PredictError, match="column 'db_id' is missing"):
        K.read_classes(write_table(tmp_path / "b.tsv", ROWS, ["id"] + TABLE_HEAD[1:]), [1])
    for levels, words in (("1,5", "level 5 is unknown"), ("one", "comma-separated integers"), ("2,2", "repeats a level")):
        with pytest.raises(PredictError, match=words):
            K.check_args(levels, "correlation", 2, 10)
    with pytest.raises(PredictError, match="--metric 'hamming' is unknown"):
        K.check_args("1", "hamming", 2, 10)
    with pytest.raises(PredictError, match="--samples 0 must be at least 1"):
        K.check_args("1", "cosine", 2, 0)
    assert K.check_args("4,1", "spearman", 2, 1) == [1, 4]


def test_program_refusals_exit_2_with_one_line(tmp_path, capsys):
    table = write_table(tmp_path / "t.tsv", ROWS)
    for argv, words in ((["--classes", table, "--metric", "hamming"], "--metric 'hamming' is unknown"),
                        (["--classes", table, "--levels", "0"], "level 0 is unknown"),
                        (["--classes", table, "--samples", "0"], "--samples 0 must be at least 1"),
                        (["--classes", table, "-c", str(tmp_path / "none.json")], "none.json")):
        with pytest.raises(SystemExit) as e:
            K.main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and err.startswith("drug_classes: ") and err.count("\n") == 1 and words in err


def test_statistics_against_a_direct_numpy_statement():
    rng = np.random.RandomState(3)
    sizes = [2, 3, 7]
    null = np.stack([rng.rand(500) * m * (m - 1) / 2 for m in sizes], axis=1)
    null[:, 0] = 0.25                                       # a constant null: std 0, z nan
    observed, n_drugs = [0.25, 2.9, null[17, 2], 0.0], [2, 3, 7, 7]
    got = K.cohesion_stats(observed, n_drugs, sizes, null)
    for r, T, m in zip(got, observed, n_drugs):
        pairs = m * (m - 1) // 2
        col = null[:, sizes.index(m)]
        assert r["n_drugs"] == m and r["n_pairs"] == pairs == len(M.pair_terms(np.zeros((m, m)), range(m)))
        assert r["mean_distance"] == T / pairs and r["null_mean"] == np.mean(col / pairs) and r["null_std"] == np.std(col / pairs, ddof=0)
        assert r["p"] == (1 + sum(1 for t in col if t <= T)) / 501
        if m == 2:
            assert math.isnan(r["z"])
        else:
            assert r["z"] == (T / pairs - np.mean(col / pairs)) / np.std(col / pairs)
    assert got[0]["p"] == 1.0 and got[3]["p"] == 1 / 501 and got[2]["p"] >= 2 / 501      # ties count; the sample itself counts


def test_benjamini_hochberg_against_its_definition():
    rng = np.random.RandomState(5)
    for p in ([0.01], [0.04, 0.01, 0.03, 0.5, 0.03], list(rng.rand(40) ** 3), [1.0, 1.0], [0.001, 0.9, 0.9, 0.002]):
        p = np.asarray(p)
        n = len(p)
        ranks = np.empty(n)
        ranks[np.argsort(p, kind="stable")] = np.arange(1, n + 1)
        want = [min(1.0, min(p[j] * n / ranks[j] for j in range(n) if ranks[j] >= ranks[i])) for i in range(n)]
        got = K.benjamini_hochberg(p)
        assert np.array_equal(got, np.asarray(want))
        assert np.all(got >= p * (1 - 2.0 ** -50)) and np.all(np.diff(got[np.argsort(p, kind="stable")]) >= 0)


def test_mirror_prefixes_are_uniform_subsets():
    """index i is among the first m places of pi_s with probability m / n: 20,000 samples, n = 50, m = 7, every i within 5 binomial sigma"""
    n, m, S = 50, 7, 20000
    hits = np.zeros(n)
    for s in range(S):
        perm = M.permutation(11, s, n)
        assert s or sorted(perm) == list(range(n))
        hits[perm[:m]] += 1
    sigma = math.sqrt(S * (m / n) * (1 - m / n))
    assert np.all(np.abs(hits - S * m / n) <= 5 * sigma), (hits.min(), hits.max(), S * m / n, sigma)
    assert not np.array_equal(M.permutation(11, 0, n), M.permutation(12, 0, n))
    assert not np.array_equal(M.permutation(11, 0, n), M.permutation(11, 1, n))


def test_mirror_ordered_sums_stay_inside_the_any_order_bound():
    rng = np.random.RandomState(7)
    D = rng.rand(300, 300)
    D = D + D.T
    a = rng.permutation(300)
    sizes = [2, 3, 64, 65, 66, 130, 300]
    exact, ordered = M.fsum_prefixes(D, a, sizes), M.ordered_prefixes(D, a, sizes)
    for m, e, o in zip(sizes, exact, ordered):
        assert abs(o - e) <= M.gamma(m * (m - 1) // 2 - 1) * e
    assert ordered[0] == D[a[1], a[0]] and M.ordered_pairs(D, a[:1]) == 0.0 and M.ordered_pairs(D, a[:66]) == ordered[4]
    assert M.fsum_pairs(D, a[:65]) == exact[3]


def test_the_reference_table_on_the_standin_drugs():
    """tests/golden/atc_classes.npz is the reference's table as classes.read_classes reads it (make_atc_fixture.py); on the 1,661 drugs of the
    whole-graph stand-in (the reference's drug_to_protein table) it gives the pool and the class sizes DESIGN.md section 9.12 models and
    tools/class_cohesion_bench.py runs"""
    from gcn_drug_repurposing_amd import synth
    rows, drugs, table = M.atc_fixture()
    assert rows == 3987
    nodes = synth.real_layers()["names_drug"]
    assert len(drugs) == 2379 and len(nodes) == 1661
    g = types.SimpleNamespace(adj=dict.fromkeys(nodes))
    pool, classes, no_node, no_profile = K.pool_and_classes(drugs, table, nodes, dict.fromkeys(nodes), g, 2)
    assert len(pool) == 1328 and len(no_node) == 2379 - 1328 and no_profile == []
    by_level = {k: sorted({len(c[3]) for c in classes if c[0] == k}) for k in (1, 2, 3, 4)}
    assert [len(by_level[k]) for k in (1, 2, 3, 4)] == [14, 41, 31, 19] and [by_level[k][-1] for k in (1, 2, 3, 4)] == [266, 111, 66, 28]
    assert len({m for s in by_level.values() for m in s}) == 58
    assert all(rows == sorted(set(rows)) and 0 <= rows[0] and rows[-1] < 1328 for _, _, _, rows in classes)
