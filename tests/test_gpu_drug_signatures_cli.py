"""GPU: drug_signatures.py end to end on the small tables (tests/golden/predict_msi_small: 12 drugs in the graph).  The signature table is
written here: 10 of the 12 drugs and an id that is no node, 8 genes, the reference table's leading columns.

The two matrices the program wrote equal diffusion.compare_profiles bit for bit -- on the profiles it left and on the table's array --, and
every cell of signature_pairs.tsv and of the printed line is recomputed from them and from the null it wrote: the pair values and their
average-tie ranks, r and every r_s with the kernel's stated order of additions (mantel_mirror.ordered_cross_sum on the standardised
matrices), z with the numpy statements of the definition, p as a count."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import scipy.stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import mantel_mirror as M  # noqa: E402
import predict_fixture as PF  # noqa: E402

from gcn_drug_repurposing_amd import mantel as MT  # noqa: E402
from gcn_drug_repurposing_amd import predict  # noqa: E402
from gcn_drug_repurposing_amd import signatures as SG  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import compare_profiles  # noqa: E402

pytestmark = pytest.mark.gpu

GENES = ["2597", "1677", "81544", "3611", "22809", "8900", "29916", "10298"]
HEAD = ["drug", "drug_name", "sig_id", "cell", "dose", "time"] + GENES
DRUGS = [f"DB{i:05d}" for i in (7, 2, 9, 0, 4, 1, 8, 3, 6, 5)] + ["DB99999"]      # not in node order; DB99999 is no node
S, SEED = 200, 5


def write_table(path, drugs=DRUGS):
    rng = np.random.RandomState(11)
    values = np.round(rng.randn(len(DRUGS), len(GENES)), 6)
    lines = ["\t".join(HEAD)]
    for d, v in zip(DRUGS, values):
        if d in drugs:
            lines.append("\t".join([d, "the drug " + d, "SIG:" + d, "MCF7", "10 µM", "6 h"] + [repr(float(x)) for x in v]))
    path.write_text("\n".join(lines) + "\n", encoding="utf-8")
    return str(path), {d: v for d, v in zip(DRUGS, values)}


def program(tmp_path, *args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, "drug_signatures.py"), *args], cwd=str(tmp_path), capture_output=True, text=True,
                          env=env, timeout=600)


@pytest.mark.parametrize("method", MT.METHODS)
def test_drug_signatures_end_to_end(tmp_path, method):
    cfg = PF.stage(tmp_path, "diffusion", with_embs=False)
    table, values = write_table(tmp_path / "bcm.tsv")
    r = program(tmp_path, "-c", cfg, "--signatures", table, "--method", method, "--permutations", str(S), "--seed", str(SEED), "--metric", "correlation",
                "--signature-metric", "euclidean", "--matrix", "D.npy", "--signature-matrix", "E.npy", "--null", "null.npy")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "drug_signatures: skipped 1 drugs of the table: not in the graph\n" in r.stderr and "no diffusion profile" not in r.stderr

    with open(tmp_path / "dp" / "node2idx.pkl", "rb") as f:
        node2idx = pickle.load(f)
    pool = sorted(DRUGS[:10], key=node2idx.__getitem__)                 # the pool in node order
    n, K = 10, 45
    D, E, null = np.load(tmp_path / "D.npy"), np.load(tmp_path / "E.npy"), np.load(tmp_path / "null.npy")
    assert D.shape == E.shape == (n, n) and null.shape == (S,)

    # the matrices: compare_profiles on the profiles the program left and on the table's array, bit for bit
    s = predict.Settings(predict.load_config(cfg))
    _, profiles = predict.diffusion_profiles(s, predict.build_graph(s))
    assert np.array_equal(D, compare_profiles(profiles, pool, pool, "correlation").cpu().numpy())
    assert np.array_equal(E, compare_profiles(np.stack([values[d] for d in pool]), None, None, "euclidean").cpu().numpy())
    assert np.array_equal(D, D.T) and np.array_equal(E, E.T)

    # r and the null: the kernel's additions on the standardised matrices
    sd, se = MT.standardise_pairs(D, method).cpu().numpy(), MT.standardise_pairs(E, method).cpu().numpy()
    for h, m in ((D, sd), (E, se)):
        assert np.max(np.abs(m - M.standardised(h, method))) <= M.gamma(4 * K)
    robs = M.ordered_cross_sum(sd, se)
    for k in range(S):
        assert null[k] == M.ordered_cross_sum(sd, se, M.permutation(SEED, k, n)), k
    iu = np.triu_indices(n, 1)
    want = (scipy.stats.spearmanr if method == "spearman" else scipy.stats.pearsonr)(D[iu], E[iu])[0]
    assert abs(robs - want) <= 2 * M.gamma(4 * K)

    # the printed line, as text
    nm, ns = float(np.mean(null)), float(np.std(null, ddof=0))
    rec = {"n": n, "n_pairs": K, "r": robs, "z": (robs - nm) / ns, "p_greater": (1 + sum(1 for t in null if t >= robs)) / (S + 1),
           "p_two_sided": (1 + sum(1 for t in null if abs(t) >= abs(robs))) / (S + 1)}
    assert r.stdout.strip().split("\n")[-1] == (f"signatures: 10 drugs, 45 pairs, 8 genes: {method} r = {robs!r}, z = {rec['z']!r}, p = {rec['p_greater']!r} "
                                                f"(two-sided {rec['p_two_sided']!r}; {S} permutations, seed {SEED}): signature_pairs.tsv")
    assert r.stdout.strip().split("\n")[-1] == SG.summary_line(rec, 8, method, S, SEED, "signature_pairs.tsv")

    # the pair table, cell by cell as text
    header = SG.HEADER + (SG.RANK_HEADER if method == "spearman" else [])
    assert open(tmp_path / "signature_pairs.tsv").readline().rstrip("\n").split("\t") == header
    got = PF.read_tsv(tmp_path / "signature_pairs.tsv")
    rd, re_ = scipy.stats.rankdata(D[iu]), scipy.stats.rankdata(E[iu])
    assert len(got) == K
    for k, (i, j) in enumerate(zip(*iu)):
        cells = [pool[i], pool[j], "the drug " + pool[i], "the drug " + pool[j], repr(float(D[i, j])), repr(float(E[i, j]))]
        cells += [repr(float(rd[k])), repr(float(re_[k]))] if method == "spearman" else []
        assert got[k] == cells, (k, got[k], cells)


def test_refusals_exit_2_with_one_line(tmp_path):
    cfg = PF.stage(tmp_path, "diffusion", with_embs=False)
    table, _ = write_table(tmp_path / "bcm.tsv")
    two, _ = write_table(tmp_path / "two.tsv", ["DB00003", "DB00008", "DB99999"])
    for args, words in ((("--signatures", two), "the pool of 2 drugs"), (("--signatures", table, "--method", "kendall"), "--method 'kendall' is unknown"),
                        (("--signatures", str(tmp_path / "none.tsv")), "none.tsv")):
        r = program(tmp_path, "-c", cfg, *args)
        assert r.returncode == 2 and "signatures:" not in r.stdout, (r.stdout, r.stderr)     # the first run may announce the profiles it computes
        lines = [l for l in r.stderr.split("\n") if l.startswith("drug_signatures: ") and "skipped" not in l]
        assert len(lines) == 1 and words in lines[0] and "Traceback" not in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "signature_pairs.tsv")
