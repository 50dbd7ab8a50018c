"""GPU: drug_classes.py end to end on the small tables (tests/golden/predict_msi_small: 12 drugs in the graph).  The class table is written
here: two ATC levels, a drug with two codes (in two classes of each level), a singleton class (dropped), an id that is no node, and two
drugs of the graph that the table does not name (outside the pool); every drug of the fixture has a profile.

Every cell of classes.tsv is recomputed from the matrix and the null the program wrote and compared as text: the observed sum with the
kernels' stated order of additions (class_cohesion_mirror.ordered_pairs), mean / std / z with the numpy statements of the definition, p as a
count, q by the Benjamini-Hochberg definition per level.  The null is held to the mirror on the written matrix within gamma(K - 1) T
(test_gpu_class_cohesion.py), and the matrix to diffusion.compare_profiles on the same profiles bit for bit."""
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import class_cohesion_mirror as M  # noqa: E402
import predict_fixture as PF  # noqa: E402

from gcn_drug_repurposing_amd import classes as K  # noqa: E402
from gcn_drug_repurposing_amd import predict  # noqa: E402
from gcn_drug_repurposing_amd.diffusion import compare_profiles  # noqa: E402

pytestmark = pytest.mark.gpu

HEAD = ["db_id", "atc_code", "level_4", "level_4_name", "level_3", "level_3_name", "level_2", "level_2_name", "level_1", "level_1_name"]
CODES = [("DB00000", "A01AA01"), ("DB00001", "A01AB01"), ("DB00002", "A01BA01"), ("DB00003", "A02AA01"), ("DB00004", "A02AA02"),
         ("DB00005", "B01AA01"), ("DB00006", "B01AB01"), ("DB00000", "B01AC06"), ("DB00007", "B02AA01"), ("DB00008", "B02BA01"),
         ("DB00009", "C01AA01"), ("DB99999", "A01AA09")]
# what the table means on the fixture: {level: {class: drugs}}; C and C01 are singletons, DB99999 is no node
WANT = {1: {"A": ["DB00000", "DB00001", "DB00002", "DB00003", "DB00004"], "B": ["DB00000", "DB00005", "DB00006", "DB00007", "DB00008"]},
        2: {"A01": ["DB00000", "DB00001", "DB00002"], "A02": ["DB00003", "DB00004"], "B01": ["DB00000", "DB00005", "DB00006"],
            "B02": ["DB00007", "DB00008"]}}
POOL = {f"DB{i:05d}" for i in range(10)}
SAMPLES, SEED = 200, 3


def write_table(path, head=HEAD):
    lines = ["\t".join(head)]
    for drug, code in CODES:
        cells = {"db_id": drug, "atc_code": code}
        for k, width in ((4, 5), (3, 4), (2, 3), (1, 1)):
            cells[f"level_{k}"], cells[f"level_{k}_name"] = code[:width], "the " + code[:width] + " drugs"
        lines.append("\t".join(cells[h] for h in head))
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def program(tmp_path, *args):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return subprocess.run([sys.executable, os.path.join(ROOT, "drug_classes.py"), *args], cwd=str(tmp_path), capture_output=True, text=True,
                          env=env, timeout=600)


def bh(p):
    n, order = len(p), sorted(range(len(p)), key=lambda i: p[i])
    rank = {i: r + 1 for r, i in enumerate(order)}
    return [min(1.0, min(p[j] * n / rank[j] for j in range(n) if rank[j] >= rank[i])) for i in range(n)]


def test_drug_classes_end_to_end(tmp_path):
    cfg = PF.stage(tmp_path, "diffusion", with_embs=False)
    table = write_table(tmp_path / "atc.tsv")
    r = program(tmp_path, "-c", cfg, "--classes", table, "--levels", "1,2", "--samples", str(SAMPLES), "--seed", str(SEED), "--matrix", "D.npy",
                "--null", "null.npy")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().split("\n")[-1] == f"classes: 6 classes of 10 drugs, {SAMPLES} random sets per size: classes.tsv"
    assert "drug_classes: skipped 1 drugs of the table: not in the graph\n" in r.stderr and "no diffusion profile" not in r.stderr

    with open(tmp_path / "dp" / "node2idx.pkl", "rb") as f:
        node2idx = pickle.load(f)
    pool = sorted(POOL, key=node2idx.__getitem__)                       # the pool in node order
    row = {n: i for i, n in enumerate(pool)}
    D, null = np.load(tmp_path / "D.npy"), np.load(tmp_path / "null.npy")
    sizes = [2, 3, 5]
    assert D.shape == (10, 10) and null.shape == (SAMPLES, 3) and np.array_equal(D, D.T) and not np.isnan(D).any()

    # the matrix: compare_profiles on the profiles the program left, bit for bit
    s = predict.Settings(predict.load_config(cfg))
    _, profiles = predict.diffusion_profiles(s, predict.build_graph(s))
    assert np.array_equal(D, compare_profiles(profiles, pool, pool, "correlation").cpu().numpy())

    # the null: the mirror's permutations on the written matrix
    for k in range(SAMPLES):
        perm = M.permutation(SEED, k, 10)
        exact = M.fsum_prefixes(D, perm, sizes)
        for m, got, want in zip(sizes, null[k], exact):
            assert abs(got - want) <= M.gamma(m * (m - 1) // 2 - 1) * want, (k, m, got, want)
        assert np.array_equal(null[k], M.ordered_prefixes(D, perm, sizes)), k

    # the table, cell by cell as text
    assert open(tmp_path / "classes.tsv").readline().rstrip("\n").split("\t") == K.HEADER
    got = PF.read_tsv(tmp_path / "classes.tsv")
    want = []
    for level, by_class in WANT.items():
        rows = []
        for code, drugs in by_class.items():
            members = sorted(row[n] for n in drugs)
            m = len(members)
            pairs = m * (m - 1) // 2
            T = M.ordered_pairs(D, members)
            col = null[:, sizes.index(m)]
            mean, nm, ns = T / pairs, float(np.mean(col / pairs)), float(np.std(col / pairs, ddof=0))
            p = (1 + sum(1 for t in col if t <= T)) / (SAMPLES + 1)
            rows.append([level, code, "the " + code + " drugs", m, pairs, mean, nm, ns, (mean - nm) / ns if ns > 0 else math.nan, p])
        for x, q in zip(rows, bh([x[9] for x in rows])):
            x.append(q)
        want += sorted(rows, key=lambda x: (x[0], x[9], x[1]))
    assert len(got) == len(want) == 6
    for g, w in zip(got, want):
        assert g == [repr(float(v)) if isinstance(v, float) else str(v) for v in w], (g, w)


def test_refusals_exit_2_with_one_line(tmp_path):
    cfg = PF.stage(tmp_path, "diffusion", with_embs=False)
    table = write_table(tmp_path / "atc.tsv")
    short = write_table(tmp_path / "short.tsv", [h for h in HEAD if h != "level_2_name"])
    for args, words in ((("--classes", short, "--levels", "1,2"), "column 'level_2_name' is missing"),
                        (("--classes", table, "--levels", "1,7"), "level 7 is unknown"),
                        (("--classes", table, "--samples", "0"), "--samples 0 must be at least 1")):
        r = program(tmp_path, "-c", cfg, *args)
        assert r.returncode == 2 and r.stdout == "", (r.stdout, r.stderr)
        assert r.stderr.startswith("drug_classes: ") and r.stderr.count("\n") == 1 and words in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "classes.tsv")
