"""GPU: knockout.py end to end on the small tables, both modes, against distances taken with scipy from the reference's own vectors
(tests/golden/knockout_msi_small.npz) and, for genes the fixture has no column for, from the mirror's (knockout_mirror.py, which
test_knockout.py holds to the fixture within 1e-15).

Bounds, derived and not measured.  A device profile is within eps = 1e-13 of the reference's in every entry (test_gpu_knockout.py), n = 111,
gamma as in profile_dist_mirror.py.
  cityblock    sum |a - b|: the two profiles move it by at most 2 n eps, the kernel's own rounding is within 4 gamma(n + 8) of scipy's value d:
               |got - want| <= 2 n eps + 4 gamma(n + 8) d.
  correlation  1 - cos of the centred vectors.  A perturbation da of a moves the unit vector a_c / |a_c| by at most |da_c| / |a_c| to
               first order, |da_c| <= |da| <= sqrt(n) eps, so the cosine moves by at most sqrt(n) eps (1 / |a_c| + 1 / |b_c|); twice that
               covers the higher orders (the ratio is below 1e-9 here, asserted), plus the kernel's 8 gamma(n + 8) absolute:
               |got - want| <= 2 sqrt(n) eps (1 / |a_c| + 1 / |b_c|) + 8 gamma(n + 8).
delta = dist_after - dist_before takes the sum of its two distances' bounds."""
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.distance import cityblock, correlation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import evaluate_fixture as EF  # noqa: E402
import knockout_mirror as KM  # noqa: E402
import predict_fixture as PF  # noqa: E402
import profile_dist_mirror as M  # noqa: E402

from gcn_drug_repurposing_amd import knockout as K  # noqa: E402

pytestmark = pytest.mark.gpu
EPS, N = 1e-13, 111


def expected(metric, a, b):
    """-> (scipy's distance, the bound above)"""
    if metric == "cityblock":
        d = cityblock(a, b)
        return d, 2 * N * EPS + M.diff_rel_bound(N) * d
    ac, bc = np.linalg.norm(a - a.mean()), np.linalg.norm(b - b.mean())
    assert np.sqrt(N) * EPS * (1 / ac + 1 / bc) < 1e-9
    return correlation(a, b), 2 * np.sqrt(N) * EPS * (1 / ac + 1 / bc) + M.dot_abs_bound(N)


class Profiles:
    """the reference's vector of a (start, gene) column where the fixture has it, else the mirror's"""

    def __init__(self):
        fx = KM.fixture()
        self.have = {(str(s), str(g) or None): p for s, g, p in zip(fx["starts"], fx["genes"], fx["profiles"])}
        self.graph = KM.small_graph()

    def __call__(self, start, gene):
        if (start, gene) not in self.have:
            self.have[(start, gene)] = KM.mirror_profile(self.graph, KM.WEIGHTS, start, gene)[0]
        return self.have[(start, gene)]


def check_row(row, prof, metric):
    d, i, g = row[0], row[1], row[2]
    assert row[3] == (prof.graph.node2name.get(g) or "NA")
    want = [expected(metric, prof(d, None), prof(i, None)), expected(metric, prof(d, g), prof(i, g)),
            expected(metric, prof(d, None), prof(d, g)), expected(metric, prof(i, None), prof(i, g))]
    before, after, delta, sd, si = (float(v) for v in row[4:9])
    for name, got, (w, bound) in zip(("dist_before", "dist_after", "shift_drug", "shift_indication"), (before, after, sd, si), want):
        print(metric, d, i, g, name, "|got - want| / bound", abs(got - w) / bound)
        assert abs(got - w) <= bound, (name, d, i, g, got, w, bound)
    assert delta == after - before
    assert abs(delta - (want[1][0] - want[0][0])) <= want[0][1] + want[1][1]
    return want[1][0] - want[0][0], want[0][1] + want[1][1]


def test_triples_mode(tmp_path):
    prof = Profiles()
    cfg = EF.stage(tmp_path, "diffusion", with_embs=False)
    table = tmp_path / "triples.tsv"
    rows = [("DB00003", "C0000000", "151"), ("DB00003", "C0000004", "151"), ("DB00003", "NodeCovid", "151"), ("DB00003", "C0000000", "151"),
            ("DB00003", "C0000000", "no_such_gene"), ("DB00003", "C0000000", "104")]
    table.write_text("drug\tindication\tgene\n" + "".join("\t".join(r) + "\n" for r in rows))
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "knockout.py"), "-c", cfg, "--triples", str(table), "--out", "ko.tsv"], cwd=str(tmp_path),
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "knockout: skipped 1 triples: gene not in the graph" in r.stderr
    assert r.stdout.strip() == "correlation: 4 knock-outs: ko.tsv"
    assert open(tmp_path / "ko.tsv").readline().rstrip("\n").split("\t") == K.HEADER
    got = PF.read_tsv(tmp_path / "ko.tsv")
    assert [tuple(x[:3]) for x in got] == [rows[0], rows[1], rows[2], rows[5]]
    for x in got:
        check_row(x, prof, "correlation")
        assert int(x[9]) > 0 and int(x[10]) > 0


def test_screen_mode(tmp_path):
    prof = Profiles()
    cfg = EF.stage(tmp_path, "diffusion", with_embs=False)
    genes = ["151", "104", "118", "119", "158", "151"]
    (tmp_path / "genes.txt").write_text("\n".join(genes) + "\n\n")
    rec = K.run(cfg, drug="DB00003", indication="C0000000", genes=str(tmp_path / "genes.txt"), metric="cityblock", out=str(tmp_path / "s.tsv"))
    assert sorted(x["gene"] for x in rec) == sorted(set(genes))
    got = PF.read_tsv(tmp_path / "s.tsv")
    assert [x[2] for x in got] == [x["gene"] for x in rec]
    want = [check_row(x, prof, "cityblock") for x in got]
    for (d0, b0), (d1, b1), x0, x1 in zip(want, want[1:], got, got[1:]):       # |delta| descending, ties by gene id
        assert abs(d0) + b0 >= abs(d1) - b1
        assert abs(float(x0[6])) > abs(float(x1[6])) or (abs(float(x0[6])) == abs(float(x1[6])) and x0[2] < x1[2])
    top = K.run(cfg, drug="DB00003", indication="C0000000", genes=str(tmp_path / "genes.txt"), metric="cityblock", top=2, out=str(tmp_path / "t.tsv"))
    assert [x["gene"] for x in top] == [x["gene"] for x in rec[:2]]
    every = K.run(cfg, drug="DB00003", indication="C0000000", all_proteins=True, metric="cityblock", out=str(tmp_path / "a.tsv"))
    proteins = [n for n in prof.graph.names if prof.graph.type[n] == "protein"]
    assert sorted(x["gene"] for x in every) == sorted(proteins)
    by_gene = {x["gene"]: x for x in every}
    for x in rec:                                                              # a gene has the same bits alone and in the full screen
        assert all(by_gene[x["gene"]][h] == x[h] or (x[h] != x[h]) for h in K.HEADER)
