"""GPU: enrich.py end to end on the small tables (60 proteins, 26 functions of up to 5 proteins).  The whole table is rebuilt from the profile
files the program itself wrote, with the numpy mirror (enrich_mirror.py: order, score, permutation, statistics): every cell equal, floats
by their repr."""
import io
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import enrich_mirror as M  # noqa: E402
import predict_fixture as PF  # noqa: E402

from gcn_drug_repurposing_amd import enrich as E  # noqa: E402

pytestmark = pytest.mark.gpu


def environment():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def program(tmp_path, cfg, *args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "enrich.py"), "-c", cfg] + list(args), cwd=str(tmp_path), capture_output=True,
                          text=True, env=environment(), timeout=600)


def written_profiles(tmp_path, nodes):
    with open(tmp_path / "dp" / "node2idx.pkl", "rb") as f:
        node2idx = pickle.load(f)
    order = sorted(node2idx, key=node2idx.get)
    return order, {n: np.load(tmp_path / "dp" / f"{n}_p_visit_array.npy") for n in nodes}


def cell(v):
    return "NA" if v is None else repr(float(v)) if isinstance(v, (float, np.floating)) else str(v)


def graph_sets(order, g, kind, universe, lo, hi):
    place = {order[i]: u for u, i in enumerate(universe)}
    sets = [(n, g.node2name.get(n), sorted(place[v] for v in g.adj[n] if v in place)) for n in order if g.type[n] == kind]
    return [t for t in sets if lo <= len(t[2]) <= hi]


def expected_table(order, prof, g, nodes, sets, universe, samples, seed, weighted=True, top=None):
    """-> (rows as the program prints them, the null [nodes][samples][sizes])"""
    sizes = sorted({len(t[2]) for t in sets})
    rows, nulls = [], []
    for node in nodes:
        pos, w = M.order(prof[node], universe)
        scored = [M.es_peak(pos, w, t[2], weighted) for t in sets]
        null, _ = M.random_scores(pos, w, sizes, seed, 0, samples, weighted)
        nulls.append(null)
        stats = M.stats([e for e, _ in scored], [k for _, k in scored], [t[2] for t in sets], pos, sizes, null)
        block = []
        for (name, label, members), (es, _), r in zip(sets, scored, stats):
            lead = [order[universe[u]] for u in r["lead"]]
            block.append((r["p"], r["nes"], [node, g.node2name.get(node), name, label, len(members), es, r["nes"], r["p"], r["q"], len(lead), ",".join(lead)]))
        block.sort(key=lambda b: (b[0] != b[0], b[0], -abs(b[1]) if b[1] == b[1] else float("inf"), b[2][2]))
        rows += [[cell(v) for v in b[2]] for b in block[:top]]
    return rows, np.stack(nulls)


def test_functions_table(tmp_path):
    cfg = PF.stage(tmp_path, "diffusion", with_embs=False)
    nodes = ["DB00003", "C0000000"]
    r = program(tmp_path, cfg, "--node", nodes[0], "--node", nodes[1], "--sets", "functions", "--min-size", "2", "--samples", "200", "--null",
                "null.npy")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    g = PF.msi_graph(False)
    order, prof = written_profiles(tmp_path, nodes)
    assert order == g.names
    universe = np.asarray([i for i, n in enumerate(order) if g.type[n] == "protein"])
    assert len(universe) == 60
    sets = graph_sets(order, g, "functional_pathway", universe, 2, 59)
    assert 2 <= len(sets) <= 26 and max(len(t[2]) for t in sets) <= 5
    want, null = expected_table(order, prof, g, nodes, sets, universe, 200, 0)
    assert open(tmp_path / "enrichment.tsv").readline().rstrip("\n").split("\t") == E.HEADER
    got = PF.read_tsv(tmp_path / "enrichment.tsv")
    assert got == want and len(got) == 2 * len(sets)
    assert r.stdout.strip().splitlines()[-1] == f"enrichment: 2 profiles x {len(sets)} sets, 200 samples, seed 0: enrichment.tsv"
    saved = np.load(tmp_path / "null.npy")
    assert saved.shape == null.shape and np.array_equal(saved.view(np.int64), null.view(np.int64))
    for node in nodes:                                                                # per node: ascending p
        ps = [float(x[7]) for x in got if x[0] == node]
        assert ps == sorted(ps) and all(0 < p <= 1 for p in ps)
    # --top, --unweighted and another seed, in process; the profile directory is reused
    rows, n_sets = E.run(cfg, nodes[:1], min_size=2, weighted=False, samples=50, seed=7, top=3, out=str(tmp_path / "e2.tsv"))
    want, _ = expected_table(order, prof, g, nodes[:1], sets, universe, 50, 7, weighted=False, top=3)
    assert PF.read_tsv(tmp_path / "e2.tsv") == want and len(want) == 3 and n_sets == len(sets)
    # the indications' sets: the node's own set is its sanity row
    rows, _ = E.run(cfg, ["C0000000"], sets="indications", min_size=1, samples=50, out=str(tmp_path / "e3.tsv"))
    isets = graph_sets(order, g, "indication", universe, 1, 59)
    want, _ = expected_table(order, prof, g, ["C0000000"], isets, universe, 50, 0)
    got = PF.read_tsv(tmp_path / "e3.tsv")
    assert got == want
    own = [x for x in got if x[2] == "C0000000"]
    assert len(own) == 1 and own[0][0] == "C0000000"
    # a .gmt with an unknown id: dropped and counted
    proteins = [order[i] for i in universe]
    gmt = tmp_path / "mine.gmt"
    gmt.write_text(f"first\tthe first set\t{proteins[0]}\tP_unknown\t{proteins[7]}\t{proteins[30]}\n"
                   f"second\tna\t{proteins[59]}\t{proteins[1]}\n"
                   f"lonely\tdropped by --min-size\t{proteins[5]}\n")
    err = io.StringIO()
    rows, n_sets = E.run(cfg, ["DB00003"], sets=str(gmt), min_size=2, samples=50, out=str(tmp_path / "e4.tsv"), err=err)
    assert f"enrich: dropped 1 ids of {gmt}: no protein node of the graph" in err.getvalue() and n_sets == 2
    msets = [("first", "the first set", [0, 7, 30]), ("second", "na", [1, 59])]
    want, _ = expected_table(order, prof, g, ["DB00003"], msets, universe, 50, 0)
    assert PF.read_tsv(tmp_path / "e4.tsv") == want
    # refusals: exit status 2, one line that names the flag, nothing written
    for extra, words in ((["--node", "DB00003", "--max-size", "1025"], "enrich: --max-size 1025 is above 1024"),
                         (["--node", "118"], "enrich: --node '118' has no diffusion profile"),
                         (["--node", "DB00003", "--samples", "0"], "enrich: --samples 0 must be at least 1")):
        r = program(tmp_path, cfg, "--out", "refused.tsv", *extra)
        assert r.returncode == 2 and r.stderr.strip().splitlines()[-1].startswith(words) and "enrichment:" not in r.stdout, (r.returncode, r.stderr)
        assert not os.path.exists(tmp_path / "refused.tsv")
