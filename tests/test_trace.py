"""CPU: the numpy mirror of csrc/trace.hip against networkx's enumeration of every shortest path, the interpret.py command on the small
fixture with the mirror standing in for the device (tests/golden/trace_msi_small, written by make_trace_fixture.py from networkx on the
reference's own graph), and the refusals that need no GPU."""
import os
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import predict_fixture as F  # noqa: E402
import trace_mirror as T  # noqa: E402

GOLD = os.path.join(HERE, "golden", "trace_msi_small")
TABLES = ("trace", "nodes", "edges", "mediators")


def digraph(adj):
    adj = sp.csr_matrix(adj)
    G = nx.DiGraph()
    G.add_nodes_from(range(adj.shape[0]))
    rows = np.repeat(np.arange(adj.shape[0]), np.diff(adj.indptr))
    G.add_edges_from(zip(rows.tolist(), adj.indices.tolist()))
    return G


def outward(w, path):
    """the weight sum of a path without its target, from the target outward"""
    b = 0.0
    for v in path[-2::-1]:
        b = w[v] + b
    return b


def check_pairs_against_networkx(adj, sources, targets, seed):
    from gcn_drug_repurposing_amd.paths import csr_arrays
    from gcn_drug_repurposing_amd.trace import NodeTable, edges_between, follow_best, Toward
    adj = sp.csr_matrix(adj)
    n = adj.shape[0]
    G = digraph(adj)
    w = np.random.RandomState(seed).randn(len(targets), n)
    pairs = [(i, j) for i in range(len(sources)) for j in range(len(targets))]
    r = T.mirror_between(adj, sources, targets, pairs, w)
    _, dt, st, best, nb = r["toward"]
    ds, ss = T.mirror_from(adj, sources)
    tw = Toward(np.asarray(targets), dt, st, best, nb, [])
    rowptr, col = csr_arrays(adj)
    reachable = 0
    for (i, j) in pairs:
        s, t = int(sources[i]), int(targets[j])
        try:
            paths = [list(p) for p in nx.all_shortest_paths(G, s, t)]
        except nx.NetworkXNoPath:
            assert r["length"][i, j] == -1 and r["n_paths"][i, j] == 0 and r["n_nodes"][i, j] == 0 and len(r["tables"][(i, j)][0]) == 0
            assert follow_best(tw, j, s) is None and nb[j, s] == -1 and best[j, s] == 0
            continue
        reachable += 1
        total = len(paths)
        assert r["length"][i, j] == len(paths[0]) - 1
        assert r["n_paths"][i, j] == total == st[j, s] == ss[i, t]            # sigma^s(t) == sigma_t(s)
        tab = NodeTable(*r["tables"][(i, j)])
        on = sorted({v for p in paths for v in p})
        assert tab.node.tolist() == on and r["n_nodes"][i, j] == len(on)
        for k, v in enumerate(on):
            through = sum(1 for p in paths if v in p)
            assert tab.through[k] == through and tab.share[k] == through / total     # to the bit: one division of the same two integers
            assert tab.hops_from[k] == paths[[v in p for p in paths].index(True)].index(v)
            assert tab.hops_from[k] + tab.hops_to[k] == len(paths[0]) - 1
        count = {}
        for p in paths:
            for e in zip(p, p[1:]):
                count[e] = count.get(e, 0) + 1
        eu, ev, es = edges_between(rowptr, col, tab, r["n_paths"][i, j], st[j])
        assert list(zip(eu.tolist(), ev.tolist())) == sorted(count)
        assert es.tolist() == [count[e] / total for e in sorted(count)]
        sums = [outward(w[j], p) for p in paths]
        got = follow_best(tw, j, s)
        assert best[j, s] == max(sums)
        assert got in paths and outward(w[j], got) == max(sums)
    # the mediators: every source's share of every interior node, in list order
    M, C = r["mediators"]
    for j, t in enumerate(targets):
        want_m, want_c = np.zeros(n), np.zeros(n, np.int32)
        for i, s in enumerate(sources):
            tab = NodeTable(*r["tables"][(i, j)])
            for v, sh in zip(tab.node, tab.share):
                if v not in (s, t):
                    want_m[v] = want_m[v] + sh
                    want_c[v] += 1
        assert np.array_equal(M[j], want_m) and np.array_equal(C[j], want_c)
    return reachable


def test_mirror_equals_networkx_for_every_drug_of_the_small_fixture():
    g = F.msi_graph(True)
    adj, names, types = g.to_csr()
    pattern = sp.csr_matrix((np.ones(adj.nnz), adj.indices, adj.indptr), shape=adj.shape)
    assert (pattern != pattern.T).nnz == 0                     # the MSI fixtures are symmetric: the random graphs below are not
    drugs = [i for i, t in enumerate(types) if t == "drug"]
    assert len(drugs) == 12
    assert check_pairs_against_networkx(adj, drugs, [names.index("NodeCovid")], seed=0) == 12
    _, sigma, _, _ = T.mirror_toward(adj, [names.index("NodeCovid")])
    assert sum(sigma[0, d] > 1 for d in drugs) == 9 and max(sigma[0, d] for d in drugs) == 6


def random_directed(seed, n=60, density=0.06):
    rng = np.random.RandomState(seed)
    a = sp.random(n, n, density=density, random_state=rng, format="lil")
    for v in range(0, n, 7):
        a[v, v] = 1.0              # self loops
    a[3:9, :] = 0                  # sinks
    a[:, 20:24] = 0                # nodes nothing points at
    a[40:44, :] = 0                # isolated: no way in or out
    a[:, 40:44] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    return a


@pytest.mark.parametrize("seed", [1, 2])
def test_mirror_equals_networkx_on_random_directed_graphs(seed):
    a = random_directed(seed)
    pattern = sp.csr_matrix((np.ones(a.nnz), a.indices, a.indptr), shape=a.shape)
    assert (pattern != pattern.T).nnz > 0                      # asymmetric
    nodes = list(range(a.shape[0]))
    reachable = check_pairs_against_networkx(a, nodes, nodes, seed)
    assert 500 < reachable < a.shape[0] ** 2                   # some pairs unreachable, most of the rest traced


def test_mirror_counts_are_exact_and_guarded():
    def layers(depth, width):
        n = 1 + depth * width
        rows, cols = [], []
        for j in range(1, depth + 1):
            for a in range(width):
                v = 1 + (j - 1) * width + a
                below = [0] if j == 1 else [1 + (j - 2) * width + b for b in range(width)]
                rows += [v] * len(below)
                cols += below
        return sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    _, s, _, _ = T.mirror_toward(layers(11, 31), [0])
    assert int(s[0, -1]) == 31 ** 10
    with pytest.raises(T.CountRefused, match="2\\^53"):
        T.mirror_toward(layers(12, 32), [0])


# ---- the command with the mirror injected ---------------------------------------------------------------------------------------------

def run_with_mirror(tmp_path, case, monkeypatch, **kw):
    from gcn_drug_repurposing_amd import interpret, predict
    monkeypatch.chdir(tmp_path)
    cfg = F.stage(tmp_path, case)
    if case == "diffusion":
        F.stage_reference_profile(tmp_path)
    s = predict.Settings(predict.load_config(cfg))
    return interpret.run(s, out="trace.tsv", nodes="nodes.tsv", edges="edges.tsv", mediators="mediators.tsv", tracer=T.MirrorTracer, **kw)


@pytest.mark.parametrize("case", ["node2vec", "gcn", "diffusion"])
def test_command_reproduces_the_enumerated_tables(tmp_path, case, monkeypatch):
    written = run_with_mirror(tmp_path, case, monkeypatch)
    assert written == {k: k + ".tsv" for k in TABLES}
    for k in TABLES:
        got = (tmp_path / (k + ".tsv")).read_bytes()
        assert got == open(os.path.join(GOLD, f"expected_{case}_{k}.tsv"), "rb").read(), k
    # row k's drug and proximity are row k's of the drug table
    drugs = F.read_tsv(os.path.join(F.D, f"expected_{case}.tsv"))
    rows = F.read_tsv(tmp_path / "trace.tsv")
    assert [r[1:3] for r in rows] == [d[0:2] for d in drugs] and len(rows) == F.TOPK


def test_drug_selection(tmp_path, monkeypatch):
    from gcn_drug_repurposing_amd import interpret
    written = run_with_mirror(tmp_path, "gcn", monkeypatch, top=3)
    rows = F.read_tsv(tmp_path / written["trace"])
    exp = F.read_tsv(os.path.join(GOLD, "expected_gcn_trace.tsv"))
    assert rows == exp[:3]
    run_with_mirror(tmp_path, "gcn", monkeypatch, all_drugs=True)
    every = F.read_tsv(tmp_path / "trace.tsv")
    assert len(every) == 12 and every[:10] == exp
    run_with_mirror(tmp_path, "gcn", monkeypatch, drugs=["DB00008", "DB00010"])
    two = F.read_tsv(tmp_path / "trace.tsv")
    assert two == [exp[0], exp[2]]                              # in the ranking's order, not the command line's
    med = F.read_tsv(tmp_path / "mediators.tsv")
    assert med and all(int(r[4]) <= 2 for r in med)
    with pytest.raises(interpret.PredictError, match="exclude each other"):
        run_with_mirror(tmp_path, "gcn", monkeypatch, top=3, drugs=["DB00008"])


# ---- refusals that need no GPU ----------------------------------------------------------------------------------------------------------

def _cli(tmp_path, cfg, args=()):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = "-1"      # a refusal comes before anything touches the GPU
    cmd = [sys.executable, os.path.join(ROOT, "interpret.py"), "-c", cfg] + list(args)
    return subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, env=env, timeout=300)


def _refused(tmp_path, cfg, args, *messages):
    r = _cli(tmp_path, cfg, args)
    assert r.returncode == 2, r.stdout + r.stderr
    for m in messages:
        assert m in r.stderr, r.stderr
    assert "Traceback" not in r.stderr
    assert not (tmp_path / "trace.tsv").exists()


def test_refusals_by_name(tmp_path):
    cfg = F.stage(tmp_path, "gcn")
    _refused(tmp_path, cfg, ["--drug", "DB99999"], "--drug 'DB99999' is not a node")
    _refused(tmp_path, cfg, ["--drug", "117"], "--drug '117' is not a drug")
    _refused(tmp_path, cfg, ["--top", "3", "--drug", "DB00008"], "--top", "--drug")
    _refused(tmp_path, cfg, ["--query", "NoSuchNode"], "--query 'NoSuchNode' is not a node")
    _refused(tmp_path, str(tmp_path / "absent.json"), [], "absent.json")
    # a query without a row in the embedding file, and a graph node without one
    emb = tmp_path / "n2v_num_64_len_16.embs.txt"
    lines = emb.read_text().splitlines()
    two = tmp_path / "short"
    two.mkdir()
    cfg2 = F.stage(two, "node2vec")
    kept = [l for l in lines[1:] if not l.startswith("NodeCovid ")]
    (two / "n2v_num_64_len_16.embs.txt").write_text(f"{len(kept)} {lines[0].split()[1]}\n" + "\n".join(kept) + "\n")
    _refused(two, cfg2, [], "--query 'NodeCovid' has no row in the embedding file")
    kept = [l for l in lines[1:] if not l.startswith("117 ")]
    (two / "n2v_num_64_len_16.embs.txt").write_text(f"{len(kept)} {lines[0].split()[1]}\n" + "\n".join(kept) + "\n")
    _refused(two, cfg2, [], "graph node '117' has no row in the embedding file")
