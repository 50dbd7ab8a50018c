"""GPU: shortest-path counts, best paths, the nodes between pairs and the mediators (csrc/trace.hip) bit-equal to the numpy mirror
(tests/trace_mirror.py, itself checked against networkx's enumeration in test_trace.py), the refusals of the C ABI, and the interpret.py
command end to end against tests/golden/trace_msi_small.  No tolerance anywhere but the device diffusion profiles' own (rtol 1e-4, as
test_gpu_predict.py gives them)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import predict_fixture as F  # noqa: E402
import trace_mirror as T  # noqa: E402
from gcn_drug_repurposing_amd import paths as P  # noqa: E402
from gcn_drug_repurposing_amd import trace as TR  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden", "trace_msi_small")


def _toward_equal(tracer, adj, targets, weights=None):
    tw = tracer.toward(targets, weights)
    d, s, b, nb = T.mirror_toward(adj, targets, weights)
    assert tw.dist.dtype == np.uint8 and tw.sigma.dtype == np.float64 and tw.sigma.shape == (len(targets), adj.shape[0])
    assert np.array_equal(tw.dist, d)
    assert np.array_equal(tw.sigma, s)
    if weights is None:
        assert tw.best is None and tw.best_next is None
    else:
        assert tw.best.dtype == np.float64 and tw.best_next.dtype == np.int32
        assert np.array_equal(tw.best_next, nb)
        assert np.array_equal(tw.best, b)
    return tw


def _from_equal(tracer, adj, sources):
    d, s = tracer.from_(sources)
    md, ms = T.mirror_from(adj, sources)
    assert np.array_equal(d, md) and np.array_equal(s, ms)


def _between_equal(tracer, adj, sources, targets, pairs, weights=None):
    r = tracer.between(sources, targets, pairs=pairs, weights=weights)
    m = T.mirror_between(adj, sources, targets, pairs, weights)
    assert np.array_equal(r.length, m["length"])
    assert np.array_equal(r.n_paths, m["n_paths"])
    assert np.array_equal(r.n_nodes, m["n_nodes"])
    assert np.array_equal(r.mediators[0], m["mediators"][0])
    assert np.array_equal(r.mediators[1], m["mediators"][1])
    assert set(r.tables) == set(m["tables"]) == set(pairs)
    for k in pairs:
        for got, want in zip(r.tables[k], m["tables"][k]):
            assert got.dtype == want.dtype and np.array_equal(got, want), k
    _, dt, st, b, nb = m["toward"]
    assert np.array_equal(r.toward.dist, dt) and np.array_equal(r.toward.sigma, st)
    if weights is not None:
        assert np.array_equal(r.toward.best, b) and np.array_equal(r.toward.best_next, nb)
    # sigma^s(t) == sigma_t(s), on the device's own numbers
    ds, ss = tracer.from_(sources)
    for i, s in enumerate(sources):
        for j, t in enumerate(targets):
            assert ss[i, t] == r.toward.sigma[j, s] == r.n_paths[i, j]
    return r


def test_msi_small_every_node_as_target_and_as_source():
    g = F.msi_graph(pathway=True)
    adj, names, _ = g.to_csr()
    n = adj.shape[0]
    nodes = list(range(n))                      # 111 nodes: two passes each, the second partial
    w = np.random.RandomState(0).randn(n, n)
    tracer = TR.PathTracer(adj)
    tw = _toward_equal(tracer, adj, nodes)
    assert len(tw.levels) == 2
    _toward_equal(tracer, adj, nodes, w)
    _from_equal(tracer, adj, nodes)
    q = names.index("NodeCovid")
    for v in nodes:
        p = tracer.best_path(q, v)
        if p is not None:
            assert p[0] == v and p[-1] == q and len(p) - 1 == tracer.last.dist[q, v] and all(adj[a, b] != 0 for a, b in zip(p, p[1:]))
    pairs = [(i, j) for i in range(0, n, 5) for j in range(0, n, 9)] + [(n - 1, n - 1), (70, 3)]
    _between_equal(tracer, adj, nodes, nodes, pairs, w)
    _between_equal(tracer, adj, nodes, nodes, pairs[:7])
    tracer.close()


def long_row_graph():
    rng = np.random.RandomState(11)
    n = 900
    a = sp.random(n, n, density=0.003, random_state=rng, format="lil")
    for v in range(0, n, 13):
        a[v, v] = 1.0                                            # self loops
    a[:, 100:106] = (rng.rand(n, 6) < 0.02).astype(float)        # the long rows are reached
    allowed = np.setdiff1d(np.arange(n), np.r_[50:60, 200:210])
    for v, k in ((100, 32), (101, 33), (102, 64), (103, 65), (104, 300), (105, 31)):   # either side of the one-lane / whole-wave boundary
        a[v, :] = 0
        a[v, rng.choice(allowed, k, replace=False)] = 1.0
    a[10:40, :] = 0                                              # sinks
    a[:, 50:60] = 0                                              # nodes nothing points at
    a[200:210, :] = 0
    a[:, 200:210] = 0                                            # isolated
    a = a.tocsr()
    a.eliminate_zeros()
    lens = np.diff(a.indptr)
    assert lens[[100, 101, 102, 103, 104, 105]].tolist() == [32, 33, 64, 65, 300, 31]
    return a


@pytest.mark.parametrize("q", [1, 64, 65])
def test_long_rows_sinks_self_loops_and_unreachable_nodes(q):
    a = long_row_graph()
    n = a.shape[0]
    rng = np.random.RandomState(q)
    targets = rng.choice(n, q, replace=False).tolist()
    sources = [100, 101, 102, 103, 104, 105, 15, 55, 205] + rng.choice(n, q, replace=False).tolist()
    w = rng.randn(q, n)
    tracer = TR.PathTracer(a)
    _toward_equal(tracer, a, targets)
    tw = _toward_equal(tracer, a, targets, w)
    assert (tw.dist == 255).any() and (tw.sigma > 1).any()
    _from_equal(tracer, a, sources[:q])
    pairs = [(i, j) for i in range(min(len(sources), 12)) for j in range(0, q, 7)]
    _between_equal(tracer, a, sources, targets, pairs, w)
    # an integer weight table ties everywhere: the smallest index among the equal successors
    wi = rng.randint(0, 2, size=(q, n)).astype(np.float64)
    _toward_equal(tracer, a, targets, wi)
    tracer.close()


def test_standin_mediators_and_pair_counts(tmp_path):
    from gcn_drug_repurposing_amd import synth
    from gcn_drug_repurposing_amd.msi import MsiGraph
    files = {}
    for name, rows in synth.standin_tables(seed=1).items():
        files[name] = str(tmp_path / (name + ".tsv"))
        with open(files[name], "w") as f:
            f.write("node_1\tnode_2\n")
            f.writelines(f"{a}\t{b}\n" for a, b in rows)
    g = MsiGraph().load(files)
    adj, names, types = g.to_csr()
    n = adj.shape[0]
    assert n == 29960
    idx = {x: i for i, x in enumerate(names)}
    inds = [idx[x] for x in g.indications_in_graph if x != "NodeCovid"]
    targets = [idx["NodeCovid"]] + inds[:63]
    sources = [idx[x] for x in g.drugs_in_graph][:128]             # two passes of sources: the accumulators continue across them
    assert len(targets) == 64 and len(sources) == 128
    w = np.random.RandomState(7).randn(64, n)
    pairs = [(i, (5 * i) % 64) for i in range(0, 128, 3)]
    tracer = TR.PathTracer(adj)
    r = _between_equal(tracer, adj, sources, targets, pairs, w)
    assert (r.toward.dist != 255).all() and (r.length > 0).all()   # the stand-in has no unreachable node: no pair is left out
    assert r.n_paths.max() > 1 and (r.mediators[1] > 0).any()
    tracer.close()


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


def test_counts_above_two_to_the_53_are_refused_not_rounded():
    a = layers(12, 32)
    assert a.shape[0] == 385
    tracer = TR.PathTracer(a)
    with pytest.raises(P.PathsError, match=r"more than 2\^53 shortest paths to target 0 \(node 0\)") as e:
        tracer.toward([0])
    assert "node 3" in str(e.value)                               # a node of layer 12 (353..384) is named
    tracer.close()
    tracer = TR.PathTracer(layers(11, 32))
    tw = tracer.toward([0])
    assert tw.sigma[0, -1] == float(32 ** 10) and tw.sigma[0, 1] == 1
    tracer.close()
    tracer = TR.PathTracer(layers(11, 31))
    tw = tracer.toward([0])
    for j in range(1, 12):
        assert [int(x) for x in tw.sigma[0, 1 + (j - 1) * 31:1 + j * 31]] == [31 ** (j - 1)] * 31      # Python's integers, exactly
    tracer.close()


def test_bad_passes_are_refused_by_name():
    import torch

    from gcn_drug_repurposing_amd import _lib
    lib = _lib.load()
    a = long_row_graph()
    n = a.shape[0]
    tracer = TR.PathTracer(a)
    w = np.zeros((2, n))
    w[1, 77] = np.nan
    with pytest.raises(P.PathsError, match=r"weight of node 77 for target 1 \(node 9\) is not finite"):
        tracer.toward([4, 9], w)
    w[1, 77] = np.inf
    with pytest.raises(P.PathsError, match="not finite"):
        tracer.toward([4, 9], w)
    with pytest.raises(P.PathsError, match="shape"):
        tracer.toward([4, 9], np.zeros((1, n)))
    with pytest.raises(P.PathsError, match="not a node index"):
        tracer.toward([n])
    with pytest.raises(P.PathsError, match="no nodes"):
        tracer.from_([])
    with pytest.raises(P.PathsError, match="budget"):
        TR.PathTracer(a, max_bytes=40 * n).toward([1])
    # the C ABI itself, with guard words behind every output: nothing is written past the buffers
    dev = torch.device("cuda")
    q = 3
    targets = np.array([4, 9, 300], np.int32)
    dist = torch.empty((q, n), dtype=torch.uint8, device=dev)
    nxt = torch.empty((q, n), dtype=torch.int32, device=dev)
    lv = C.c_int32(0)
    h = tracer._fwd
    st = _lib.current_stream()
    assert lib.gss_paths_run(h, q, targets.ctypes.data, _lib.ptr(dist), _lib.ptr(nxt), C.byref(lv), st) == 0
    levels = lv.value
    assert levels >= 2
    pad = 64
    sigma = torch.full((q * n + pad,), -7.0, dtype=torch.float64, device=dev)
    best = torch.full((q * n + pad,), -7.0, dtype=torch.float64, device=dev)
    bnext = torch.full((q * n + pad,), -7, dtype=torch.int32, device=dev)
    wd = torch.zeros((q, n), dtype=torch.float64, device=dev)

    def count(q_=q, dist_=dist, levels_=levels, w_=wd, sigma_=sigma, best_=best, bnext_=bnext, t_=targets):
        return lib.gss_paths_count(h, q_, t_.ctypes.data, _lib.ptr(dist_), levels_, _lib.ptr(w_), _lib.ptr(sigma_), _lib.ptr(best_),
                                   _lib.ptr(bnext_), st)

    def refused(text, **kw):
        assert count(**kw) == -22
        assert text in lib.gss_last_error().decode(), lib.gss_last_error()

    assert count() == 0
    assert (sigma[q * n:] == -7).all() and (best[q * n:] == -7).all() and (bnext[q * n:] == -7).all()
    d, s, _, _ = T.mirror_toward(a, targets)
    assert np.array_equal(sigma[:q * n].cpu().numpy().reshape(q, n), s)
    refused("Q=0 targets; a pass takes 1 to 64", q_=0)
    refused("Q=65 targets; a pass takes 1 to 64", q_=65, t_=np.zeros(65, np.int32))
    refused("levels=255 is outside 0..254", levels_=255)
    refused("levels=-1 is outside 0..254", levels_=-1)
    refused(f"levels={levels - 1} is smaller than the distance of node", levels_=levels - 1)
    refused("null argument", sigma_=None)
    refused("given together", best_=None)
    refused("is not a node index", t_=np.array([4, 9, n], np.int32))
    refused("is not 0 exactly at the target", t_=np.array([4, 9, 301], np.int32))
    wrong = dist.clone()
    wrong[1, 500] = 0
    refused("is not 0 exactly at the target", dist_=wrong)
    assert (sigma[q * n:] == -7).all() and (best[q * n:] == -7).all() and (bnext[q * n:] == -7).all()
    tracer.close()
    # a column twice in a row (the handle accepts it: its tie rule only needs the columns not to descend)
    rowptr = np.array([0, 1, 3, 4], np.int32)
    col = np.array([1, 2, 2, 0], np.int32)
    twice = TR.PathTracer((rowptr, col))
    with pytest.raises(P.PathsError, match="row 1 of the graph holds a column twice"):
        twice.toward([2])
    twice.close()
    # the between pass: Q = 0 / 65 and a node out of range, before anything is launched
    z = torch.zeros(64 * 64 + 8, dtype=torch.float64, device=dev)
    zi = torch.zeros(64 * 64 + 8, dtype=torch.int32, device=dev)
    ids = np.zeros(65, np.int32)

    def between(ns, nt, ids_=ids):
        return lib.gss_paths_between(n, ns, ids_.ctypes.data, _lib.ptr(dist), _lib.ptr(z), nt, ids_.ctypes.data, _lib.ptr(dist), _lib.ptr(z),
                                     _lib.ptr(zi), _lib.ptr(z), _lib.ptr(zi), None, None, st)
    assert between(0, 1) == -22 and b"S=0 sources" in lib.gss_last_error()
    assert between(1, 65) == -22 and b"T=65 targets" in lib.gss_last_error()
    assert between(1, 1, np.array([n], np.int32)) == -22 and b"not a node index" in lib.gss_last_error()


# ---- the command end to end ------------------------------------------------------------------------------------------------------------

def _close(got, want, rtol):
    return abs(float(got) - float(want)) <= rtol * abs(float(want))


@pytest.mark.parametrize("case", ["node2vec", "gcn", "diffusion"])
def test_cli_reproduces_the_enumerated_tables(tmp_path, case):
    cfg = F.stage(tmp_path, case)
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "interpret.py"), "-c", cfg, "--nodes", "nodes.tsv", "--edges", "edges.tsv",
                        "--mediators", "mediators.tsv"], cwd=tmp_path, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # the score columns of a device-computed diffusion profile: rtol 1e-4 (test_gpu_predict.py); every count, path and share byte-equal
    loose = {"trace": (2, 7), "nodes": (9,), "edges": (), "mediators": ()} if case == "diffusion" else {}
    for k in ("trace", "nodes", "edges", "mediators"):
        got = open(tmp_path / (k + ".tsv")).read()
        want = open(os.path.join(GOLD, f"expected_{case}_{k}.tsv")).read()
        if not loose.get(k):
            assert got == want, k
            continue
        grows, wrows = [x.split("\t") for x in got.split("\n")], [x.split("\t") for x in want.split("\n")]
        assert len(grows) == len(wrows)
        for a, b in zip(grows, wrows):
            assert len(a) == len(b)
            for c, (x, y) in enumerate(zip(a, b)):
                if c in loose[k] and x != y:
                    assert _close(x, y, 1e-4), (k, a, b)
                else:
                    assert x == y, (k, a, b)
