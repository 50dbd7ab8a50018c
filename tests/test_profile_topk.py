"""CPU: the numpy mirror of csrc/profile_topk.hip (keys, digit sweeps, index digits among ties, collection, final sort) against the statement
np.argsort(-col[members], kind="stable")[:k], for equality; the refusals diffusion.top_nodes / top_overlap and explain.check_args make
before the GPU is touched; the row ordering and the Jaccard arithmetic of explain.py's two tables on hand-made selections; the exports.
The device kernels are checked in test_gpu_profile_topk.py, the program end to end in test_gpu_explain_cli.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import profile_topk_mirror as T  # noqa: E402

KS = (1, 5, 64, 1024)


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


def test_mirror_constants_are_the_kernels():
    csrc = os.path.join(ROOT, "gcn-drug-repurposing_amd", "csrc")
    text = open(os.path.join(csrc, "profile_topk.hip")).read() + open(os.path.join(csrc, "profile_front.h")).read()   # the shared front end
    for name, value in (("kKeyPanel", T.PANEL), ("kTkThreads", T.THREADS), ("kStatusBytes", T.STATUS_BYTES), ("kTkMaxK", T.MAX_K),
                        ("kTkMaxGroups", T.MAX_GROUPS)):
        assert [int(v) for v in re.findall(r"constexpr int %s = (\d+);" % name, text)] == [value]                  # stated once
    assert len(re.findall(r"constexpr int kKeyMaxRows = 1 << 24;", text)) == 1 and T.MAX_ROWS == 1 << 24


def test_generator_holds_what_the_kernel_must_survive():
    p = T.columns(2000, 8, 3)
    v = p[2]                                                                    # zeros_and_tails
    assert (v == 0).mean() > 0.4 and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()
    assert np.isinf(v).sum() >= 2 and (np.abs(v) == 5e-324).sum() >= 2
    assert len(np.unique(p[1])) <= 5 and len(np.unique(p[3])) == 1              # heavy ties, all equal


@pytest.mark.parametrize("n", T.SIZES)
def test_mirror_equals_the_argsort_statement(n):
    p = T.columns(n, 8, 100 * n)
    for G in (1, 3):
        for variant, group in enumerate((None,) if G == 1 else (T.groups(n, G, n), T.groups(n, G, n + 7, empty=1))):
            for k in KS:
                for j, v in enumerate(p):
                    got, want = T.mirror_topk(v, group, G, k), T.expected(v, group, G, k)
                    assert same(got, want), (n, G, variant, k, j)
                    if G == 3 and variant == 1:
                        assert want[2][1] == 0 and np.all(want[0][1] == -1)      # the empty group


def test_mirror_ties_across_the_kth_place():
    n = 70000                                                                   # three distinct values; the middle run sits at indices
    v = np.full(n, -1.0)                                                        # whose third 8-bit digit is not zero
    v[66000:] = 0.5
    v[::7000] = 2.0                                                             # ten nodes above the run
    for k in (1, 5, 10, 11, 64, 1024):
        assert same(T.mirror_topk(v, None, 1, k), T.expected(v, None, 1, k)), k
    _, I, sweeps = T.mirror_select(T.keys(v), np.arange(n), 1024)
    assert sweeps > 8 and I == 66000 + 1014 - 1                                 # the index digits were needed: the last admitted tie
    flat = np.full(1000, 0.25)
    idx, _, cnt = T.mirror_topk(flat, None, 1, 64)
    assert np.array_equal(idx[0], np.arange(64)) and cnt[0] == 64               # all equal: the first k nodes
    _, I, sweeps = T.mirror_select(T.keys(np.random.RandomState(0).rand(30000)), np.arange(30000), 20)
    assert I is None and sweeps <= 4                                            # distinct keys: the select stops early


def test_mirror_nan_flags_only_its_own_group():
    n = 300
    v = T.column("uniform", n, 5)
    group = T.groups(n, 3, 9)
    at1, out = np.flatnonzero(group == 1)[4], np.flatnonzero(group == -1)[2]
    v[out] = np.nan
    assert same(T.mirror_topk(v, group, 3, 7), T.expected(v, group, 3, 7)) and np.all(T.mirror_topk(v, group, 3, 7)[2] == 7)
    v[at1] = np.nan
    idx, val, cnt = T.mirror_topk(v, group, 3, 7)
    assert list(cnt) == [7, -1, 7] and np.all(idx[1] == -1) and np.all(val[1] == T.NAN_BITS) and same((idx, val, cnt), T.expected(v, group, 3, 7))


def test_workspace_formula():
    assert T.workspace_bytes(29960, 2502, 2, 20) == 256 + 512 * 29960 * 8 == T.workspace_bytes(29960, 512, 8, 1024)
    assert T.workspace_bytes(10, 3, 1, 1) == 256 + 240 and T.workspace_bytes(10, 0, 1, 1) == 256
    for bad in ((0, 1, 1, 1), ((1 << 24) + 1, 1, 1, 1), (5, -1, 1, 1), (5, 1, 0, 1), (5, 1, 9, 1), (5, 1, 1, 0), (5, 1, 1, 1025)):
        assert T.workspace_bytes(*bad) == 0


# ---- the library's exports -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import gcn_drug_repurposing_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        pkg.build()
    return pkg.load()


def test_library_exports_header_binding_and_abi(lib):
    import gcn_drug_repurposing_amd as pkg
    assert pkg._lib.ABI_VERSION == lib.gss_abi_version() >= 19      # 19 brought these entry points; later versions keep them
    header = open(os.path.join(ROOT, "include", "gssgcn.h")).read()
    assert "#define GSS_ABI_VERSION %d " % pkg._lib.ABI_VERSION in header and " 19: exact typed top-k selection" in header
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.LIB_PATH], capture_output=True, text=True).stdout
    for name in ("gss_profile_topk", "gss_profile_topk_workspace_bytes", "gss_topk_overlap"):
        assert re.search(r" T %s$" % name, out, flags=re.M), name
        assert name in pkg._lib.SIGNATURES and re.search(r"\b%s\(" % name, header), name
    for args in ((1, 1, 1, 1), (63, 17, 3, 5), (29960, 511, 2, 20), (29960, 513, 8, 1024), (29960, 2502, 2, 20), (1 << 24, 3, 1, 1), (5, 0, 1, 1),
                 (0, 1, 1, 1), ((1 << 24) + 1, 1, 1, 1), (5, -1, 1, 1), (5, 1, 0, 1), (5, 1, 9, 1), (5, 1, 1, 0), (5, 1, 1, 1025)):
        assert lib.gss_profile_topk_workspace_bytes(*args) == T.workspace_bytes(*args), args


def test_entry_point_refusals_that_come_before_the_gpu(lib):
    """argument checks that return before any HIP call (no device here): the pointers are never dereferenced"""
    def call(n, x, ld, nc, G, group, k, idx, val, cnt, ws, ws_bytes):
        rc = lib.gss_profile_topk(n, x, ld, nc, None, G, group, k, idx, val, cnt, ws, ws_bytes, None)
        return rc, lib.gss_last_error().decode()
    need = T.workspace_bytes(8, 4, 1, 3)
    ok = dict(n=8, x=8, ld=4, nc=4, G=1, group=None, k=3, idx=8, val=8, cnt=8, ws=8, ws_bytes=need)
    cases = [(dict(n=0), "n=0"), (dict(n=(1 << 24) + 1), "above the limit of 16777216"), (dict(k=0), "k=0 is outside [1, 1024]"),
             (dict(k=1025), "k=1025 is outside [1, 1024]"), (dict(G=0), "G=0 groups is outside [1, 8]"), (dict(G=9, group=8), "G=9 groups is outside [1, 8]"),
             (dict(nc=-1), "nc=-1"), (dict(ld=0), "ld=0"), (dict(x=None), "x is null"), (dict(idx=None), "idx is null"), (dict(val=None), "val is null"),
             (dict(cnt=None), "cnt is null"), (dict(ws=None), "workspace is null"), (dict(G=2), "group is null"), (dict(ld=3), "ld=3 is below nc=4"),
             (dict(ws=12), "not 8-byte aligned"), (dict(ws_bytes=need - 1), f"below the {need} that n=8, nc=4 need")]
    for change, message in cases:
        rc, msg = call(**dict(ok, **change))
        assert rc == -22 and msg.startswith("profile_topk: ") and message in msg, (message, rc, msg)
    assert call(**dict(ok, nc=0, x=None, idx=None, val=None, cnt=None, ws=None, ws_bytes=0))[0] == 0      # nc = 0: a no-op

    def overlap(S=4, G=2, k=5, idx=8, cnt=8, T_=3, a=8, b=8, shared=8):
        rc = lib.gss_topk_overlap(S, G, k, idx, cnt, T_, a, b, shared, None)
        return rc, lib.gss_last_error().decode()
    for change, message in ((dict(S=0), "S=0"), (dict(k=0), "k=0 is outside [1, 1024]"), (dict(k=2000), "k=2000 is outside"), (dict(G=9), "G=9 groups is outside [1, 8]"),
                            (dict(T_=-1), "T=-1"), (dict(idx=None), "idx is null"), (dict(cnt=None), "cnt is null"), (dict(a=None), "a is null"),
                            (dict(b=None), "b is null"), (dict(shared=None), "shared is null")):
        rc, msg = overlap(**change)
        assert rc == -22 and msg.startswith("topk_overlap: ") and message in msg, (message, rc, msg)
    assert overlap(T_=0, a=None, b=None, shared=None)[0] == 0


# ---- diffusion.top_nodes / top_overlap: the refusals of the host ---------------------------------------------------------------------------

def test_python_refusals_come_before_the_library(monkeypatch):
    import torch

    from gcn_drug_repurposing_amd import _lib, diffusion
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the refusal"))
    p = np.ones((3, 10))
    named = {"a": p[0], "b": p[1]}
    for k in (0, 1025, -3, 2.5):
        with pytest.raises(ValueError, match=r"top_nodes: k=.* is outside \[1, 1024\]"):
            diffusion.top_nodes(p, k=k)
    with pytest.raises(ValueError, match=r"top_nodes: G=9 groups is outside \[1, 8\]"):
        diffusion.top_nodes(p, groups=np.zeros(10, np.int32), n_groups=9)
    with pytest.raises(ValueError, match=r"top_nodes: G=0 groups is outside \[1, 8\]"):
        diffusion.top_nodes(p, groups=np.zeros(10, np.int32), n_groups=0)
    with pytest.raises(ValueError, match=r"top_nodes: G=12 groups is outside \[1, 8\]"):
        diffusion.top_nodes(p, groups=np.arange(10) + 2)
    with pytest.raises(ValueError, match="top_nodes: n_groups=2 needs a groups array"):
        diffusion.top_nodes(p, n_groups=2)
    with pytest.raises(ValueError, match="top_nodes: groups has 9 entries, the profiles 10 nodes"):
        diffusion.top_nodes(p, groups=np.zeros(9, np.int32))
    with pytest.raises(ValueError, match=r"top_nodes: groups\[4\] = 2 is outside \[-1, G=2\)"):
        diffusion.top_nodes(p, groups=[0, 1, -1, 0, 2, 0, 0, 0, 0, 0], n_groups=2)
    with pytest.raises(ValueError, match=r"top_nodes: groups\[1\] = -2 is outside \[-1, G=1\)"):
        diffusion.top_nodes(p, groups=[0, -2, 0, 0, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ValueError, match="top_nodes: groups must be an integer array"):
        diffusion.top_nodes(p, groups=np.zeros(10))
    with pytest.raises(ValueError, match="top_nodes: column 'q' has no profile"):
        diffusion.top_nodes(named, ["a", "q"])
    with pytest.raises(ValueError, match="top_nodes: cols must name"):
        diffusion.top_nodes(named)
    with pytest.raises(ValueError, match=r"top_nodes: column index 3 is outside \[0, 3\)"):
        diffusion.top_nodes(p, [0, 3])
    with pytest.raises(ValueError, match="top_nodes: a host profile array must be"):
        diffusion.top_nodes(np.ones(4))
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        diffusion.top_nodes(p, device="cpu")
    idx, cnt = torch.zeros(4, 2, 5, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"top_overlap: a\[1\] = 4 is outside \[0, S=4\)"):
        diffusion.top_overlap(idx, cnt, [0, 4], [0, 1])
    with pytest.raises(ValueError, match=r"top_overlap: b\[0\] = -1 is outside \[0, S=4\)"):
        diffusion.top_overlap(idx, cnt, [0, 1], [-1, 1])
    with pytest.raises(ValueError, match="top_overlap: a lists 2 selections and b 1"):
        diffusion.top_overlap(idx, cnt, [0, 1], [1])
    with pytest.raises(ValueError, match="top_overlap: idx and cnt must be"):
        diffusion.top_overlap(idx, cnt[:3], [0], [1])
    with pytest.raises(ValueError, match=r"top_overlap: G=9 groups is outside"):
        diffusion.top_overlap(torch.zeros(2, 9, 5, dtype=torch.int32), torch.zeros(2, 9, dtype=torch.int32), [0], [1])
    with pytest.raises(_lib.GssError, match="no CPU fallback"):
        diffusion.top_overlap(idx, cnt, [0], [1])


def test_metric_names_are_untouched():
    from gcn_drug_repurposing_amd import diffusion
    assert diffusion.METRICS == ("cityblock", "euclidean", "canberra", "cosine", "correlation")
    assert diffusion.RANK_METRICS == ("spearman",) and diffusion.ALL_METRICS == diffusion.METRICS + ("spearman",)


# ---- explain.py ------------------------------------------------------------------------------------------------------------------------------

def test_explain_check_args():
    from gcn_drug_repurposing_amd import explain as E
    from gcn_drug_repurposing_amd.predict import PredictError
    assert E.check_args(E.DEFAULT_TYPES, 20, "DB1", "C1") == ["protein", "functional_pathway"]
    assert E.check_args("drug, protein", 1024, pairs="p.tsv") == ["drug", "protein"]
    assert E.check_args("indication", 1, treatments=True) == ["indication"]
    assert E.parse_args(["--drug", "D", "--indication", "I"]).top == 20 and E.parse_args([]).types == "protein,functional_pathway"
    cases = [(("gene", 20, "D", "I"), {}, "--types: 'gene' is unknown"), (("protein,protein", 20, "D", "I"), {}, "--types: repeated type"),
             (("", 20, "D", "I"), {}, "--types lists no type"), (("protein", 0, "D", "I"), {}, "--top 0 is outside 1 .. 1024"),
             (("protein", 1025, "D", "I"), {}, "--top 1025 is outside 1 .. 1024"), (("protein", 20), {}, "give either --drug and --indication, or one of"),
             (("protein", 20, "D", "I"), dict(pairs="p.tsv"), "give either --drug and --indication, or one of"),
             (("protein", 20, "D", "I"), dict(treatments=True), "give either"), (("protein", 20, "D"), {}, "needs both --drug and --indication"),
             (("protein", 20, None, "I"), {}, "needs both --drug and --indication"),
             (("protein", 20), dict(pairs="p.tsv", treatments=True), "one of --pairs / --treatments, not both"),
             (("protein", 20), dict(pairs="p.tsv", edges="e.tsv"), "--edges needs a single pair")]
    for args, kw, message in cases:
        with pytest.raises(PredictError) as e:
            E.check_args(*args, **kw)
        assert message in str(e.value), (message, str(e.value))


def test_explain_refuses_before_graph_and_gpu(tmp_path, monkeypatch):
    import predict_fixture as PF
    from gcn_drug_repurposing_amd import _lib, explain as E, predict
    from gcn_drug_repurposing_amd.predict import PredictError
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was loaded before the refusal"))
    monkeypatch.setattr(predict, "build_graph", lambda s: pytest.fail("the graph was built before the refusal"))
    cfg = PF.stage(tmp_path, "diffusion", with_embs=False)
    bad = tmp_path / "bad.tsv"
    bad.write_text("drug\tdisease\nDB00003\tC0000000\n")
    with pytest.raises(PredictError, match="--pairs .*bad.tsv.*: the table needs the columns drug and indication"):
        E.run(cfg, pairs=str(bad))
    with pytest.raises(PredictError, match="config: missing key networks.drug_to_indication"):
        E.run(cfg, treatments=True)
    with pytest.raises(PredictError, match="--types: 'gene' is unknown"):
        E.run(cfg, drug="DB00003", indication="C0000000", types="gene")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env["HIP_VISIBLE_DEVICES"] = "-1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "explain.py"), "-c", cfg, "--drug", "DB00003", "--indication", "C0000000", "--top", "2000"],
                       cwd=str(tmp_path), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2 and r.stderr.strip() == "explain: --top 2000 is outside 1 .. 1024" and r.stdout == ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "explain.py"), "--help"], cwd=str(tmp_path), capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and all(t in r.stdout for t in E.TYPES + ("--treatments", "--pairs", "--edges"))


class Graph:
    def __init__(self, names):
        self.node2name = {n: "name of " + n for n in names}
        self.node2name[names[0]] = None


def test_explain_node_rows_order_and_cells():
    from gcn_drug_repurposing_amd import explain as E
    names = ["n%d" % i for i in range(12)]
    g = Graph(names)
    # type 0: drug ranks 3, 1, 7, 5; indication ranks 5, 9, 3 -> shared 3 (drug rank 1) and 5 (drug rank 4); then 1, 7 (drug only), then 9
    idx = np.array([[[3, 1, 7, 5], [2, -1, -1, -1]], [[5, 9, 3, -1], [-1, -1, -1, -1]]], np.int32)
    cnt = np.array([[4, 1], [3, 0]], np.int32)
    pd, pi = np.arange(12) / 16.0, np.arange(12) / -32.0
    rows = E.node_rows(["protein", "functional_pathway"], idx, cnt, pd, pi, names, g)
    assert [r[0] for r in rows] == ["n3", "n5", "n1", "n7", "n9", "n2"]
    assert [r[2] for r in rows] == ["protein"] * 5 + ["functional_pathway"]
    assert [(r[3], r[5], r[7]) for r in rows] == [(1, 3, 1), (4, 1, 1), (2, "", 0), (3, "", 0), ("", 2, 0), (1, "", 0)]
    assert all(r[4] == pd[int(r[0][1:])] and r[6] == pi[int(r[0][1:])] for r in rows)      # the values are always the profile's
    assert rows[0][1] == "name of n3" and E.node_rows(["protein"], idx[:, :1, :1] * 0, cnt[:, :1] * 0 + 1, pd, pi, names, g)[0][1] is None
    # shared nodes sort by the drug's rank before the indication's
    idx2 = np.array([[[4, 6]], [[6, 4]]], np.int32)
    assert [r[0] for r in E.node_rows(["drug"], idx2, np.array([[2], [2]]), pd, pi, names, g)] == ["n4", "n6"]


def test_explain_pair_rows_and_jaccard():
    from gcn_drug_repurposing_amd import explain as E
    from gcn_drug_repurposing_amd.predict import PredictError
    assert E.jaccard(2, 4, 3) == 2 / 5 and E.jaccard(0, 3, 3) == 0.0 and E.jaccard(3, 3, 3) == 1.0 and np.isnan(E.jaccard(0, 0, 0))
    names = ["n%d" % i for i in range(12)]
    g = Graph(names + ["D", "I", "J"])
    idx = np.array([[[3, 1, 7, 5], [2, -1, -1, -1]], [[5, 9, 3, -1], [-1, -1, -1, -1]], [[7, 5, 1, 3], [2, 4, -1, -1]]], np.int32)
    cnt = np.array([[4, 1], [3, 0], [4, 2]], np.int32)
    where = {"D": 0, "I": 1, "J": 2}
    pairs = [("D", "I"), ("D", "J"), ("D", "I")]
    shared = T.expected_overlap(idx, cnt, [0, 0, 0], [1, 2, 1])
    assert shared.tolist() == [[2, 0], [4, 1], [2, 0]]
    rows = E.pair_rows(["protein", "functional_pathway"], pairs, where, idx, cnt, shared, names, g)
    assert E.pair_header(["protein", "functional_pathway"]) == ["drug", "drug_name", "indication", "indication_name", "shared_protein",
                                                                "jaccard_protein", "nodes_protein", "shared_functional_pathway",
                                                                "jaccard_functional_pathway", "nodes_functional_pathway"]
    assert rows[0] == ["D", "name of D", "I", "name of I", 2, 2 / 5, "n3,n5", 0, 0.0, ""]              # in the order of the drug's ranks
    assert rows[1] == ["D", "name of D", "J", "name of J", 4, 1.0, "n3,n1,n7,n5", 1, 1 / 2, "n2"]
    assert rows[2] == rows[0]
    empty = E.pair_rows(["protein"], [("I", "I")], where, idx[:, 1:], cnt[:, 1:], np.array([[0]]), names, g)
    assert empty[0][4] == 0 and np.isnan(empty[0][5]) and empty[0][6] == ""
    with pytest.raises(PredictError, match="the device counted 3 shared nodes, the lists hold 2"):
        E.pair_rows(["protein"], pairs[:1], where, idx, cnt, np.array([[3]]), names, g)


def test_explain_groups_edges_and_nan_refusal():
    import predict_fixture as PF
    from gcn_drug_repurposing_amd import explain as E
    from gcn_drug_repurposing_amd.predict import PredictError
    g = PF.msi_graph(False)
    names = g.names
    grp = E.node_groups(names, g, ["protein", "functional_pathway"])
    assert grp.dtype == np.int32 and set(grp.tolist()) == {-1, 0, 1}
    assert all((g.type[n] == "protein") == (grp[i] == 0) and (g.type[n] == "functional_pathway") == (grp[i] == 1) for i, n in enumerate(names))
    keep = set(names[:40]) | {"DB00003"}
    rows = E.edge_rows(g, keep)
    adj, order, _ = g.to_csr()
    want = [(order[u], order[v], float(adj[u, v])) for u in range(len(order)) for v in adj.indices[adj.indptr[u]:adj.indptr[u + 1]]
            if order[u] in keep and order[v] in keep]
    assert [tuple(r) for r in rows] == want and len(rows) > 10
    prof = {"DB00003": np.ones(len(names))}
    prof["DB00003"][np.flatnonzero(grp == 1)[3]] = np.nan
    with pytest.raises(PredictError, match=f"the profile of 'DB00003' is NaN at node {names[np.flatnonzero(grp == 1)[3]]!r} .type functional_pathway."):
        E.refuse_nan(["DB00003"], np.array([[5, -1]]), prof, grp, ["protein", "functional_pathway"], names)
    E.refuse_nan(["DB00003"], np.array([[5, 5]]), prof, grp, ["protein", "functional_pathway"], names)
