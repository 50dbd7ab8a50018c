"""numpy restatement of csrc/trace.hip on top of paths_mirror.mirror_trees: shortest-path counts, best paths, the nodes between pairs and
the mediators, in the arithmetic the contract fixes (include/gssgcn.h), so the device results equal these to the bit.  Test-side only.
MirrorTracer has PathTracer's interface and stands in for it where there is no GPU."""
import numpy as np
import scipy.sparse as sp

from paths_mirror import mirror_trees

LIMIT = 2.0 ** 53


class CountRefused(ValueError):
    pass


def _edges(adj):
    adj = sp.csr_matrix(adj)
    adj.sort_indices()
    rows = np.repeat(np.arange(adj.shape[0]), np.diff(adj.indptr)).astype(np.int64)
    return rows, adj.indices.astype(np.int64)


def mirror_toward(adj, targets, weights=None):
    """-> (dist uint8 [Q, N], sigma fp64 [Q, N], best fp64 [Q, N] or None, best_next int32 [Q, N] or None)"""
    adj = sp.csr_matrix(adj)
    n = adj.shape[0]
    targets = np.asarray(targets, np.int64).reshape(-1)
    dist, _ = mirror_trees(adj, targets)
    rows, cols = _edges(adj)
    Q = len(targets)
    sigma = np.zeros((Q, n), np.float64)
    best = nb = None
    if weights is not None:
        weights = np.asarray(weights, np.float64)
        assert weights.shape == (Q, n)
        if not np.isfinite(weights).all():
            q, v = np.argwhere(~np.isfinite(weights))[0]
            raise CountRefused(f"the weight of node {v} for target {q} is not finite")
        best = np.zeros((Q, n), np.float64)
        nb = np.full((Q, n), -1, np.int32)
    for q in range(Q):
        d = dist[q].astype(np.int64)
        sigma[q, d == 0] = 1.0
        finite = d[d != 255]
        for L in range(1, int(finite.max()) + 1 if len(finite) else 1):
            m = (d[rows] == L) & (d[cols] == L - 1)        # a self loop never passes: d[v] != d[v] - 1
            r, c = rows[m], cols[m]
            s = np.bincount(r, weights=sigma[q, c], minlength=n)
            at = d == L
            if (s[at] >= LIMIT).any():                      # exact integers only: redo the level in Python's integers
                exact = {}
                for a, b in zip(r, c):
                    exact[a] = exact.get(a, 0) + int(sigma[q, b])
                over = [a for a, x in exact.items() if x > 2 ** 53]
                if over:
                    raise CountRefused(f"node {min(over)} has more than 2^53 shortest paths to target {q}")
            sigma[q, at] = s[at]
            if weights is not None:
                # per row the successor with the largest best, the smallest index on equal values: keys rows, -best, cols
                order = np.lexsort((c, -best[q, c], r))
                r2, c2 = r[order], c[order]
                first = np.ones(len(r2), bool)
                first[1:] = r2[1:] != r2[:-1]
                v, u = r2[first], c2[first]
                nb[q, v] = u
                best[q, v] = weights[q, v] + best[q, u]
    return dist, sigma, best, nb


def mirror_from(adj, sources):
    d, s, _, _ = mirror_toward(sp.csr_matrix(adj).T.tocsr(), sources)
    return d, s


def on_path(ds, dt, D):
    return (ds != 255) & (dt != 255) & (ds.astype(np.int64) + dt.astype(np.int64) == D)


def mirror_between(adj, sources, targets, pairs=(), weights=None, mediators=True):
    """-> dict with the fields of trace.Between"""
    sources = np.asarray(sources, np.int64).reshape(-1)
    targets = np.asarray(targets, np.int64).reshape(-1)
    n = sp.csr_matrix(adj).shape[0]
    dt, st, best, nb = mirror_toward(adj, targets, weights)
    ds, ss = mirror_from(adj, sources)
    S, T = len(sources), len(targets)
    length = np.full((S, T), -1, np.int32)
    n_paths = np.zeros((S, T), np.float64)
    n_nodes = np.zeros((S, T), np.int32)
    M = np.zeros((T, n), np.float64)
    C = np.zeros((T, n), np.int32)
    for i, s in enumerate(sources):                       # list order: the order of the mediator sums
        D = dt[:, s].astype(np.int64)                     # [T]
        ok = D != 255
        on = on_path(ds[i][None, :], dt, D[:, None]) & ok[:, None]          # [T, N]
        length[i, ok] = D[ok]
        n_paths[i, ok] = st[ok, s]
        n_nodes[i] = on.sum(1)
        if mediators:
            inner = on & (ds[i] != 0)[None, :] & (dt != 0)
            tt, vv = np.nonzero(inner)
            M[tt, vv] = M[tt, vv] + (ss[i, vv] * st[tt, vv]) / st[tt, s]
            C[tt, vv] += 1
    tables = {}
    for i, j in pairs:
        if length[i, j] < 0:
            tables[(i, j)] = tuple(np.zeros(0, t) for t in (np.int32, np.uint8, np.uint8, np.float64, np.float64, np.float64))
            continue
        v = np.nonzero(on_path(ds[i], dt[j], int(length[i, j])))[0]
        through = ss[i, v] * st[j, v]
        tables[(i, j)] = (v.astype(np.int32), ds[i, v], dt[j, v], ss[i, v], through, through / st[j, sources[i]])
    return dict(sources=sources, targets=targets, length=length, n_paths=n_paths, n_nodes=n_nodes, tables=tables,
                mediators=(M, C) if mediators else None, toward=(targets, dt, st, best, nb))


class MirrorTracer:
    """trace.PathTracer's interface on the mirror (the CLI's injectable tracer in the CPU tests)"""

    def __init__(self, adj_csr):
        from gcn_drug_repurposing_amd.paths import csr_arrays
        self.adj = sp.csr_matrix(adj_csr)
        self.rowptr, self.col = csr_arrays(self.adj)
        self.n = self.adj.shape[0]
        self.last = None

    def close(self):
        pass

    def toward(self, targets, weights=None):
        from gcn_drug_repurposing_amd.trace import Toward
        d, s, b, nb = mirror_toward(self.adj, targets, weights)
        self.last = Toward(np.asarray(targets, np.int64), d, s, b, nb, [])
        return self.last

    def from_(self, sources):
        return mirror_from(self.adj, sources)

    def best_path(self, q, v):
        from gcn_drug_repurposing_amd.trace import follow_best
        return follow_best(self.last, q, v)

    def between(self, sources, targets, pairs=None, weights=None, mediators=True):
        from gcn_drug_repurposing_amd.trace import Between, NodeTable, Toward
        if pairs == "all":
            pairs = [(i, j) for i in range(len(sources)) for j in range(len(targets))]
        r = mirror_between(self.adj, sources, targets, pairs or (), weights, mediators)
        self.last = Toward(*r["toward"], [])
        return Between(r["sources"], r["targets"], r["length"], r["n_paths"], r["n_nodes"],
                       {k: NodeTable(*t) for k, t in r["tables"].items()}, r["mediators"], self.last)
