"""numpy / scipy mirror of csrc/paths.hip: dist from a breadth-first search toward each target (scipy.sparse.csgraph on the transposed
graph), next as the smallest-index successor one hop closer (the tie rule).  Test-side only."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import shortest_path


def mirror_trees(adj, targets):
    """adj: CSR with A[u, v] != 0 for u -> v.  -> (dist uint8 [Q, N] (255 = unreachable), next int32 [Q, N] (-1 at the target / unreachable))"""
    adj = sp.csr_matrix(adj)
    n = adj.shape[0]
    pattern = sp.csr_matrix((np.ones(adj.nnz, np.float64), adj.indices, adj.indptr), shape=adj.shape)
    targets = np.asarray(targets, np.int64)
    d = shortest_path(pattern.T.tocsr(), method="D", unweighted=True, indices=targets)   # [Q, N]: hops from the target on A^T
    d = np.atleast_2d(d)
    fin = np.isfinite(d)
    dist = np.where(fin, d, 255).astype(np.uint8)
    rows = np.repeat(np.arange(n), np.diff(adj.indptr))
    cols = adj.indices.astype(np.int64)
    nxt = np.full((len(targets), n), -1, np.int32)
    for q in range(len(targets)):
        dq = np.where(fin[q], d[q], np.inf)
        ok = np.isfinite(dq[rows]) & (dq[cols] == dq[rows] - 1)
        best = np.full(n, n, np.int64)
        np.minimum.at(best, rows[ok], cols[ok])
        has = best < n
        nxt[q, has] = best[has]
    return dist, nxt


def follow(dist, nxt, t, v):
    if dist[v] == 255:
        return None
    out = [int(v)]
    while out[-1] != t:
        out.append(int(nxt[out[-1]]))
    return out
