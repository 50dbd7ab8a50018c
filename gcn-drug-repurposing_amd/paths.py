"""Shortest-path trees toward a set of target nodes on the device (csrc/paths.hip): the "shortest path to Covid" and "path length"
columns of predict_drug.output_drugs (predict_drug.py:268-273) and run_covid.py:310-319, which ran one networkx search per row.

One pass answers up to 64 targets for every source node at once: dist [Q, N] (hop count of the shortest directed path v -> t_q, 255 =
unreachable) and next [Q, N] (its first hop, -1 at t_q and where t_q is unreachable).  The tie rule is the contract: next is the
successor with the smallest node index that is one hop closer.  No CPU fallback: without the library or a GPU this raises.
"""
from __future__ import annotations

import numpy as np

MAX_TARGETS = 64                  # targets per pass (one bit of a uint64 each)
DEFAULT_MAX_BYTES = 1 << 30       # budget of one pass: 5 Q N bytes of output + 24 N of state
UNREACHABLE = 255


class PathsError(ValueError):
    pass


def csr_arrays(adj):
    """(rowptr int32 [N+1], col int32) of a square scipy CSR, columns ascending within each row"""
    import scipy.sparse as sp
    adj = sp.csr_matrix(adj)
    if adj.shape[0] != adj.shape[1]:
        raise PathsError(f"the adjacency must be square, got {adj.shape}")
    if not adj.has_sorted_indices:
        adj = adj.copy()
        adj.sort_indices()
    if adj.nnz > np.iinfo(np.int32).max:
        raise PathsError(f"{adj.nnz} entries do not fit int32 row pointers")
    return adj.indptr.astype(np.int32), adj.indices.astype(np.int32)


class ShortestPathTrees:
    """ShortestPathTrees(adj_csr).to(targets) -> (dist uint8 [Q, N], next int32 [Q, N]) on the host; .path(q, v) -> [v, ..., t_q] or
    None.  adj_csr: scipy CSR with A[u, v] != 0 for the directed edge u -> v (MsiGraph.to_csr()[0]), or a (rowptr, col) pair."""

    def __init__(self, adj_csr, max_bytes=DEFAULT_MAX_BYTES):
        import ctypes as C

        from . import _lib
        if isinstance(adj_csr, tuple):
            rowptr, col = (np.ascontiguousarray(x, dtype=np.int32) for x in adj_csr)
        else:
            rowptr, col = csr_arrays(adj_csr)
        self.n = len(rowptr) - 1
        if self.n < 1:
            raise PathsError("the graph has no nodes")
        self.max_bytes = int(max_bytes)
        self.lib = _lib.load()
        col_buf = col if len(col) else np.zeros(1, np.int32)
        h = C.c_void_p()
        self._check(self.lib.gss_paths_create(C.byref(h), self.n, len(col), rowptr.ctypes.data, col_buf.ctypes.data, 0, self.max_bytes,
                                              _lib.current_stream()), "gss_paths_create")
        self._h = h
        self.targets = None
        self.dist = None
        self.next = None
        self.levels = []

    def _check(self, rc, what):
        if rc != 0:
            from . import _lib
            msg = self.lib.gss_last_error().decode(errors="replace")
            cls = PathsError if rc == -22 else _lib.GssError
            raise cls(f"{what}: {msg}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.gss_paths_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def to(self, targets):
        """shortest-path trees toward every target, ceil(Q / 64) device passes -> (dist [Q, N] uint8, next [Q, N] int32), kept for .path"""
        import ctypes as C

        import torch

        from . import _lib
        t = np.asarray(targets, dtype=np.int64).reshape(-1)
        if len(t) == 0:
            raise PathsError("to: no targets (Q = 0)")
        bad = t[(t < 0) | (t >= self.n)]
        if len(bad):
            raise PathsError(f"to: target {int(bad[0])} is not a node index in [0, {self.n})")
        if self._h is None:
            raise PathsError("to: the handle is closed")
        q_pass = min(MAX_TARGETS, len(t))
        need = 5 * q_pass * self.n + 24 * self.n
        if need > self.max_bytes:
            raise PathsError(f"to: a pass of {q_pass} targets needs {need} bytes (5 Q N + 24 N, N={self.n}), above the budget "
                             f"max_bytes={self.max_bytes}")
        dev = torch.device("cuda")
        dist = np.empty((len(t), self.n), np.uint8)
        nxt = np.empty((len(t), self.n), np.int32)
        d_dist = torch.empty((q_pass, self.n), dtype=torch.uint8, device=dev)
        d_next = torch.empty((q_pass, self.n), dtype=torch.int32, device=dev)
        self.levels = []
        for lo in range(0, len(t), MAX_TARGETS):
            sub = np.ascontiguousarray(t[lo:lo + MAX_TARGETS], dtype=np.int32)
            lv = C.c_int32(0)
            self._check(self.lib.gss_paths_run(self._h, len(sub), sub.ctypes.data, _lib.ptr(d_dist), _lib.ptr(d_next), C.byref(lv),
                                               _lib.current_stream()), "gss_paths_run")
            dist[lo:lo + len(sub)] = d_dist[:len(sub)].cpu().numpy()
            nxt[lo:lo + len(sub)] = d_next[:len(sub)].cpu().numpy()
            self.levels.append(int(lv.value))
        self.targets, self.dist, self.next = t, dist, nxt
        return dist, nxt

    def path(self, q, v):
        """node indices v, ..., t_q of the shortest path v -> t_q (the tie rule's), or None when t_q is unreachable from v"""
        return follow(self.dist, self.next, self.targets, q, v)


def follow(dist, nxt, targets, q, v):
    """walk next from v to targets[q] -> [v, ..., t_q] or None (host; the tables need a few thousand of these)"""
    if dist is None:
        raise PathsError("path: run .to(targets) first")
    v = int(v)
    d = int(dist[q, v])
    if d == UNREACHABLE:
        return None
    out = [v]
    for _ in range(d):
        v = int(nxt[q, v])
        out.append(v)
    if v != int(targets[q]):
        raise PathsError(f"path: following next from {out[0]} did not end at target {int(targets[q])}")
    return out
