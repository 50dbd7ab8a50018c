"""What lies between a node and a query besides one shortest path (csrc/trace.hip): the number of shortest paths, the best one under a
node weight, the nodes and edges on them with the share of the paths through each, and the mediators of a query over a list of sources.
The reference's interpret.py names this ("tracing the connections in the networks based on exact connections or computed proximities")
and stops there.

Graph: the directed pattern of a scipy CSR with A[u, v] != 0 for u -> v (MsiGraph.to_csr()[0]).  Toward a target t: d_t(v) hops,
sigma_t(v) shortest paths, with weights the best path (best_next, best).  From a source s: the same on the transposed pattern, a second
handle.  Every count is an exact integer in fp64 (a pass with a count above 2^53 is refused).  No CPU fallback.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from .paths import DEFAULT_MAX_BYTES, MAX_TARGETS, UNREACHABLE, PathsError, csr_arrays

Toward = namedtuple("Toward", "targets dist sigma best best_next levels")
NodeTable = namedtuple("NodeTable", "node hops_from hops_to paths_from through share")
Between = namedtuple("Between", "sources targets length n_paths n_nodes tables mediators toward")


def transpose_arrays(rowptr, col):
    """(rowptr, col) of the transposed pattern, columns ascending (host, scipy)"""
    import scipy.sparse as sp
    n = len(rowptr) - 1
    a = sp.csr_matrix((np.ones(len(col), np.int8), col, rowptr), shape=(n, n)).T.tocsr()
    a.sort_indices()
    return a.indptr.astype(np.int32), a.indices.astype(np.int32)


def check_nodes(what, nodes, n):
    t = np.asarray(nodes, dtype=np.int64).reshape(-1)
    if len(t) == 0:
        raise PathsError(f"{what}: no nodes given")
    bad = t[(t < 0) | (t >= n)]
    if len(bad):
        raise PathsError(f"{what}: {int(bad[0])} is not a node index in [0, {n})")
    return t


def check_weights(weights, q, n):
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (q, n):
        raise PathsError(f"weights: shape {w.shape}, expected one row of {n} per target: ({q}, {n})")
    return w


def edges_between(rowptr, col, table, n_paths, paths_to):
    """the edges u -> v on the shortest paths of one pair, from its node table and the CSR: u and v on them and one hop apart;
    share = sigma^s(u) * sigma_t(v) / sigma_t(s) -> (from, to, share), ordered by (from, to)"""
    pos = {int(v): k for k, v in enumerate(table.node)}
    out_u, out_v, out_s = [], [], []
    for k, u in enumerate(table.node):
        for v in col[rowptr[u]:rowptr[u + 1]]:
            j = pos.get(int(v))
            if j is not None and int(table.hops_from[j]) == int(table.hops_from[k]) + 1 and int(table.hops_to[j]) == int(table.hops_to[k]) - 1:
                out_u.append(int(u))
                out_v.append(int(v))
                out_s.append(table.paths_from[k] * paths_to[int(v)] / n_paths)
    return np.asarray(out_u, np.int32), np.asarray(out_v, np.int32), np.asarray(out_s, np.float64)


def follow_best(toward, q, v):
    """node indices v, ..., t_q along best_next, or None where t_q is unreachable"""
    if toward is None or toward.best_next is None:
        raise PathsError("best_path: run .toward(targets, weights) first")
    v = int(v)
    d = int(toward.dist[q, v])
    if d == UNREACHABLE:
        return None
    out = [v]
    for _ in range(d):
        v = int(toward.best_next[q, v])
        out.append(v)
    if v != int(toward.targets[q]):
        raise PathsError(f"best_path: following best_next from {out[0]} did not end at target {int(toward.targets[q])}")
    return out


class _Pass:
    """one device pass of a handle: dist, next, sigma (and w, best, best_next) [64, N] buffers, reused by every pass"""

    def __init__(self, tracer, handle, weighted):
        import torch
        dev = torch.device("cuda")
        n = tracer.n
        self.t, self.h = tracer, handle
        self.dist = torch.empty((MAX_TARGETS, n), dtype=torch.uint8, device=dev)
        self.next = torch.empty((MAX_TARGETS, n), dtype=torch.int32, device=dev)
        self.sigma = torch.empty((MAX_TARGETS, n), dtype=torch.float64, device=dev)
        self.w = self.best = self.best_next = None
        if weighted:
            self.w = torch.empty((MAX_TARGETS, n), dtype=torch.float64, device=dev)
            self.best = torch.empty((MAX_TARGETS, n), dtype=torch.float64, device=dev)
            self.best_next = torch.empty((MAX_TARGETS, n), dtype=torch.int32, device=dev)

    def run(self, nodes, weights=None):
        """nodes: int32 [q <= 64]; weights: host fp64 [q, N] or None -> levels"""
        import ctypes as C

        import torch

        from . import _lib
        t, lib = self.t, self.t.lib
        q = len(nodes)
        lv = C.c_int32(0)
        t._check(lib.gss_paths_run(self.h, q, nodes.ctypes.data, _lib.ptr(self.dist), _lib.ptr(self.next), C.byref(lv), _lib.current_stream()),
                 "gss_paths_run")
        if weights is not None:
            self.w[:q].copy_(torch.from_numpy(weights))
        wt = weights is not None
        t._check(lib.gss_paths_count(self.h, q, nodes.ctypes.data, _lib.ptr(self.dist), lv.value, _lib.ptr(self.w if wt else None),
                                     _lib.ptr(self.sigma), _lib.ptr(self.best if wt else None), _lib.ptr(self.best_next if wt else None),
                                     _lib.current_stream()), "gss_paths_count")
        return int(lv.value)


class PathTracer:
    """PathTracer(adj_csr): two gss_paths handles, one on A and one on its transpose.
    .toward(targets, weights=None) -> Toward(targets, dist, sigma, best, best_next, levels), host arrays [Q, N], kept for .best_path
    .from_(sources) -> (dist, sigma): hops and shortest paths s -> v
    .between(sources, targets, pairs=None, weights=None, mediators=True) -> Between
    .best_path(q, v) -> [v, ..., t_q] along best_next, or None"""

    def __init__(self, adj_csr, max_bytes=DEFAULT_MAX_BYTES):
        from . import _lib
        if isinstance(adj_csr, tuple):
            rowptr, col = (np.ascontiguousarray(x, dtype=np.int32) for x in adj_csr)
        else:
            rowptr, col = csr_arrays(adj_csr)
        self.n = len(rowptr) - 1
        if self.n < 1:
            raise PathsError("the graph has no nodes")
        self.rowptr, self.col = rowptr, col
        self.max_bytes = int(max_bytes)
        self.lib = _lib.load()
        self._fwd = self._bwd = None
        self._fwd = self._create(rowptr, col)
        self._bwd = self._create(*transpose_arrays(rowptr, col))
        self._passes = {}
        self.last = None

    def _create(self, rowptr, col):
        import ctypes as C

        from . import _lib
        col_buf = col if len(col) else np.zeros(1, np.int32)
        h = C.c_void_p()
        self._check(self.lib.gss_paths_create(C.byref(h), self.n, len(col), rowptr.ctypes.data, col_buf.ctypes.data, 0, self.max_bytes,
                                              _lib.current_stream()), "gss_paths_create")
        return h

    def _check(self, rc, what):
        if rc != 0:
            from . import _lib
            msg = self.lib.gss_last_error().decode(errors="replace")
            cls = PathsError if rc == -22 else _lib.GssError
            raise cls(f"{what}: {msg}")

    def close(self):
        self._passes = {}
        for name in ("_fwd", "_bwd"):
            h = getattr(self, name, None)
            if h is not None and h.value:
                self.lib.gss_paths_destroy(h)
            setattr(self, name, None)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _pass(self, side, weighted):
        if self._fwd is None:
            raise PathsError("the tracer is closed")
        per = 33 if weighted else 13
        need = per * MAX_TARGETS * self.n + 24 * self.n
        if need > self.max_bytes:
            raise PathsError(f"a pass of {MAX_TARGETS} needs {need} bytes ({per} Q N + 24 N, N={self.n}), above the budget max_bytes={self.max_bytes}")
        key = (side, weighted)
        if key not in self._passes:
            self._passes[key] = _Pass(self, self._fwd if side == "toward" else self._bwd, weighted)
        return self._passes[key]

    def _sweep(self, side, nodes, weights):
        t = check_nodes(side, nodes, self.n)
        w = check_weights(weights, len(t), self.n)
        p = self._pass(side, w is not None)
        out = self._host(t, w is not None)
        for lo in range(0, len(t), MAX_TARGETS):
            sub = np.ascontiguousarray(t[lo:lo + MAX_TARGETS], dtype=np.int32)
            out.levels.append(p.run(sub, None if w is None else w[lo:lo + len(sub)]))
            self._fetch(p, out, lo, len(sub))
        return out

    def _host(self, t, weighted):
        """the host tables of a sweep over the nodes t, to be filled pass by pass"""
        shape = (len(t), self.n)
        return Toward(t, np.empty(shape, np.uint8), np.empty(shape, np.float64), np.empty(shape, np.float64) if weighted else None,
                      np.empty(shape, np.int32) if weighted else None, [])

    @staticmethod
    def _fetch(p, out, lo, k):
        out.dist[lo:lo + k] = p.dist[:k].cpu().numpy()
        out.sigma[lo:lo + k] = p.sigma[:k].cpu().numpy()
        if out.best is not None:
            out.best[lo:lo + k] = p.best[:k].cpu().numpy()
            out.best_next[lo:lo + k] = p.best_next[:k].cpu().numpy()

    def toward(self, targets, weights=None):
        self.last = self._sweep("toward", targets, weights)
        return self.last

    def from_(self, sources):
        r = self._sweep("from", sources, None)
        return r.dist, r.sigma

    def best_path(self, q, v):
        return follow_best(self.last, q, v)

    def between(self, sources, targets, pairs=None, weights=None, mediators=True):
        """sources [S], targets [T] node indices; pairs: (i, j) positions whose node tables are wanted (None: none, "all": every pair).
        -> Between: length int32 [S, T] (-1 unreachable), n_paths fp64 [S, T], n_nodes int32 [S, T] (end points included),
        tables {(i, j): NodeTable}, mediators (M fp64 [T, N], C int32 [T, N]) or None, toward (the Toward of the targets)"""
        import torch

        from . import _lib
        s_all = check_nodes("between: sources", sources, self.n)
        t_all = check_nodes("between: targets", targets, self.n)
        w = check_weights(weights, len(t_all), self.n)
        S, T, n = len(s_all), len(t_all), self.n
        if pairs == "all":
            pairs = [(i, j) for i in range(S) for j in range(T)]
        pairs = [(int(i), int(j)) for i, j in (pairs or [])]
        for i, j in pairs:
            if not (0 <= i < S and 0 <= j < T):
                raise PathsError(f"between: pair ({i}, {j}) is outside the {S} sources x {T} targets")
        dev = torch.device("cuda")
        length = np.empty((S, T), np.int32)
        n_paths = np.empty((S, T), np.float64)
        n_nodes = np.empty((S, T), np.int32)
        M = np.zeros((T, n), np.float64) if mediators else None
        Cn = np.zeros((T, n), np.int32) if mediators else None
        tables = {}
        tw = self._host(t_all, w is not None)
        pt, ps = self._pass("toward", w is not None), self._pass("from", False)
        d_len = torch.empty((MAX_TARGETS, MAX_TARGETS), dtype=torch.int32, device=dev)
        d_paths = torch.empty((MAX_TARGETS, MAX_TARGETS), dtype=torch.float64, device=dev)
        d_nodes = torch.empty((MAX_TARGETS, MAX_TARGETS), dtype=torch.int32, device=dev)
        st = _lib.current_stream
        for tlo in range(0, T, MAX_TARGETS):
            tsub = np.ascontiguousarray(t_all[tlo:tlo + MAX_TARGETS], dtype=np.int32)
            nt = len(tsub)
            tw.levels.append(pt.run(tsub, None if w is None else w[tlo:tlo + nt]))
            self._fetch(pt, tw, tlo, nt)
            d_M = torch.zeros((nt, n), dtype=torch.float64, device=dev) if mediators else None
            d_C = torch.zeros((nt, n), dtype=torch.int32, device=dev) if mediators else None
            for slo in range(0, S, MAX_TARGETS):
                ssub = np.ascontiguousarray(s_all[slo:slo + MAX_TARGETS], dtype=np.int32)
                ns = len(ssub)
                ps.run(ssub)
                ids = (n, ns, ssub.ctypes.data, _lib.ptr(ps.dist), _lib.ptr(ps.sigma), nt, tsub.ctypes.data, _lib.ptr(pt.dist), _lib.ptr(pt.sigma))
                self._check(self.lib.gss_paths_between(*ids, _lib.ptr(d_len), _lib.ptr(d_paths), _lib.ptr(d_nodes), _lib.ptr(d_M), _lib.ptr(d_C),
                                                       st()), "gss_paths_between")
                # the three tables are [ns][nt] with row stride nt in the first ns * nt words of their buffers
                k = ns * nt
                length[slo:slo + ns, tlo:tlo + nt] = d_len.view(-1)[:k].cpu().numpy().reshape(ns, nt)
                n_paths[slo:slo + ns, tlo:tlo + nt] = d_paths.view(-1)[:k].cpu().numpy().reshape(ns, nt)
                n_nodes[slo:slo + ns, tlo:tlo + nt] = d_nodes.view(-1)[:k].cpu().numpy().reshape(ns, nt)
                chosen = [(i, j) for i, j in pairs if slo <= i < slo + ns and tlo <= j < tlo + nt]
                if chosen:
                    counts = np.array([n_nodes[i, j] for i, j in chosen], np.int64)
                    offset = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                    cap = int(offset[-1])
                    local = np.array([(i - slo, j - tlo) for i, j in chosen], np.int32)
                    d_pairs, d_off = torch.from_numpy(local).to(dev), torch.from_numpy(offset).to(dev)
                    size = max(cap, 1)
                    o_node = torch.empty(size, dtype=torch.int32, device=dev)
                    o_hf, o_ht = (torch.empty(size, dtype=torch.uint8, device=dev) for _ in range(2))
                    o_pf, o_th, o_sh = (torch.empty(size, dtype=torch.float64, device=dev) for _ in range(3))
                    self._check(self.lib.gss_paths_between_fill(*ids, len(chosen), _lib.ptr(d_pairs), _lib.ptr(d_off), cap, _lib.ptr(o_node),
                                                                _lib.ptr(o_hf), _lib.ptr(o_ht), _lib.ptr(o_pf), _lib.ptr(o_th), _lib.ptr(o_sh), st()),
                                "gss_paths_between_fill")
                    cols = [x.cpu().numpy() for x in (o_node, o_hf, o_ht, o_pf, o_th, o_sh)]
                    for p, (i, j) in enumerate(chosen):
                        a, b = int(offset[p]), int(offset[p + 1])
                        tables[(i, j)] = NodeTable(*(c[a:b].copy() for c in cols))
            if mediators:
                M[tlo:tlo + nt] = d_M.cpu().numpy()
                Cn[tlo:tlo + nt] = d_C.cpu().numpy()
        self.last = tw
        return Between(s_all, t_all, length, n_paths, n_nodes, tables, (M, Cn) if mediators else None, tw)
