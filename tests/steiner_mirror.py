"""The definition of gss_steiner_trees (include/gssgcn.h) in numpy and plain Python: Mehlhorn's form of the Kou-Markowsky-Berman Steiner
tree approximation on unit weights.  1. a level-by-level search from all terminals leaves in every node (dist, src): the distance to the
nearest terminal and the smallest position among the nearest.  2. the bridges -- edges u < v whose ends have different src -- are
sorted by (w, u, v), w = dist(u) + dist(v) + 1, and Kruskal takes the minimum spanning forest of the terminals.  3. the parent chains
from both ends of every chosen bridge are walked; parent(x) is the smallest neighbour one level nearer to the same terminal.

ABLATIONS names plausible wrong rules; tree(..., ablation=name) computes with one of them.  tests/test_steiner_mirror.py shows that each
changes an asserted output on some case of tests/steiner_cases.py."""
from __future__ import annotations

import heapq

import numpy as np

ABLATIONS = ("src_larger", "order_wvu", "parent_largest", "parent_any_src", "prim_first_found", "w_without_one")
COUNTS = ("n_comp", "length", "n_steiner", "n_edges", "max_w")
FAR = np.iinfo(np.int64).max


def nearest(rowptr, col, terminals, larger=False):
    """-> (dist, src) int64 [n], -1 where no terminal reaches; src = the smallest (with `larger` the largest) position among the nearest
    terminals; and the number of nodes at which two neighbours one level nearer disagreed on src (where the rule decided)"""
    n = len(rowptr) - 1
    dist, src = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    frontier = np.asarray(terminals, np.int64)
    dist[frontier], src[frontier] = 0, np.arange(len(frontier))
    level, decided = 0, 0
    while len(frontier):
        deg = (rowptr[frontier + 1] - rowptr[frontier]).astype(np.int64)
        start = np.repeat(rowptr[frontier].astype(np.int64) - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg)
        nb = col[start + np.arange(int(deg.sum()))].astype(np.int64)
        s = np.repeat(src[frontier], deg)
        new = dist[nb] < 0
        nb, s = nb[new], s[new]
        lo, hi = np.full(n, FAR), np.full(n, -1, np.int64)
        np.minimum.at(lo, nb, s)
        np.maximum.at(hi, nb, s)
        frontier = np.unique(nb)
        level += 1
        dist[frontier], src[frontier] = level, (hi if larger else lo)[frontier]
        decided += int((lo[frontier] != hi[frontier]).sum())
    return dist, src, decided


def bridges(rowptr, col, dist, src, plus=1):
    """-> (u, v, w) of every bridge, in the CSR's order"""
    n = len(rowptr) - 1
    u = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    v = col.astype(np.int64)
    keep = (u < v) & (dist[u] >= 0) & (dist[v] >= 0)
    keep[keep] = src[u[keep]] != src[v[keep]]
    u, v = u[keep], v[keep]
    return u, v, dist[u] + dist[v] + plus


def kruskal(T, u, v, w, a, b, order):
    """the bridges (u, v, w) between terminals (a, b), taken in `order` -> (indices of the chosen, how often the next bridge of the same
    weight would also have joined two components: where the order past w decided which went first)"""
    root = list(range(T))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i

    chosen, ties = [], 0
    a, b, w = a[order].tolist(), b[order].tolist(), w[order].tolist()
    for i in range(len(a)):
        ra, rb = find(a[i]), find(b[i])
        if ra == rb:
            continue
        if i + 1 < len(a) and w[i + 1] == w[i] and find(a[i + 1]) != find(b[i + 1]):
            ties += 1
        root[max(ra, rb)] = min(ra, rb)
        chosen.append(int(order[i]))
        if len(chosen) == T - 1:
            break
    return chosen, ties


def prim_first_found(T, u, v, w, a, b):
    """the wrong rule: per pair of terminals the first bridge found of the least weight, then Prim from terminal 0 (and from the smallest
    terminal not yet reached), ties to the bridge pushed first"""
    pair = {}
    for i in range(len(u)):
        k = (min(a[i], b[i]), max(a[i], b[i]))
        if k not in pair or w[i] < w[pair[k]]:
            pair[k] = i
    adj = [[] for _ in range(T)]
    for (p, q), i in pair.items():
        adj[p].append((q, i))
        adj[q].append((p, i))
    seen, chosen, pushed = [False] * T, [], 0
    for start in range(T):
        if seen[start]:
            continue
        seen[start] = True
        heap = []
        for q, i in adj[start]:
            heapq.heappush(heap, (int(w[i]), pushed, q, i))
            pushed += 1
        while heap:
            _, _, q, i = heapq.heappop(heap)
            if seen[q]:
                continue
            seen[q] = True
            chosen.append(i)
            for r, j in adj[q]:
                if not seen[r]:
                    heapq.heappush(heap, (int(w[j]), pushed, r, j))
                    pushed += 1
    return chosen


def tree(rowptr, col, terminals, ablation=None):
    """one unit -> {"dist", "src": int64 [n]; the COUNTS; "steiner": the Steiner nodes ascending, "parent": theirs; "bridge": int64 [k, 2]
    ascending; "edges": [(a, b, kind)] the parent edges ("path", a the child) in the order of "steiner" and then the bridges;
    "src_decided", "order_decided": the tie counts of nearest() and kruskal()}"""
    assert ablation is None or ablation in ABLATIONS, ablation
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    terminals = np.asarray(terminals, np.int64)
    T = len(terminals)
    dist, src, src_decided = nearest(rowptr, col, terminals, larger=ablation == "src_larger")
    u, v, w = bridges(rowptr, col, dist, src, plus=0 if ablation == "w_without_one" else 1)
    a, b = src[u], src[v]
    order_decided = 0
    if ablation == "prim_first_found":
        chosen = prim_first_found(T, u, v, w, a.tolist(), b.tolist())
    else:
        order = np.lexsort((u, v, w) if ablation == "order_wvu" else (v, u, w))
        chosen, order_decided = kruskal(T, u, v, w, a, b, order)
    chosen = sorted(chosen, key=lambda i: (u[i], v[i]))
    bridge = np.array([(u[i], v[i]) for i in chosen], np.int64).reshape(-1, 2)
    parent = {}
    for x in bridge.ravel().tolist():
        while dist[x] > 0 and x not in parent:
            nb = col[rowptr[x]:rowptr[x + 1]].astype(np.int64)
            ok = dist[nb] == dist[x] - 1
            if ablation != "parent_any_src":
                ok &= src[nb] == src[x]
            parent[x] = int(nb[ok].max() if ablation == "parent_largest" else nb[ok].min())
            x = parent[x]
    steiner = np.array(sorted(parent), np.int64)
    weights = w[chosen] if len(chosen) else np.zeros(0, np.int64)
    out = {"dist": dist, "src": src, "n_comp": T - len(chosen), "length": int(weights.sum()), "n_steiner": len(steiner),
           "n_edges": len(steiner) + len(chosen), "max_w": int(weights.max()) if len(chosen) else 0,
           "steiner": steiner, "parent": np.array([parent[x] for x in steiner.tolist()], np.int64), "bridge": bridge,
           "src_decided": src_decided, "order_decided": order_decided}
    out["edges"] = [(int(x), parent[int(x)], "path") for x in steiner] + [(int(p), int(q), "bridge") for p, q in bridge]
    return out


def table(rowptr, col, units, ablation=None):
    """every unit -> {the COUNTS: int32 [U]; "steiner", "parent", "bridge", "edges": lists over units; "src_decided", "order_decided": int64 [U]}"""
    trees = [tree(rowptr, col, t, ablation) for t in units]
    out = {f: np.array([t[f] for t in trees], np.int32) for f in COUNTS}
    out.update({f: [t[f] for t in trees] for f in ("steiner", "parent", "bridge", "edges")})
    out.update({f: np.array([t[f] for t in trees], np.int64) for f in ("src_decided", "order_decided")})
    return out
