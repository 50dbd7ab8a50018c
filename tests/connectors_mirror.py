"""Numpy / plain Python statement of the seed connector growth of csrc/seed_connect.hip (include/gssgcn.h has the definition), for tests
and for tools/connectors_bench.py's baseline only.

  * grow(rowptr, col, seeds, n_add): one unit.  M = the seeds in their order, then the added nodes in the order added; comp[i] is the
    position in M of the smallest member of i's component (a plain union-find over the seeds' induced edges first, the smaller root
    kept; after that the components are kept flat).  A step: for every node v outside M with a neighbour in M, tot(v) = 1 + the sizes
    of the DISTINCT components among its neighbours, L'(v) = max(L, tot(v)); the candidate with the smallest (-L', deg, v) is added
    unless there is none or its L' < L + 2.  Beside the outputs of the entry point it reports per step how many candidates shared the
    winner's L' (ties_lcc) and its (L', deg) (ties_deg): where ties_lcc > 1 = ties_deg the degree decided, where ties_deg > 1 the node;
    and the step's work: the candidates, the CSR entries of their rows, the most components next to one candidate;
  * table(rowptr, col, units, n_add): the entry point's arrays for a list of units;
  * largest_root(comp): the root of the largest component, of two as large the smaller (the final LCC the summaries refer to).
"""
from __future__ import annotations

import numpy as np

STEP_FIELDS = ("node", "lcc", "merged", "deg")
COUNT_FIELDS = ("ties_lcc", "ties_deg", "candidates", "entries", "most_merged")   # per step, for the tests and the cost model
UNIT_FIELDS = ("steps", "first_lcc", "final_lcc", "seeds_in", "added_in")


def _seed_components(rowptr, col, seeds, pos):
    """comp [len(seeds)]: the plain union-find over the hits of every seed's row in the seed list, the smaller root kept"""
    m = len(seeds)
    parent = list(range(m))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for i, v in enumerate(seeds):
        for c in col[rowptr[v]:rowptr[v + 1]]:
            j = pos[c]
            if j >= 0 and j != i:
                a, b = find(i), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(m)], np.int64)


def largest_root(comp):
    """the root of the largest component (None when there is no member); of two as large the smaller root"""
    comp = np.asarray(comp, np.int64)
    if len(comp) == 0:
        return None
    return int(np.argmax(np.bincount(comp)))          # argmax returns the first of equal counts


def grow(rowptr, col, seeds, n_add, on_step=None):
    """-> dict: node, lcc, merged, deg and COUNT_FIELDS int64 [n_add]; steps, first_lcc, final_lcc, seeds_in, added_in ints; label int64
    [len(seeds) + steps]; members int64 [len(seeds) + steps] (M in order).  on_step(members, L), when given, is called before every
    choice, the one that stops the growth included (not when n_add ends it)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    n = len(rowptr) - 1
    degree = np.diff(rowptr)
    src = np.repeat(np.arange(n), degree)
    seeds = [int(v) for v in seeds]
    m = len(seeds)
    pos = np.full(n, -1, np.int64)                       # position in M, -1 outside
    pos[seeds] = np.arange(m)
    comp = np.full(m + n_add, -1, np.int64)
    comp[:m] = _seed_components(rowptr, col, seeds, pos)
    members = list(seeds)
    out = {f: np.zeros(n_add, np.int64) for f in STEP_FIELDS + COUNT_FIELDS}
    out["node"][:] = -1
    L = int(np.bincount(comp[:m]).max()) if m else 0
    out["first_lcc"] = L
    t = 0
    while t < n_add:
        if on_step:
            on_step(np.array(members, np.int64), L)
        cur = m + t
        size = np.bincount(comp[:cur], minlength=max(cur, 1))
        hit = (pos[src] < 0) & (pos[col] >= 0)           # entries (v, c): v outside M, c inside
        if not hit.any():
            break
        pair = np.unique(src[hit] * (m + n_add) + comp[pos[col[hit]]])       # (candidate, component), each once
        v, r = pair // (m + n_add), pair % (m + n_add)
        cand, first = np.unique(v, return_index=True)
        tot = 1 + np.add.reduceat(size[r], first)
        merged = np.diff(np.append(first, len(v)))
        new = np.maximum(L, tot)
        order = np.lexsort((cand, degree[cand], -new))
        j = int(order[0])
        if new[j] - L < 2:
            break
        out["node"][t], out["lcc"][t], out["merged"][t], out["deg"][t] = cand[j], new[j], merged[j], degree[cand[j]]
        out["ties_lcc"][t] = int((new == new[j]).sum())
        out["ties_deg"][t] = int(((new == new[j]) & (degree[cand] == degree[cand[j]])).sum())
        out["candidates"][t], out["entries"][t], out["most_merged"][t] = len(cand), degree[cand].sum(), merged.max()
        roots = r[first[j]:first[j] + merged[j]]
        comp[:cur][np.isin(comp[:cur], roots)] = roots.min()
        comp[cur] = roots.min()
        pos[cand[j]] = cur
        members.append(int(cand[j]))
        L = int(new[j])
        t += 1
    label = comp[:m + t].copy()
    top = largest_root(label)
    inside = label == top if top is not None else np.zeros(0, bool)
    out.update(steps=t, final_lcc=L, seeds_in=int(inside[:m].sum()), added_in=int(inside[m:].sum()), label=label,
               members=np.array(members, np.int64))
    return out


def table(rowptr, col, units, n_add):
    """-> {"node", "lcc", "merged", "deg" and COUNT_FIELDS: int32 [U, n_add]; "steps", "first_lcc", "final_lcc", "seeds_in", "added_in": int32 [U];
    "label", "members": lists of int64 arrays}"""
    res = [grow(rowptr, col, u, n_add) for u in units]
    out = {f: np.stack([r[f] for r in res]).astype(np.int32).reshape(len(units), n_add) for f in STEP_FIELDS + COUNT_FIELDS}
    out.update({f: np.array([r[f] for r in res], np.int32) for f in UNIT_FIELDS})
    out["label"] = [r["label"] for r in res]
    out["members"] = [r["members"] for r in res]
    return out
