"""Gene knock-outs of diffusion profiles, in batch.

The question the multiscale interactome was built for -- which genes does a treatment run through? -- as the reference defines the
experiment: `msi.graph.remove_edges_from(in_edges(g) + out_edges(g))`, `weight_graph(weights)`, then DiffusionProfiles' arithmetic
(multiscale/diff_prof/diffusion_profiles.py:30-90) for the drug and for the indication, and the distance between the two profiles before
and after.  g stays in the node list as an isolated node, so N, the indices, the start vector 1 / N and the threshold N tol are those of the
whole graph.  The reference ships the gene lists for it (data/pharmgkb_df.tsv) and no code; on its CPU path a knock-out costs a graph rebuild
and two scipy power iterations.

Here a knock-out is one more column of the batched power iteration (csrc/ppr.hip): column (start s, gene g) differs from column (s, None)
in the rows of g's neighbours only, and those differences are index lists on the shared transition matrix M':

  weight_graph gives an edge w[class] / (the node's successors of that class), so without g a neighbour i of g keeps n_P - 1 protein-class
  successors, each now at w_P / (n_P - 1), and its other classes keep their weight; the row is renormalised by its new sum.  The host
  computes that row exactly (the sum in storage order, as scipy's M.sum(axis=1) adds it) and from it
    rho_P(i, c)  the factor of the row's protein-class entries relative to M'  -> an override x[i][c] *= rho_P (gss_ppr_desc.ovr_*);
    a correction (rho_O - rho_P) M'[i][j] x[i][c] for every other successor j  -> corr_* of gss_ppr_set_knockout, grouped by (column, j);
    a row that lost everything (g was its only successor), and g's own row: ratio 0 and listed in zero_*: what sits there is dangling;
  dead[c] = g: the shared matrix still delivers i -> g, so x[g][c] is forced to 0 after the product;
  the start node's "selected" row (sel_*) is rebuilt without g, start_dangling is set where g was its only protein, and the in-edges the
  start keeps (keep_*) take their new value.

KnockoutProblem wraps a PprProblem of the columns' distinct start nodes and rewrites its per-column lists; PprProblem itself is
unchanged.  What every column of a graph shares (the weighting, M', its row sums, the transpose) is a KnockoutGraph, built once."""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from . import msi as _msi
from .diffusion import PprProblem


class KnockoutError(ValueError):
    pass


def typed_edge_arrays(graph):
    """the typed graph as arrays, built once per graph: -> (names, src [E], dst [E], class id [E], class names), edges in adjacency order.
    An edge's class is its successor's type, except between two pathways, where the hierarchy table decides (MsiGraph._class_of): only
    those edges are looked up one by one"""
    names = graph.names
    idx = {n: i for i, n in enumerate(names)}
    deg = np.fromiter((len(s) for s in graph.adj.values()), np.int64, len(names))
    src = np.repeat(np.arange(len(names), dtype=np.int64), deg)
    dst = np.fromiter((idx[v] for succs in graph.adj.values() for v in succs), np.int64, int(deg.sum()))
    classes = sorted({graph.type[x] for x in names} | {_msi.UP, _msi.DOWN})
    class_id = {c: i for i, c in enumerate(classes)}
    type_id = np.asarray([class_id[graph.type[x]] for x in names], np.int64)
    cls = type_id[dst]
    fp = class_id.get(_msi.FUNCTIONAL_PATHWAY, -1)
    for e in np.flatnonzero((type_id[src] == fp) & (type_id[dst] == fp)):
        cls[e] = class_id[graph._class_of(names[src[e]], names[dst[e]])]
    return names, src, dst, cls, classes


def weight_edges(n, src, dst, cls, classes, weights, without=None):
    """MsiGraph.weight_graph + to_csr on the edge arrays: -> m0 CSR fp64 sorted.  `without`: a node index whose edges are dropped before
    the weighting (the knocked-out graph itself: what tools and tests compare against)"""
    if without is not None:
        live = (src != without) & (dst != without)
        src, dst, cls = src[live], dst[live], cls[live]
    w_of = np.zeros(len(classes))
    for i in np.unique(cls):
        w_of[i] = weights[classes[i]]
    count = np.zeros((n, len(classes)))
    np.add.at(count, (src, cls), 1.0)
    w = w_of[cls] / count[src, cls]                                   # msi.py:255-262: weights[class] / float(successors of that class)
    m0 = sp.csr_matrix((w, (src, dst)), shape=(n, n))
    m0.sort_indices()
    return m0


def weighted_csr(graph, weights, without=None):
    """MsiGraph.weight_graph + to_csr without touching the graph: -> (m0 CSR fp64 sorted, names, is_protein [N] bool).  `without`: a node
    name whose edges are dropped before the weighting"""
    names, src, dst, cls, classes = typed_edge_arrays(graph)
    m0 = weight_edges(len(names), src, dst, cls, classes, weights, None if without is None else names.index(without))
    return m0, names, np.asarray([graph.type[x] == _msi.PROTEIN for x in names], dtype=bool)


def row_sums_with(data, indptr, rows, replaced):
    """row sum in storage order with a set of entries replaced: `replaced` [entries of the listed rows, concatenated] holds the value
    every stored entry of rows `rows` takes (the generalisation of diffusion._row_sum_without to many rows and many entries).  Strictly
    left to right in fp64 through the csr_matvec loop that is behind scipy's M.sum(axis=1) itself (np.add.reduceat adds in another
    order): the entries become a CSR matrix of one column that multiplies [1.0]"""
    cnt = (indptr[rows + 1] - indptr[rows]).astype(np.int64)
    if not len(rows):
        return np.zeros(0)
    ptr = np.concatenate(([0], np.cumsum(cnt)))
    m = sp.csr_matrix((np.asarray(replaced, np.float64), np.zeros(int(ptr[-1]), np.int32), ptr), shape=(len(rows), 1))
    return np.asarray(m @ np.ones(1)).reshape(-1)


class KnockoutGraph:
    """what every column of a typed graph under one set of class weights shares, computed once: the weighted matrix m0, the shared matrix
    M' as PprProblem builds it (every drug / indication row in its "not selected" form, cut entries stored as 0.0) with its inverse row
    sums, the protein-class successor counts, and m0's transpose for the in-neighbours of a gene"""

    def __init__(self, msi_graph, weights):
        names, src, dst, cls, classes = typed_edge_arrays(msi_graph)
        self.graph = msi_graph
        self.names = names
        self.idx = idx = {x: i for i, x in enumerate(names)}
        self.n = n = len(names)
        self.w_p = float(weights[_msi.PROTEIN])
        self.m0 = m0 = weight_edges(n, src, dst, cls, classes, weights)
        self.is_protein = is_protein = np.asarray([msi_graph.type[x] == _msi.PROTEIN for x in names], dtype=bool)
        start_names = msi_graph.drugs_in_graph + msi_graph.indications_in_graph
        self.proteins_of = {idx[s]: sorted(idx[p] for p in msi_graph.drug_or_indication2proteins[s]) for s in start_names}
        self.indptr, self.indices = m0.indptr.astype(np.int64), m0.indices.astype(np.int64)
        indptr, indices = self.indptr, self.indices
        self.cut = cut = m0.data.copy()
        self.startlike = np.zeros(n, dtype=bool)
        self.prot_arr = {}
        for t, prots in self.proteins_of.items():
            lo, hi = indptr[t], indptr[t + 1]
            self.prot_arr[t] = np.asarray(prots, np.int64)
            cut[lo:hi][np.isin(indices[lo:hi], self.prot_arr[t])] = 0.0
            self.startlike[t] = True
        row_of = np.repeat(np.arange(n), np.diff(indptr))
        s_cut = np.asarray(sp.csr_matrix((cut, m0.indices, m0.indptr), shape=m0.shape).sum(axis=1)).flatten()
        s_cut[s_cut != 0] = 1.0 / s_cut[s_cut != 0]
        self.s_cut = s_cut
        self.entry_p = is_protein[indices]                             # class "protein" = the successor is a protein (msi.py:230-253)
        self.n_p = np.bincount(row_of[self.entry_p], minlength=n)
        self.m0t = m0.T.tocsr()
        self.m0t.sort_indices()
        self.base_of = {}                                              # PprProblem per set of distinct start nodes


class KnockoutProblem:
    """index lists of gss_ppr_create + gss_ppr_set_knockout for columns [(start node, gene or None)] of the typed graph (an MsiGraph, or
    a KnockoutGraph of it that several problems share).  Same attributes as PprProblem (PprEngine takes either), plus dead, corr_ptr,
    corr_grp_row, corr_grp_col, corr_src, corr_val."""

    def __init__(self, msi_graph, weights, columns):
        kg = msi_graph if isinstance(msi_graph, KnockoutGraph) else KnockoutGraph(msi_graph, weights)
        msi_graph, idx, is_protein, proteins_of = kg.graph, kg.idx, kg.is_protein, kg.proteins_of
        if not columns:
            raise KnockoutError("knockout: no columns")
        starts, genes = [], []
        for s, g in columns:
            if s not in idx:
                raise KnockoutError(f"knockout: start node {s!r} is not in the graph")
            if idx[s] not in proteins_of:
                raise KnockoutError(f"knockout: start node {s!r} is not a drug or an indication with proteins")
            if g is not None:
                if g not in idx:
                    raise KnockoutError(f"knockout: gene {g!r} is not in the graph")
                if g == s:
                    raise KnockoutError(f"knockout: gene {g!r} is the column's own start node")
                if not is_protein[idx[g]]:
                    raise KnockoutError(f"knockout: {g!r} is a {msi_graph.type[g]}, and only proteins can be knocked out")
            starts.append(idx[s]); genes.append(-1 if g is None else idx[g])
        self.columns = list(columns)
        self.names = kg.names
        self.m0 = kg.m0
        self.proteins_of = proteins_of
        # PprProblem's lists of a column depend on its start node alone: built once per distinct start (a screen has two), shared by
        # the chunks of one KnockoutGraph, and read below through `of`
        uniq, of = np.unique(np.asarray(starts, np.int64), return_inverse=True)
        base = kg.base_of.get(tuple(uniq.tolist()))
        if base is None:
            base = kg.base_of[tuple(uniq.tolist())] = PprProblem(kg.m0, uniq, proteins_of)
        self.base, self.base_column = base, of
        self.n, self.mt, self.z_rows = base.n, base.mt, base.z_rows
        self.k = len(starts)
        self.kpad = max(64, -(-self.k // 64) * 64)
        self.starts = np.asarray(starts, np.int32)
        self._rewrite(kg, np.asarray(starts, np.int64), np.asarray(genes, np.int64))
        key = self.ovr_col.astype(np.int64) * self.n + self.ovr_row       # the device scales x[row][column] in place, one thread per entry
        if len(np.unique(key)) != len(key):
            raise KnockoutError("knockout: two override entries for one (row, column)")

    def _rewrite(self, kg, starts, genes):
        base, n = self.base, self.n
        m0, is_protein, w_p = kg.m0, kg.is_protein, kg.w_p
        indptr, indices, cut, startlike, s_cut, entry_p, n_p, m0t = (kg.indptr, kg.indices, kg.cut, kg.startlike, kg.s_cut, kg.entry_p,
                                                                      kg.n_p, kg.m0t)
        k = self.k
        ovr_col, ovr_row, ovr_ratio, zero_ptr, zero_ovr = [], [], [], [0], []
        sel_col, sel_row, sel_val = [], [], []
        keep_ptr, keep_row, keep_val = [0], [], []
        grp_col, grp_row, grp_ptr, corr_src, corr_val = [], [], [0], [], []
        start_dangling = base.start_dangling[self.base_column].copy()
        sel_ptr = np.searchsorted(base.sel_col, np.arange(base.k + 1))
        n_ovr = 0
        for c in range(k):
            s, g, u = int(starts[c]), int(genes[c]), int(self.base_column[c])
            o_lo, o_hi = base.ovr_ptr[u], base.ovr_ptr[u + 1]
            b_row, b_ratio = base.ovr_row[o_lo:o_hi].astype(np.int64), base.ovr_ratio[o_lo:o_hi].copy()
            b_zero = np.zeros(len(b_row), dtype=bool)
            b_zero[base.zero_ovr[base.zero_ptr[u]:base.zero_ptr[u + 1]] - o_lo] = True
            k_lo, k_hi = base.keep_ptr[u], base.keep_ptr[u + 1]
            kr, kv = base.keep_row[k_lo:k_hi].astype(np.int64), base.keep_val[k_lo:k_hi].copy()
            s_lo, s_hi = sel_ptr[u], sel_ptr[u + 1]
            sr, sv = base.sel_row[s_lo:s_hi].astype(np.int64), base.sel_val[s_lo:s_hi]
            if g >= 0:
                nbr = m0t.indices[m0t.indptr[g]:m0t.indptr[g + 1]].astype(np.int64)       # rows with an edge into g
                # not g itself (a self-loop g -> g goes with g's edges: g's own row is the ratio-0 entry below)
                rows = nbr[(nbr != s) & (nbr != g) & ~startlike[nbr] & (s_cut[nbr] != 0)]
                # every stored entry of those rows, concatenated: position e in the matrix, its row's place r in `rows`
                cnt = indptr[rows + 1] - indptr[rows]
                first = np.concatenate(([0], np.cumsum(cnt)[:-1])).astype(np.int64) if len(rows) else np.zeros(0, np.int64)
                r = np.repeat(np.arange(len(rows)), cnt)
                e = np.arange(int(cnt.sum())) - first[r] + indptr[rows][r]
                dest, is_p = indices[e], entry_p[e]
                left = n_p[rows] - 1                                                       # protein-class successors without g
                new_p = np.where(left > 0, w_p / np.maximum(left, 1).astype(np.float64), 0.0)
                v = cut[e].copy()
                v[is_p] = new_p[r[is_p]]
                v[dest == g] = 0.0
                in_prots = np.isin(rows, kg.prot_arr[s])
                v[(dest == s) & in_prots[r]] = 0.0                                          # diffusion_profiles.py:33-36
                total = row_sums_with(cut, indptr, rows, v)
                inv = np.where(total != 0, 1.0 / np.where(total != 0, total, 1.0), 0.0)     # :52
                true = inv[r] * v                                                          # :53-54, the row of this column's matrix
                shared = s_cut[rows][r] * cut[e]
                rho_o = inv / s_cut[rows]
                rho_p = np.where(left > 0, (inv * new_p) / (s_cut[rows] * (w_p / n_p[rows].astype(np.float64))), rho_o)
                # corrections: the successors outside the protein class, where the two factors differ (not the start: keep_* carries it)
                fix = ~is_p & (v != 0) & (dest != s) & (left[r] > 0)
                cv = true[fix] - rho_p[r[fix]] * shared[fix]
                order = np.argsort(dest[fix], kind="stable")                               # groups by row j, entries in list order
                cj, cs_, cv = dest[fix][order], rows[r[fix]][order], cv[order]
                if len(cj):
                    new_grp = np.flatnonzero(np.concatenate(([True], cj[1:] != cj[:-1])))
                    grp_row.extend(cj[new_grp].tolist()); grp_col.extend([c] * len(new_grp))
                    grp_ptr.extend((len(corr_src) + np.append(new_grp[1:], len(cj))).tolist())
                    corr_src.extend(cs_.tolist()); corr_val.extend(cv.tolist())
                # in-edges the start keeps from such a row: yself reads the scaled x, so the value is taken relative to rho_P
                to_s = np.flatnonzero((dest == s) & (v != 0))
                for t in to_s:
                    hit = np.flatnonzero(kr == rows[r[t]])
                    kv[hit] = 0.0 if rho_p[r[t]] == 0 else true[t] / rho_p[r[t]]
                keep = kr != g
                kr, kv = kr[keep], kv[keep]
                # overrides: the rewritten rows replace the base's entries for them (the new factor contains the cut of the edge into s)
                gone = np.isin(b_row, rows) | (b_row == g)
                b_row, b_ratio, b_zero = b_row[~gone], b_ratio[~gone], b_zero[~gone]
                b_row = np.concatenate((b_row, rows)); b_ratio = np.concatenate((b_ratio, rho_p)); b_zero = np.concatenate((b_zero, inv == 0))
                if s_cut[g] != 0:                                                          # g's own row: isolated, so dangling
                    b_row = np.append(b_row, g); b_ratio = np.append(b_ratio, 0.0); b_zero = np.append(b_zero, True)
                # the start's "selected" row without g
                lo, hi = indptr[s], indptr[s + 1]
                if np.any(indices[lo:hi] == g):
                    left_s = n_p[s] - 1
                    vs = m0.data[lo:hi].copy()
                    vs[entry_p[lo:hi]] = w_p / float(left_s) if left_s > 0 else 0.0
                    vs[indices[lo:hi] == g] = 0.0
                    tot = float(np.cumsum(vs)[-1])
                    if tot != 0:
                        live = (vs != 0) & (indices[lo:hi] != s)
                        sr, sv = indices[lo:hi][live], (1.0 / tot) * vs[live]
                    else:
                        sr, sv = np.zeros(0, np.int64), np.zeros(0)
                        start_dangling[c] = 1
            ovr_col.extend([c] * len(b_row)); ovr_row.extend(b_row.tolist()); ovr_ratio.extend(b_ratio.tolist())
            zero_ovr.extend((n_ovr + np.flatnonzero(b_zero)).tolist())
            zero_ptr.append(len(zero_ovr))
            n_ovr += len(b_row)
            sel_col.extend([c] * len(sr)); sel_row.extend(sr.tolist()); sel_val.extend(np.asarray(sv).tolist())
            keep_row.extend(kr.tolist()); keep_val.extend(kv.tolist())
            keep_ptr.append(len(keep_row))
        self.start_dangling = start_dangling
        self.ovr_col = np.asarray(ovr_col, np.int32); self.ovr_row = np.asarray(ovr_row, np.int32)
        self.ovr_ratio = np.asarray(ovr_ratio, np.float64)
        self.zero_ptr = np.asarray(zero_ptr, np.int32); self.zero_ovr = np.asarray(zero_ovr, np.int32)
        self.ovr_ptr = np.searchsorted(self.ovr_col, np.arange(k + 1)).astype(np.int32)
        self.sel_col = np.asarray(sel_col, np.int32); self.sel_row = np.asarray(sel_row, np.int32)
        self.sel_val = np.asarray(sel_val, np.float64)
        self.keep_ptr = np.asarray(keep_ptr, np.int32); self.keep_row = np.asarray(keep_row, np.int32)
        self.keep_val = np.asarray(keep_val, np.float64)
        self.dead = genes.astype(np.int32)
        self.corr_ptr = np.asarray(grp_ptr, np.int32)
        self.corr_grp_row = np.asarray(grp_row, np.int32); self.corr_grp_col = np.asarray(grp_col, np.int32)
        self.corr_src = np.asarray(corr_src, np.int32); self.corr_val = np.asarray(corr_val, np.float64)


def _engine(prob, device="cuda"):
    """PprEngine of a KnockoutProblem with its knock-out lists set on the handle (gss_ppr_set_knockout)"""
    import torch
    from . import _lib
    from .diffusion import PprEngine
    eng = PprEngine(prob, device)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.x.device)  # noqa: E731
    ko = dict(dead=t(prob.dead), corr_ptr=t(prob.corr_ptr), corr_grp_row=t(prob.corr_grp_row), corr_grp_col=t(prob.corr_grp_col),
              corr_src=t(prob.corr_src), corr_val=t(prob.corr_val))
    eng.bufs.update(ko)                                  # the handle keeps the pointers: the tensors live as long as the engine
    n_grp, n_corr = len(prob.corr_grp_row), len(prob.corr_src)
    p = lambda b: b.data_ptr() if b.numel() else None  # noqa: E731
    _lib.check(eng.lib.gss_ppr_set_knockout(eng.handle, ko["dead"].data_ptr(), n_grp, p(ko["corr_ptr"]) if n_grp else None,
                                            p(ko["corr_grp_row"]), p(ko["corr_grp_col"]), n_corr, p(ko["corr_src"]), p(ko["corr_val"])),
               "gss_ppr_set_knockout")
    return eng


def knockout_profiles(msi_graph, weights, columns, alpha, max_iter, tol, device="cuda", max_columns=4096):
    """profiles of the columns [(start, gene or None)] -> (profiles [K][N] fp64, iterations [K]); chunks of at most max_columns columns,
    as diffusion.diffusion_profiles"""
    columns = list(columns)
    n = len(msi_graph.adj)
    out = np.empty((len(columns), n), dtype=np.float64)
    its = np.empty(len(columns), dtype=np.int32)
    kg = KnockoutGraph(msi_graph, weights)                 # the weighting and the shared matrix: once, not per chunk
    for lo in range(0, len(columns), max_columns):
        sub = columns[lo:lo + max_columns]
        eng = _engine(KnockoutProblem(kg, weights, sub), device)
        x, it = eng.run(alpha, tol, max_iter)
        out[lo:lo + len(sub)] = x[:, :len(sub)].t().contiguous().cpu().numpy()
        its[lo:lo + len(sub)] = it
        del eng
    return out, its


# ---- the experiment: distances before and after ----------------------------------------------------------------------------------------------

HEADER = ["drug", "indication", "gene", "gene name", "dist_before", "dist_after", "delta", "shift_drug", "shift_indication",
          "iterations_drug", "iterations_indication"]


def plan_chunks(triples, max_columns=4096):
    """(drug, indication, gene) triples -> chunks [(columns [(start, gene or None)], pairs [(column a, column b)], rows)], every chunk of
    at most max_columns columns.  A (start, gene) column is computed once per chunk, and a triple's baseline columns (start, None) are in
    its chunk.  A triple's two knocked-out columns are laid out side by side; in a screen of one drug-indication pair they start at an even
    column, and the paired-distance kernel then reads them with one 16-byte load (elsewhere with two of 8 bytes: no column is spent on
    padding).  rows: per triple the positions of its four distances in the chunk's pair list."""
    if max_columns < 4:
        raise KnockoutError(f"knockout: max_columns={max_columns} leaves no room for two baselines and two knock-outs")
    chunks = []
    cols, where, pairs, pair_at, rows = [], {}, [], {}, []

    def flush():
        nonlocal cols, where, pairs, pair_at, rows
        if rows:
            chunks.append((cols, pairs, rows))
        cols, where, pairs, pair_at, rows = [], {}, [], {}, []

    def column(key):
        if key not in where:
            where[key] = len(cols)
            cols.append(key)
        return where[key]

    def pair(a, b):
        if (a, b) not in pair_at:
            pair_at[(a, b)] = len(pairs)
            pairs.append((a, b))
        return pair_at[(a, b)]

    for d, i, g in triples:
        if len(cols) + 4 > max_columns:                               # at most four new columns
            flush()
        bd, bi = column((d, None)), column((i, None))
        kd, ki = column((d, g)), column((i, g))
        rows.append((d, i, g, pair(bd, bi), pair(kd, ki), pair(bd, kd), pair(bi, ki), kd, ki))
    flush()
    return chunks


def knockout_distances(msi_graph, triples, metric, weights, alpha, max_iter, tol, device="cuda", max_columns=4096):
    """-> one record (dict with HEADER's keys) per (drug, indication, gene) triple, in the order given.  Per chunk: one batched power
    iteration for all its columns, one gss_profile_dist_pairs launch for all its distances."""
    from .diffusion import check_metric, compare_profile_pairs
    check_metric(metric)
    out = []
    kg = KnockoutGraph(msi_graph, weights)                 # the weighting and the shared matrix: once, not per chunk
    for cols, pairs, rows in plan_chunks(list(triples), max_columns):
        eng = _engine(KnockoutProblem(kg, weights, cols), device)
        x, its = eng.run(alpha, tol, max_iter)
        dist = compare_profile_pairs(x, [a for a, _ in pairs], [b for _, b in pairs], metric, device).cpu().numpy()
        for d, i, g, before, after, sd, si, kd, ki in rows:
            out.append({"drug": d, "indication": i, "gene": g, "gene name": msi_graph.node2name.get(g),
                        "dist_before": float(dist[before]), "dist_after": float(dist[after]), "delta": float(dist[after] - dist[before]),
                        "shift_drug": float(dist[sd]), "shift_indication": float(dist[si]),
                        "iterations_drug": int(its[kd]), "iterations_indication": int(its[ki])})
        del eng
    return out


def knockout_screen(msi_graph, drug, indication, genes, metric, weights=None, alpha=None, max_iter=None, tol=None, device="cuda",
                    max_columns=4096):
    """every gene of `genes` knocked out of one drug-indication pair -> records sorted by |delta| descending, ties by gene id.  The
    weights, alpha, max_iter and tol default to the diffusion method's (predict.DIFFUSION)."""
    from .predict import DIFFUSION
    genes = list(dict.fromkeys(genes))
    rec = knockout_distances(msi_graph, [(drug, indication, g) for g in genes], metric, DIFFUSION["weights"] if weights is None else weights,
                             DIFFUSION["alpha"] if alpha is None else alpha, DIFFUSION["max_iter"] if max_iter is None else max_iter,
                             DIFFUSION["tol"] if tol is None else tol, device, max_columns)
    return sorted(rec, key=lambda r: (-abs(r["delta"]) if r["delta"] == r["delta"] else 1.0, r["gene"]))


def write_records(path, records):
    from .predict import write_tsv
    write_tsv(path, HEADER, [[r[h] for h in HEADER] for r in records])


# ---- knockout.py ---------------------------------------------------------------------------------------------------------------------------

def read_triples(path):
    """a tab-separated table with the columns drug, indication, gene (data/pharmgkb_df.tsv) -> [(drug, indication, gene)] in row order"""
    import csv
    with open(path, newline="") as f:
        rows = csv.reader(f, delimiter="\t")
        header = next(rows, None)
        if header is None or any(c not in header for c in ("drug", "indication", "gene")):
            raise KnockoutError(f"--triples {path!r}: the table needs the columns drug, indication and gene")
        at = [header.index(c) for c in ("drug", "indication", "gene")]
        return [tuple(r[a] for a in at) for r in rows if len(r) > max(at)]


def usable_triples(msi_graph, triples, err):
    """the triples the graph can answer, each once, in order; the others are counted on `err` by reason"""
    starts = set(msi_graph.drugs_in_graph + msi_graph.indications_in_graph)
    skipped = {}
    keep = []
    for d, i, g in dict.fromkeys(triples):
        if d not in starts or msi_graph.type.get(d) != _msi.DRUG:
            why = "drug not in the graph"
        elif i not in starts or msi_graph.type.get(i) != _msi.INDICATION:
            why = "indication not in the graph"
        elif msi_graph.type.get(g) != _msi.PROTEIN:
            why = "gene not in the graph"
        else:
            keep.append((d, i, g))
            continue
        skipped[why] = skipped.get(why, 0) + 1
    for why in sorted(skipped):
        print(f"knockout: skipped {skipped[why]} triples: {why}", file=err)
    return keep


def parse_args(argv=None):
    import argparse
    from .diffusion import ALL_METRICS as METRICS
    p = argparse.ArgumentParser(description="Drug Repurposing: knock genes out of the diffusion profiles of a drug and an indication (knockout.py)")
    p.add_argument("-c", "--config", default="config.json", type=str, help="config file path (default: config.json), as evaluate_auc.py reads it")
    p.add_argument("--triples", default=None, type=str, help="a TSV with the columns drug, indication, gene (data/pharmgkb_df.tsv): one row out per triple")
    p.add_argument("--drug", default=None, type=str, help="screen mode: the drug id")
    p.add_argument("--indication", default=None, type=str, help="screen mode: the indication id")
    p.add_argument("--genes", default=None, type=str, help="screen mode: a file with one protein id per line")
    p.add_argument("--all-proteins", action="store_true", help="screen mode: every protein of the graph")
    p.add_argument("--top", default=None, type=int, help="screen mode: keep the K genes with the largest |delta|")
    p.add_argument("--metric", default="correlation", type=str, help="distance between two profiles: " + ", ".join(METRICS) + " (default: correlation)")
    p.add_argument("--out", default="knockouts.tsv", type=str, help="the table (default: knockouts.tsv)")
    return p.parse_args(argv)


def run(cfg_path, triples=None, drug=None, indication=None, genes=None, all_proteins=False, top=None, metric="correlation",
        out="knockouts.tsv", err=None, device="cuda"):
    """the command -> the records written"""
    import sys
    from . import evaluate
    from .diffusion import check_metric
    from .predict import DIFFUSION, PredictError
    err = sys.stderr if err is None else err
    try:
        check_metric(metric)
    except ValueError as e:
        raise KnockoutError(f"--metric: {e}") from None
    screen = drug is not None or indication is not None or genes is not None or all_proteins
    if (triples is None) == (not screen):
        raise KnockoutError("give either --triples, or --drug and --indication with --genes or --all-proteins")
    if screen and (drug is None or indication is None or (genes is None) == (not all_proteins)):
        raise KnockoutError("screen mode needs --drug, --indication and one of --genes / --all-proteins")
    if top is not None and (not screen or top < 1):
        raise KnockoutError("--top K needs the screen mode and K >= 1")
    try:
        s = evaluate.Settings(evaluate.load_config(cfg_path))
    except PredictError as e:
        raise KnockoutError(str(e)) from None
    g = _msi.MsiGraph().load(s.tables())
    par = (DIFFUSION["weights"], DIFFUSION["alpha"], DIFFUSION["max_iter"], DIFFUSION["tol"])
    if screen:
        if all_proteins:
            gene_list = [n for n in g.names if g.type[n] == _msi.PROTEIN]
        else:
            with open(genes) as f:
                gene_list = [line.strip() for line in f if line.strip()]
        rec = knockout_screen(g, drug, indication, gene_list, metric, device=device)
        rec = rec[:top] if top is not None else rec
    else:
        rec = knockout_distances(g, usable_triples(g, read_triples(triples), err), metric, *par, device=device)
    write_records(out, rec)
    return rec


def main(argv=None):
    import json
    import sys
    a = parse_args(argv)
    try:
        rec = run(a.config, a.triples, a.drug, a.indication, a.genes, a.all_proteins, a.top, a.metric, a.out)
    except (KnockoutError, OSError, json.JSONDecodeError) as e:
        print(f"knockout: {e}", file=sys.stderr)
        sys.exit(2)
    print(f"{a.metric}: {len(rec)} knock-outs: {a.out}")
