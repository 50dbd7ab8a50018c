"""Diffusion profiles (the reference's 'diffusion' comparator) on the device SpMM -- SURVEY.md section 8-f4.

Mirror of multiscale/diff_prof/diffusion_profiles.py: class DiffusionProfiles with the reference's constructor, file
naming (:92-98: '<clean name>_p_visit_array.npy', np.save of the fp64 vector) and loader (:158-171), so
evaluate_auc.py:97-111,156-161 / predict_drug.py:98-113 read the result unchanged.  The reference runs one scipy power
iteration per drug / indication in a process pool (:125-156); here all start nodes are columns of one fp64 matrix and an
iteration is one batched SpMM through libgssgcn.so (gss_ppr_*, csrc/ppr.hip).  No CPU fallback.

Host side (this file): what the reference also does on the host with scipy -- the weighted adjacency, its row sums
(:49-56) and, per start node, which rows of x need special treatment (:30-47) -- as index lists, not as a matrix copy
per start node.

compare_profiles: the comparison of two profiles the method rests on (multiscale/README.md, overview (c)), which the reference never makes: a
pairwise distance between columns of the profile matrix (gss_profile_dist, csrc/profile_dist.hip), on the tensor PprEngine.run returned or on
profiles loaded from a directory.  rank_profiles: the average-tie ranks of the nodes within each profile (gss_profile_rank,
csrc/profile_rank.hip); the "spearman" distance is the correlation distance of those ranks.  top_nodes: the k highest nodes of each
profile per node group -- the proteins and the biological functions a treatment runs through -- and top_overlap: how many of them two
profiles share (gss_profile_topk, gss_topk_overlap, csrc/profile_topk.hip)."""
from __future__ import annotations

import ctypes as C
import os
import pickle

import numpy as np
import scipy.sparse as sp

from . import _lib


def _row_sum_without(data: np.ndarray, skip: int) -> float:
    """row sum in storage order with one entry replaced by 0.0 (what scipy's M.sum(axis=1) gives after M[p, s] = 0):
    np.cumsum adds left to right in fp64, like the csr_matvec loop behind that sum"""
    row = data.copy()
    row[skip] = 0.0
    return float(np.cumsum(row)[-1])


class PprProblem:
    """index lists for gss_ppr_create from (raw weighted adjacency, start nodes, {drug/indication: its proteins})"""

    def __init__(self, m0: sp.csr_matrix, starts, proteins_of: dict):
        m0 = sp.csr_matrix(m0, dtype=np.float64)
        m0.sort_indices()
        n = m0.shape[0]
        starts = np.asarray(starts, dtype=np.int64)
        indptr, indices, data = m0.indptr, m0.indices, m0.data
        rowsum = np.asarray(m0.sum(axis=1)).flatten()                 # diffusion_profiles.py:51 for an untouched row
        # the shared matrix: every drug / indication row in its "not selected" form -- edges to its proteins cut (:38-46)
        cut = m0.copy()
        for t, prots in proteins_of.items():
            lo, hi = indptr[t], indptr[t + 1]
            hit = np.isin(indices[lo:hi], np.fromiter((int(p) for p in prots), dtype=np.int64, count=len(prots)))
            cut.data[lo:hi][hit] = 0.0
        cut_sum = np.asarray(cut.sum(axis=1)).flatten()               # :51 (the cut entries stay stored as 0.0, as in the reference)
        s_cut = cut_sum.copy()
        s_cut[s_cut != 0] = 1.0 / s_cut[s_cut != 0]                   # :52
        mprime = (sp.diags(s_cut, 0, format="csr") @ cut).tocsr()      # :53-54
        mprime.eliminate_zeros()
        mt = mprime.T.tocsr()
        mt.sort_indices()
        ovr_col, ovr_row, ovr_ratio, zero_ptr, zero_ovr = [], [], [], [0], []
        sel_col, sel_row, sel_val = [], [], []
        keep_ptr, keep_row, keep_val = [0], [], []
        mpc = mprime.tocsc()
        start_dangling = np.zeros(len(starts), dtype=np.int32)
        for c, s in enumerate(starts):
            s = int(s)
            prots = set(int(p) for p in proteins_of[s])
            for p in sorted(prots):                                   # :33-36: M[p, s] = 0, then row p renormalised
                lo, hi = indptr[p], indptr[p + 1]
                j = lo + np.searchsorted(indices[lo:hi], s)
                if j >= hi or indices[j] != s or s_cut[p] == 0:
                    continue
                new = _row_sum_without(cut.data[lo:hi], j - lo)
                ratio = 0.0 if new == 0 else (1.0 / new) / s_cut[p]
                if ratio == 0.0:
                    zero_ovr.append(len(ovr_col))
                ovr_col.append(c); ovr_row.append(p); ovr_ratio.append(ratio)
            zero_ptr.append(len(zero_ovr))
            # the start node's own row is whole in M_s: its "not selected" form must not act in this column ...
            if s_cut[s] != 0:
                ovr_col.append(c); ovr_row.append(s); ovr_ratio.append(0.0)
            # ... and its "selected" form (all out-edges over their sum) does
            if rowsum[s] != 0:
                inv = 1.0 / rowsum[s]
                for j, w in zip(indices[indptr[s]:indptr[s + 1]], data[indptr[s]:indptr[s + 1]]):
                    if w != 0 and int(j) != s:
                        sel_col.append(c); sel_row.append(int(j)); sel_val.append(float(inv * w))
            else:
                start_dangling[c] = 1
            lo, hi = mpc.indptr[s], mpc.indptr[s + 1]                 # in-edges of s that are not cut
            for i, w in zip(mpc.indices[lo:hi], mpc.data[lo:hi]):
                if int(i) not in prots and int(i) != s:
                    keep_row.append(int(i)); keep_val.append(float(w))
            if rowsum[s] != 0 and m0[s, s] != 0:                      # a self loop of the start node
                keep_row.append(s); keep_val.append(float(m0[s, s] / rowsum[s]))
            keep_ptr.append(len(keep_row))
        self.n, self.k = n, len(starts)
        self.kpad = max(64, -(-self.k // 64) * 64)
        self.mt = mt
        self.starts = starts.astype(np.int32)
        self.start_dangling = start_dangling
        self.z_rows = np.flatnonzero(s_cut == 0).astype(np.int32)     # :77 is_dangling, for rows no start node changes
        self.ovr_col = np.asarray(ovr_col, np.int32); self.ovr_row = np.asarray(ovr_row, np.int32)
        self.ovr_ratio = np.asarray(ovr_ratio, np.float64)
        self.zero_ptr = np.asarray(zero_ptr, np.int32); self.zero_ovr = np.asarray(zero_ovr, np.int32)
        # the overrides were appended column by column: entries [ovr_ptr[c], ovr_ptr[c + 1]) belong to column c (gss_ppr_desc.ovr_ptr)
        assert np.all(np.diff(self.ovr_col) >= 0)
        self.ovr_ptr = np.searchsorted(self.ovr_col, np.arange(self.k + 1)).astype(np.int32)
        self.sel_col = np.asarray(sel_col, np.int32); self.sel_row = np.asarray(sel_row, np.int32)
        self.sel_val = np.asarray(sel_val, np.float64)
        self.keep_ptr = np.asarray(keep_ptr, np.int32); self.keep_row = np.asarray(keep_row, np.int32)
        self.keep_val = np.asarray(keep_val, np.float64)


class PprEngine:
    """device handle (gss_ppr) for one PprProblem"""

    def __init__(self, prob: PprProblem, device="cuda"):
        import torch
        self.lib = _lib.load()
        self.prob = prob
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.GssError("diffusion profiles run on the GPU only (no CPU fallback)")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        mt = prob.mt
        self.h_rowptr = np.ascontiguousarray(mt.indptr.astype(np.int32))
        self.bufs = dict(t_rowptr=t(self.h_rowptr), t_col=t(mt.indices.astype(np.int32)), t_val=t(mt.data.astype(np.float64)),
                         start=t(prob.starts), start_dangling=t(prob.start_dangling), z_rows=t(prob.z_rows),
                         ovr_col=t(prob.ovr_col), ovr_row=t(prob.ovr_row), ovr_ratio=t(prob.ovr_ratio), zero_ptr=t(prob.zero_ptr),
                         zero_ovr=t(prob.zero_ovr), sel_col=t(prob.sel_col), sel_row=t(prob.sel_row), sel_val=t(prob.sel_val),
                         keep_ptr=t(prob.keep_ptr), keep_row=t(prob.keep_row), keep_val=t(prob.keep_val), ovr_ptr=t(prob.ovr_ptr))
        d = _lib.PprDesc()
        d.n, d.k, d.kpad, d.nnz = prob.n, prob.k, prob.kpad, int(mt.nnz)
        d.h_rowptr = self.h_rowptr.ctypes.data
        d.n_z, d.n_ovr, d.n_sel = len(prob.z_rows), len(prob.ovr_col), len(prob.sel_col)
        for name, buf in self.bufs.items():
            setattr(d, name, buf.data_ptr() if buf.numel() else None)
        self.handle = C.c_void_p()
        _lib.check(self.lib.gss_ppr_create(C.byref(self.handle), C.byref(d)), "gss_ppr_create")
        self.x = torch.empty(prob.n, prob.kpad, dtype=torch.float64, device=dev)

    def run(self, alpha: float, tol: float, max_iter: int):
        """-> (x device tensor [n][kpad] (column c = start node c), iterations [k])"""
        iters = np.zeros(self.prob.k, dtype=np.int32)
        rc = self.lib.gss_ppr_run(self.handle, float(alpha), float(tol), int(max_iter), self.x.data_ptr(), iters.ctypes.data,
                                  _lib.current_stream())
        if rc == -34:  # GSS_ENOTCONV; the reference raises here (diffusion_profiles.py:90)
            raise RuntimeError("power iteration failed to converge in %d iterations" % max_iter)
        _lib.check(rc, "gss_ppr_run")
        return self.x, iters

    def spmm(self, x, y):
        _lib.check(self.lib.gss_ppr_spmm(self.handle, x.data_ptr(), y.data_ptr(), _lib.current_stream()), "gss_ppr_spmm")

    def check_guards(self):
        """raises if a kernel wrote behind one of the handle's buffers (gss_ppr_check_guards; tests call it)"""
        _lib.check(self.lib.gss_ppr_check_guards(self.handle), "gss_ppr_check_guards")

    def device_bytes(self) -> int:
        return int(self.lib.gss_ppr_device_bytes(self.handle))

    def __del__(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.gss_ppr_destroy(self.handle)
            self.handle = C.c_void_p()


METRICS = ("cityblock", "euclidean", "canberra", "cosine", "correlation")   # index = GSS_DIST_* of include/gssgcn.h


RANK_METRICS = ("spearman",)   # the metric of the same position in RANK_BASE on the average-tie ranks of the profiles (gss_profile_rank); no C id
RANK_BASE = ("correlation",)
ALL_METRICS = METRICS + RANK_METRICS


def check_metric(metric):
    """-> the GSS_DIST_* id the distance kernels take: the metric's own, or for a rank metric that of the metric applied to the ranks"""
    if metric not in ALL_METRICS:
        raise ValueError(f"profile distance {metric!r} is unknown; choose one of {', '.join(ALL_METRICS)}")
    return METRICS.index(RANK_BASE[RANK_METRICS.index(metric)] if metric in RANK_METRICS else metric)


def _column_list(what, sel, width, names=None, who="compare_profiles"):
    """-> int32 column indices of a selection: integers (None = every column), or keys of `names` ({key: column})"""
    if sel is None:
        return np.arange(width, dtype=np.int32)
    if names is not None:
        missing = [k for k in sel if k not in names]
        if missing:
            raise ValueError(f"{who}: {what} {missing[0]!r} has no profile")
        return np.asarray([names[k] for k in sel], dtype=np.int32)
    idx = np.asarray(sel, dtype=np.int64).reshape(-1)
    bad = np.flatnonzero((idx < 0) | (idx >= width))
    if len(bad):
        raise ValueError(f"{who}: {what} index {int(idx[bad[0]])} is outside [0, {width})")
    return idx.astype(np.int32)


def _device_list(cols, dev):
    """a host column list -> what a kernel takes for it: None when it is 0, 1, ... len - 1 ("the first columns" needs no list, and no check
    of one), else a device int32 tensor"""
    import torch
    return None if np.array_equal(cols, np.arange(len(cols))) else torch.from_numpy(np.ascontiguousarray(cols, dtype=np.int32)).to(dev)


def _workspace(need, dev):
    """a device workspace of at least `need` bytes, 8-byte aligned"""
    import torch
    return torch.empty((need + 7) // 8, dtype=torch.float64, device=dev)


def _rank_columns(x, cols):
    """average-tie ranks of the listed columns (host int32 array) of the device fp64 matrix x [N][width] -> device fp64 [N][len(cols)]
    (gss_profile_rank, csrc/profile_rank.hip; exact, a column with a NaN comes out NaN)"""
    import torch
    n, nc = x.shape[0], len(cols)
    r = torch.empty(n, nc, dtype=torch.float64, device=x.device)
    if nc == 0:
        return r
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.gss_profile_rank_workspace_bytes(n, nc))
        ws, lst = _workspace(need, x.device), _device_list(cols, x.device)
        _lib.check(lib.gss_profile_rank(n, x.data_ptr(), _lib.row_stride(x), nc, _lib.ptr(lst), r.data_ptr(), nc, ws.data_ptr(), need,
                                        _lib.current_stream()), "gss_profile_rank")
    return r


def _rank_referenced(x, lists):
    """a rank metric's first step: the unique columns the lists name are ranked once -> (rank matrix [N][unique], the lists remapped into it)"""
    uniq = np.unique(np.concatenate(lists)).astype(np.int32)
    return _rank_columns(x, uniq), [np.searchsorted(uniq, c).astype(np.int32) for c in lists]


_SEL_ARG = {"row": "rows", "column": "cols"}   # a selection's word in a message -> the argument it came in (col_a and col_b are both)


def _profile_source(profiles, sels, labels, who, required=None, lists_who=None):
    """The one place that knows the three kinds of `profiles`: the device tensor x [N][kpad] (used in place; a selection lists column
    indices), a host array [K][N] (a selection lists its rows) and a {name: vector} dict (a selection lists names).  sels: one or two
    selections, labels: their words in a message ("column"; "row", "column"; "col_a", "col_b") -> (N, [one int32 column list per
    selection], upload), where upload(dev) gives the device fp64 matrix [N][width] with unit column stride that the lists index.  The
    selections of a dict share one key table, in the order of first appearance: every named profile is uploaded once.  A selection that
    is None means every profile, which a dict cannot offer; with `required` it is refused in those words for every kind.  Refusals come
    in the order source, selections; those of a list's entries carry lists_who (who unless given).  Nothing here touches the GPU."""
    import torch
    absent = any(sel is None for sel in sels)
    if isinstance(profiles, dict):
        if absent:
            raise ValueError(f"{who}: {required or ' and '.join(_SEL_ARG.get(l, l) for l in labels) + ' must name the profiles of a dict'}")
        keys = list(dict.fromkeys(k for sel in sels for k in sel))
        names = {k: i for i, k in enumerate(keys) if k in profiles}
        lists = [_column_list(l, sel, len(keys), names, who=lists_who or who) for l, sel in zip(labels, sels)]
        host = [np.asarray(profiles[k], dtype=np.float64).reshape(-1) for k in keys]
        if len({len(v) for v in host}) > 1:
            raise ValueError(f"{who}: the profiles differ in length")
        if not host and len(sels) == 1:   # two empty selections are an empty result, one empty selection is a mistake
            raise ValueError(f"{who}: no profile is named")
        return len(host[0]) if host else 0, lists, lambda dev: torch.from_numpy(np.stack(host)).to(dev).t().contiguous()
    if isinstance(profiles, torch.Tensor):
        x = profiles
        if (x.dim() != 2 or x.dtype != torch.float64 or not x.is_cuda or x.shape[1] < 1 or (x.shape[1] > 1 and x.stride(1) != 1)
                or (x.shape[0] > 1 and x.stride(0) < x.shape[1])):
            raise ValueError(f"{who}: a profile tensor must be a device fp64 matrix [N][columns] with unit column stride and "
                             "a row stride of at least its width")
        n, width, upload = x.shape[0], x.shape[1], lambda dev: x
    else:
        host = np.ascontiguousarray(profiles, dtype=np.float64)
        if host.ndim != 2:
            raise ValueError(f"{who}: a host profile array must be [K][N], not {host.shape}")
        n, width, upload = host.shape[1], host.shape[0], lambda dev: torch.from_numpy(host).to(dev).t().contiguous()
    if absent and required:
        raise ValueError(f"{who}: {required}")
    return n, [_column_list(l, sel, width, who=lists_who or who) for l, sel in zip(labels, sels)], upload


def rank_profiles(profiles, cols=None, device="cuda"):
    """average-tie ranks of the nodes within diffusion profiles -> device tensor fp64 [N][len(cols)], column j =
    scipy.stats.rankdata(profile cols[j], method="average"), exactly (gss_profile_rank): the order of a profile's nodes, "the proteins and
    functions a profile ranks highest", and the transform behind the "spearman" distance.  `profiles` is what compare_profiles accepts: the
    device tensor x [N][kpad] (used in place; cols are column indices), a host array [K][N] (cols index its rows) or a {name: vector} dict
    (cols are names).  cols may repeat and come in any order; None means every profile (not for a dict).  A profile that holds a NaN has
    NaN for every rank.  A host array or dict is uploaded only after every refusal the host can make.  No CPU fallback."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError("profile ranks are computed on the GPU only (no CPU fallback)")
    n, (c,), upload = _profile_source(profiles, (cols,), ("column",), "rank_profiles")
    if n < 1:
        raise ValueError("rank_profiles: the profiles are empty")
    return _rank_columns(upload(dev), c)


MAX_TOP, MAX_GROUPS = 1024, 8   # gss_profile_topk's limits on k and G


def top_nodes(profiles, cols=None, k=20, groups=None, n_groups=None, device="cuda"):
    """the k highest nodes of diffusion profiles, per node group -> device tensors (idx int32 [len(cols)][G][k], val fp64 [len(cols)][G][k],
    cnt int32 [len(cols)][G]): for profile cols[j] and group g, idx[j][g][:cnt[j][g]] are the group's nodes in the order of
    np.argsort(-profile[members], kind="stable")[:k] -- descending value, ties by the smaller node index, exactly -- and val their values;
    the slots from cnt on hold -1 and NaN, and a profile with a NaN among the group's nodes has cnt = -1 and nothing listed
    (gss_profile_topk).  `profiles` is what rank_profiles accepts: the device tensor x [N][kpad] (used in place; cols are column indices), a
    host array [K][N] (cols index its rows) or a {name: vector} dict (cols are names); cols may repeat and come in any order, None means
    every profile (not for a dict).  `groups`: a host or device integer array [N] with each node's group in [-1, G), -1 = never listed
    (msi.py's node types, for "the proteins and the biological functions"); None = one group of all nodes.  G = n_groups, or the highest
    group + 1.  k <= 1024, G <= 8.  No CPU fallback."""
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError("the top nodes of a profile are selected on the GPU only (no CPU fallback)")
    if not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_TOP:
        raise ValueError(f"top_nodes: k={k!r} is outside [1, {MAX_TOP}]")
    n, (c,), upload = _profile_source(profiles, (cols,), ("column",), "top_nodes")
    if n < 1:
        raise ValueError("top_nodes: the profiles are empty")
    grp = None
    if groups is None:
        G = 1 if n_groups is None else int(n_groups)
        if G != 1:
            raise ValueError(f"top_nodes: n_groups={n_groups!r} needs a groups array (without one every node is in group 0)")
    else:
        on_device = isinstance(groups, torch.Tensor) and groups.is_cuda
        grp = groups if isinstance(groups, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(groups))
        if grp.dim() != 1 or grp.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
            raise ValueError(f"top_nodes: groups must be an integer array [N], not {tuple(grp.shape)} of {grp.dtype}")
        if grp.shape[0] != n:
            raise ValueError(f"top_nodes: groups has {grp.shape[0]} entries, the profiles {n} nodes")
        if n_groups is not None:
            G = int(n_groups)
        elif on_device:
            G = max(1, int(grp.max()) + 1)
        else:
            G = max(1, int(grp.numpy().max()) + 1)
        if not 1 <= G <= MAX_GROUPS:
            raise ValueError(f"top_nodes: G={G} groups is outside [1, {MAX_GROUPS}]")
        bad = torch.nonzero((grp < -1) | (grp >= G))
        if bad.numel():
            at = int(bad[0])
            raise ValueError(f"top_nodes: groups[{at}] = {int(grp[at])} is outside [-1, G={G})")
    nc = len(c)
    x = upload(dev)
    idx = torch.empty(nc, G, k, dtype=torch.int32, device=x.device)
    val = torch.empty(nc, G, k, dtype=torch.float64, device=x.device)
    cnt = torch.empty(nc, G, dtype=torch.int32, device=x.device)
    if nc == 0:
        return idx, val, cnt
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.gss_profile_topk_workspace_bytes(n, nc, G, int(k)))
        ws, lst = _workspace(need, x.device), _device_list(c, x.device)
        d_grp = None if grp is None else grp.to(device=x.device, dtype=torch.int32).contiguous()
        _lib.check(lib.gss_profile_topk(n, x.data_ptr(), _lib.row_stride(x), nc, _lib.ptr(lst), G, _lib.ptr(d_grp), int(k), idx.data_ptr(),
                                        val.data_ptr(), cnt.data_ptr(), ws.data_ptr(), need, _lib.current_stream()), "gss_profile_topk")
    return idx, val, cnt


def top_overlap(idx, cnt, a, b):
    """how many nodes two selections of top_nodes share, per group -> device tensor int32 [T][G]: entry (t, g) = the number of node indices
    in both idx[a[t]][g][:cnt] and idx[b[t]][g][:cnt] (len(np.intersect1d(...))); -1 where either side has cnt = -1.  idx, cnt: top_nodes'
    device tensors [S][G][k] and [S][G]; a, b: integer lists of T selection numbers in [0, S), on the host or the device; pairs may repeat
    (gss_topk_overlap).  No CPU fallback."""
    import torch
    if (not isinstance(idx, torch.Tensor) or not isinstance(cnt, torch.Tensor) or idx.dim() != 3 or cnt.dim() != 2 or idx.dtype != torch.int32
            or cnt.dtype != torch.int32 or tuple(cnt.shape) != tuple(idx.shape[:2])):
        raise ValueError("top_overlap: idx and cnt must be top_nodes' int32 tensors [S][G][k] and [S][G]")
    S, G, k = idx.shape
    if not 1 <= k <= MAX_TOP:
        raise ValueError(f"top_overlap: k={k} is outside [1, {MAX_TOP}]")
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"top_overlap: G={G} groups is outside [1, {MAX_GROUPS}]")
    lists = []
    for name, v in (("a", a), ("b", b)):
        if not (isinstance(v, torch.Tensor) and v.is_cuda):
            h = np.asarray(v, dtype=np.int64).reshape(-1)
            bad = np.flatnonzero((h < 0) | (h >= S))
            if len(bad):
                raise ValueError(f"top_overlap: {name}[{int(bad[0])}] = {int(h[bad[0]])} is outside [0, S={S})")
            v = torch.from_numpy(h.astype(np.int32))
        lists.append(v)
    if lists[0].numel() != lists[1].numel():
        raise ValueError(f"top_overlap: a lists {lists[0].numel()} selections and b {lists[1].numel()}")
    if not idx.is_cuda or not cnt.is_cuda:
        raise _lib.GssError("top_overlap: the selections are compared on the GPU only (no CPU fallback)")
    T = lists[0].numel()
    shared = torch.empty(T, G, dtype=torch.int32, device=idx.device)
    if T == 0:
        return shared
    lib = _lib.load()
    with torch.cuda.device(idx.device):
        da, db = (v.to(device=idx.device, dtype=torch.int32).contiguous().view(-1) for v in lists)
        idx, cnt = idx.contiguous(), cnt.contiguous()
        _lib.check(lib.gss_topk_overlap(S, G, k, idx.data_ptr(), cnt.data_ptr(), T, da.data_ptr(), db.data_ptr(), shared.data_ptr(),
                                        _lib.current_stream()), "gss_topk_overlap")
    return shared


def compare_profiles(profiles, rows, cols, metric, device="cuda"):
    """distance between diffusion profiles -> device tensor fp64 [len(rows)][len(cols)], scipy.spatial.distance.cdist's value of `metric`
    (one of ALL_METRICS) for every (row profile, column profile) pair; "spearman" = 1 - Spearman's rho = the correlation distance of the
    profiles' average-tie ranks (the unique profiles rows and cols name are ranked once by gss_profile_rank, then compared as correlation
    compares: a constant profile or one with a NaN gives NaN).  `profiles` is
      * the device tensor PprEngine.run returned, x [N][kpad] with profile c in column c: used in place; rows / cols are column indices;
      * a host array [K][N] (one profile per row): uploaded once, transposed into the kernel's layout; rows / cols index its rows;
      * the {name: vector} dict DiffusionProfiles.load_diffusion_profiles fills: the named profiles are uploaded once; rows / cols are names.
    rows / cols may repeat and come in any order; None means every profile (not for a dict).  An unknown metric is refused by name before
    the GPU is touched, and a host array or dict is uploaded only after every refusal the host can make.  No CPU fallback."""
    metric_id = check_metric(metric)
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError("profile distances run on the GPU only (no CPU fallback)")
    n, (ca, cb), upload = _profile_source(profiles, (rows, cols), ("row", "column"), "compare_profiles")
    out = torch.empty(len(ca), len(cb), dtype=torch.float64, device=dev)
    if len(ca) == 0 or len(cb) == 0:
        return out
    if n < 1:
        raise ValueError("compare_profiles: the profiles are empty")
    x = upload(dev)
    if metric in RANK_METRICS:   # the referenced profiles are ranked once; metric_id is the base metric's, applied to the ranks
        x, (ca, cb) = _rank_referenced(x, [ca, cb])
    with torch.cuda.device(x.device):
        la, lb = _device_list(ca, x.device), _device_list(cb, x.device)
        _lib.check(_lib.load().gss_profile_dist(n, x.data_ptr(), _lib.row_stride(x), len(ca), _lib.ptr(la), len(cb), _lib.ptr(lb), metric_id,
                                                out.data_ptr(), len(cb), _lib.current_stream()), "gss_profile_dist")
    return out


def compare_profile_pairs(profiles, col_a, col_b, metric, device="cuda"):
    """distance between listed pairs of diffusion profiles -> device tensor fp64 [T], entry t = scipy.spatial.distance's value of `metric`
    (one of ALL_METRICS; "spearman" as in compare_profiles) for profiles col_a[t] and col_b[t] (gss_profile_dist_pairs: T distances for the price of T, where compare_profiles
    would compute T x T and keep the diagonal).  `profiles` is what compare_profiles accepts: the device tensor PprEngine.run returned
    (x [N][kpad], profile c in column c, used in place), a host array [K][N] (the lists index its rows) or a {name: vector} dict (the lists
    are names; the named profiles are uploaded once).  Pairs may repeat and come in any order; an entry's bits do not depend on the rest of
    the list.  A host array or dict is uploaded only after every refusal the host can make.  No CPU fallback."""
    metric_id = check_metric(metric)
    import torch
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError("profile distances run on the GPU only (no CPU fallback)")
    n, (ca, cb), upload = _profile_source(profiles, (col_a, col_b), ("col_a", "col_b"), "compare_profile_pairs",
                                          required="col_a and col_b must list the pairs", lists_who="compare_profiles")
    if len(ca) != len(cb):
        raise ValueError(f"compare_profile_pairs: col_a lists {len(ca)} profiles and col_b {len(cb)}")
    if len(ca) == 0:
        return torch.empty(0, dtype=torch.float64, device=profiles.device if isinstance(profiles, torch.Tensor) else dev)
    if n < 1:
        raise ValueError("compare_profile_pairs: the profiles are empty")
    x = upload(dev)
    out = torch.empty(len(ca), dtype=torch.float64, device=x.device)
    if metric in RANK_METRICS:
        x, (ca, cb) = _rank_referenced(x, [ca, cb])
    lib = _lib.load()
    with torch.cuda.device(x.device):
        need = int(lib.gss_profile_dist_pairs_workspace_bytes(n, len(ca)))
        ws = _workspace(need, x.device)
        da, db = torch.from_numpy(ca).to(x.device), torch.from_numpy(cb).to(x.device)
        _lib.check(lib.gss_profile_dist_pairs(n, x.data_ptr(), _lib.row_stride(x), len(ca), da.data_ptr(), db.data_ptr(), metric_id,
                                              out.data_ptr(), ws.data_ptr(), need, _lib.current_stream()), "gss_profile_dist_pairs")
    return out


def diffusion_profiles(m0, starts, proteins_of, alpha, max_iter, tol, device="cuda", max_columns=4096):
    """p_visit vectors of the given start nodes -> (profiles [K][N] fp64, iterations [K]).
    m0[u, v] = weight of edge u -> v (nx.to_scipy_sparse_matrix of the weighted MSI, diffusion_profiles.py:22-28)."""
    starts = np.asarray(starts, dtype=np.int64)
    out = np.empty((len(starts), m0.shape[0]), dtype=np.float64)
    its = np.empty(len(starts), dtype=np.int32)
    for lo in range(0, len(starts), max_columns):
        sub = starts[lo:lo + max_columns]
        eng = PprEngine(PprProblem(m0, sub, proteins_of), device)
        x, it = eng.run(alpha, tol, max_iter)
        out[lo:lo + len(sub)] = x[:, :len(sub)].t().contiguous().cpu().numpy()
        its[lo:lo + len(sub)] = it
        del eng
    return out, its


class DiffusionProfiles:
    """diffusion_profiles.py:12-171.  `msi` is a gcn_drug_repurposing_amd.msi.MsiGraph (loaded, not yet weighted)."""

    def __init__(self, alpha, max_iter, tol, weights, num_cores, save_load_file_path):
        self.alpha = alpha
        self.max_iter = max_iter
        self.tol = tol
        self.weights = weights
        self.num_cores = num_cores     # kept for signature compatibility; the batch runs on one GPU
        self.save_load_file_path = save_load_file_path

    def clean_file_name(self, file_name):   # :92-93
        return "".join([c for c in file_name if c.isalpha() or c.isdigit() or c == ' ' or c == "_"]).rstrip()

    def save_diffusion_profile(self, diffusion_profile, selected_drug_or_indication):   # :95-97
        f = os.path.join(self.save_load_file_path, self.clean_file_name(selected_drug_or_indication) + "_p_visit_array.npy")
        np.save(f, diffusion_profile)

    def calculate_diffusion_profiles(self, msi, device="cuda"):   # :125-156
        os.makedirs(self.save_load_file_path, exist_ok=True)
        names = msi.names
        node2idx = {n: i for i, n in enumerate(names)}
        with open(os.path.join(self.save_load_file_path, "node2idx.pkl"), "wb") as f:   # msi.save_node2idx (msi.py:180-184)
            pickle.dump(node2idx, f)
        msi.weight_graph(self.weights)
        m0, _, _ = msi.to_csr()
        start_names = msi.drugs_in_graph + msi.indications_in_graph
        proteins_of = {node2idx[s]: [node2idx[p] for p in msi.drug_or_indication2proteins[s]] for s in start_names}
        prof, iters = diffusion_profiles(m0, [node2idx[s] for s in start_names], proteins_of, self.alpha, self.max_iter, self.tol, device)
        for s, v in zip(start_names, prof):
            self.save_diffusion_profile(v, s)
        self.iterations = dict(zip(start_names, iters.tolist()))
        return prof

    def load_diffusion_profiles(self, drugs_and_indications):   # :158-171
        assert self.save_load_file_path is not None
        out = {}
        for s in drugs_and_indications:
            path = os.path.join(self.save_load_file_path, self.clean_file_name(s) + "_p_visit_array.npy")
            if os.path.exists(path):
                out[s] = np.load(path)
            else:
                print("Loading failed at " + str(s) + " | " + str(path))
        self.drug_or_indication2diffusion_profile = out
