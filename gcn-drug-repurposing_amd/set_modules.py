"""Module significance of gene sets (Menche et al. 2015, "Uncovering disease-disease relationships through the incomplete interactome"):
does a disease's gene set -- or a drug's target set -- form a module on the interactome at all?  The statistic is the size of the largest
connected component of the subgraph the set induces on the network's LCC, compared with the same statistic over degree-matched random
sets of the same size: the very sets, bit for bit, that proximity.py's z-scores are computed against (side 0 drugs, side 1 diseases, the
same seed).  The induced edge count is reported beside it.

The random sets and the component search run in HIP kernels (csrc/proximity.hip random_sets_kernel, csrc/set_modules.hip); no CPU
fallback: without the library or a GPU this raises.  The statistics are host numpy over the integers that come back (null_stats).
"""
from __future__ import annotations

import numpy as np

from ._nulls import benjamini_hochberg
from .proximity import ProximityError, degree_bins, random_set_table

MAX_SET = 4096                   # members of one set the component kernel holds in LDS
STAT_FIELDS = ("mean", "sd", "z", "p", "q")


def null_stats(obs, null, empty=None, real=False):
    """obs [n_sets] and null [n_sets, n_random] integers -> {"mean", "sd", "z", "p", "q": fp64 [n_sets]}: the null's mean (computed once:
    the integer sum divided once) and population sd (ddof = 0) about it, z = (obs - mean) / sd (NaN when sd = 0), the one-sided
    p = (1 + #{r: null_r >= obs}) / (n_random + 1), and Benjamini-Hochberg q over the sets that are not `empty` (bool [n_sets]; those get
    NaN everywhere and take no part in q).  With `real` the statistic is a ratio of integers (connectors.py's fraction of a set joined)
    and is taken as fp64 instead"""
    kind = np.float64 if real else np.int64
    obs = np.asarray(obs, kind)
    null = np.asarray(null, kind).reshape(len(obs), -1)
    k = null.shape[1]
    if k < 1:
        raise ValueError("null_stats: the null holds no sample")
    live = np.ones(len(obs), bool) if empty is None else ~np.asarray(empty, bool)
    mean = null.sum(axis=1) / k
    dev = null - mean[:, None]
    sd = np.sqrt((dev * dev).sum(axis=1) / k)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = np.where(sd > 0, (obs - mean) / np.where(sd > 0, sd, 1.0), np.nan)
    p = (1 + (null >= obs[:, None]).sum(axis=1)) / (k + 1)
    q = np.full(len(obs), np.nan)
    if live.any():
        q[live] = benjamini_hochberg(p[live])
    out = {"mean": mean, "sd": sd, "z": z, "p": p, "q": q}
    for v in out.values():
        v[~live] = np.nan
    return out


def largest_component(label):
    """the label of the largest component of one set's labels (None for an empty set); of two as large, the smaller label"""
    label = np.asarray(label, np.int64)
    if len(label) == 0:
        return None
    count = np.bincount(label)
    return int(np.argmax(count))          # argmax returns the first, i.e. the smallest label, of equal counts


class ModuleEngine:
    """owns the device CSR of `network` (a proximity.Network) and nothing else: no distance matrix"""

    def __init__(self, network):
        import torch
        from . import _lib
        self.lib = _lib.load()
        self.net = network
        self._torch = torch
        self._dev = torch.device("cuda")
        self._rowptr = torch.from_numpy(network.rowptr).to(self._dev)
        self._col = torch.from_numpy(network.col if len(network.col) else np.zeros(1, np.int32)).to(self._dev)

    def close(self):
        self._rowptr = self._col = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def set_table(self, node_sets, side, n_random, seed, bins):
        """random sets of every set (sample 0 = the set) -> (nodes [n_sets, R, max_size], sizes [n_sets, R]) device int32: what
        ProximityEngine.set_table returns, bit for bit"""
        n = self.net.n
        return random_set_table(lambda *args: self.lib.gss_random_sets(n, *args), "gss_random_sets", n, self._dev, node_sets, side, n_random,
                                seed, bins)

    def components(self, nodes, sizes, labels=False):
        """a set table -> device int32 lcc, n_comp, n_edges [n_sets, R] (and label [n_sets, R, max_size], -1 past every size, with labels)"""
        from . import _lib
        torch = self._torch
        if self._rowptr is None:
            raise ProximityError("components: the engine is closed")
        n_sets, R, max_size = nodes.shape
        if max_size > MAX_SET:
            raise ProximityError(f"a set table of up to {max_size} nodes per set; at most {MAX_SET} are supported")
        nodes, sizes = nodes.contiguous(), sizes.contiguous()
        lcc, n_comp, n_edges = (torch.empty((n_sets, R), dtype=torch.int32, device=self._dev) for _ in range(3))
        label = torch.full((n_sets, R, max_size), -1, dtype=torch.int32, device=self._dev) if labels else None
        _lib.check(self.lib.gss_set_components(self.net.n, _lib.ptr(self._rowptr), _lib.ptr(self._col), n_sets * R, max_size, _lib.ptr(nodes),
                                               _lib.ptr(sizes), _lib.ptr(lcc), _lib.ptr(n_comp), _lib.ptr(n_edges), _lib.ptr(label),
                                               _lib.current_stream()), "gss_set_components")
        return (lcc, n_comp, n_edges, label) if labels else (lcc, n_comp, n_edges)

    def module_table(self, gene_sets, side, n_random=1000, seed=452456, min_bin_size=100):
        """gene_sets: a list of gene-id collections (intersected with the LCC here); side: 0 the drugs' random sets, 1 the diseases'.
        Returns {"n", "lcc", "n_comp", "n_edges", "short": int64 [n_sets] (the observed set; short = random sets that came out a member
        short), "lcc_stats", "edges_stats": null_stats of the LCC size / the induced edge count, "null_lcc", "null_edges": int32
        [n_sets, n_random], "members": the LCC node indices of every set, ascending, "label": per member the position of the smallest
        member of its component}.  An empty set has NaN statistics and takes no part in q."""
        if int(n_random) < 2:
            raise ProximityError(f"n_random={n_random}: need at least 2 random samples for a standard deviation")
        if int(min_bin_size) < 1:
            raise ProximityError(f"min_bin_size={min_bin_size} must be >= 1")
        if side not in (0, 1):
            raise ProximityError(f"side={side} must be 0 (drugs) or 1 (diseases)")
        if not gene_sets:
            raise ProximityError("module_table: gene_sets must not be empty")
        n_random = int(n_random)
        sets = [self.net.node_set(s) for s in gene_sets]
        big = max(len(s) for s in sets)
        if big > MAX_SET:
            raise ProximityError(f"a set has {big} genes in the LCC; at most {MAX_SET} are supported")
        bins = degree_bins(self.net.degree, min_bin_size)
        nodes, sizes = self.set_table(sets, side, n_random, seed, bins)
        lcc, n_comp, n_edges = (x.cpu().numpy() for x in self.components(nodes, sizes))
        label = self.components(nodes[:, :1], sizes[:, :1], labels=True)[3][:, 0].cpu().numpy()
        sz = sizes.cpu().numpy()
        n = np.array([len(s) for s in sets], np.int64)
        empty = n == 0
        return {"n": n, "lcc": lcc[:, 0].astype(np.int64), "n_comp": n_comp[:, 0].astype(np.int64), "n_edges": n_edges[:, 0].astype(np.int64),
                "short": (sz[:, 1:] < sz[:, :1]).sum(axis=1).astype(np.int64),
                "lcc_stats": null_stats(lcc[:, 0], lcc[:, 1:], empty), "edges_stats": null_stats(n_edges[:, 0], n_edges[:, 1:], empty),
                "null_lcc": np.ascontiguousarray(lcc[:, 1:]), "null_edges": np.ascontiguousarray(n_edges[:, 1:]),
                "members": sets, "label": [label[i, :len(s)].astype(np.int64) for i, s in enumerate(sets)]}
