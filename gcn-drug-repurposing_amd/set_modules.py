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
from ._network_engine import MAX_SET, NetworkEngine
from .proximity import ProximityError, degree_bins

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


class ModuleEngine(NetworkEngine):
    """the network's device CSR and nothing else: no distance matrix.  set_table and components are NetworkEngine's"""

    def module_table(self, gene_sets, side, n_random=1000, seed=452456, min_bin_size=100):
        """gene_sets: a list of gene-id collections (intersected with the LCC here); side: 0 the drugs' random sets, 1 the diseases'.
        Returns {"n", "lcc", "n_comp", "n_edges", "short": int64 [n_sets] (the observed set; short = random sets that came out a member
        short), "lcc_stats", "edges_stats": null_stats of the LCC size / the induced edge count, "null_lcc", "null_edges": int32
        [n_sets, n_random], "members": the LCC node indices of every set, ascending, "label": per member the position of the smallest
        member of its component}.  An empty set has NaN statistics and takes no part in q."""
        n_random = self.null_arguments("module_table", gene_sets, side, n_random, min_bin_size)
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
