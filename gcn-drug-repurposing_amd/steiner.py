"""Approximate Steiner trees of gene sets on the interactome: the smallest subnetwork that connects a disease's genes -- or a drug's
targets --, by Mehlhorn's 1988 form of the Kou-Markowsky-Berman 2(1 - 1/l) approximation on unit edge weights.  Every node finds its
nearest seed, the edges between the regions of two seeds are bridges of weight dist + dist + 1, the minimum spanning forest of the
seeds over the bridges (ties by the bridge's nodes) is the tree's skeleton, and the shortest paths under the chosen bridges fill it in.
set_modules.py asks whether a set forms a module, diamond.py grows one, connectors.py joins its fragments greedily; this connects every
seed of a component, names the connector (Steiner) nodes, and asks whether the set needs fewer of them, or a shorter tree, than
degree-matched random sets: the very sets, bit for bit, that proximity.py and set_modules.py score against.  Fewer connectors and a
shorter tree than random are the signal, so both statistics take the lower tail: p = (1 + #{random <= observed}) / (n_random + 1).

Every seed set, and every random set of the null, is one unit of one kernel (csrc/steiner.hip; include/gssgcn.h has the definition and
the tie rules, DESIGN.md section 9.20 the cost model).  No CPU fallback: without the library or a GPU this raises.  Host code is setup
and the statistics over the integers that come back (table_stats).
"""
from __future__ import annotations

import numpy as np

from ._network_engine import NetworkEngine
from .proximity import ProximityError, degree_bins
from .set_modules import null_stats

MAX_NODES = 30720                # a node index is 15 bits of a bridge's key
MAX_SEEDS = 4096                 # the seed table's row length: a position is 12 bits of a node's word
LDS_BUDGET = 160 * 1024 - 512    # 4 bytes per node + 16 per seed position must fit
COUNT_FIELDS = ("n_comp", "length", "n_steiner", "n_edges", "max_w")
CHUNK_BYTES = 256 << 20          # the outputs of one call: 20 bytes per unit, with lists 8 max_add + 8 (max_size - 1) more


def lower_tail_stats(obs, null, empty=None):
    """set_modules.null_stats with the lower tail: p = (1 + #{r: null_r <= obs}) / (n_random + 1); mean, sd and z as they are"""
    s = null_stats(-np.asarray(obs, np.int64), -np.asarray(null, np.int64), empty)
    s["mean"], s["z"] = -s["mean"], -s["z"]
    return s


def table_stats(n, sizes, n_steiner, length):
    """n int [n_sets] (genes on the LCC) and, per (set, sample) with sample 0 the set itself, the sizes and the trees' integers
    [n_sets, n_random + 1] -> {"steiner_stats", "length_stats": lower_tail_stats of the Steiner nodes and of the tree's length; "short":
    random sets that came out a member short}.  A set with fewer than 2 genes has NaN statistics and takes no part in q."""
    n = np.asarray(n, np.int64)
    sizes, n_steiner, length = (np.asarray(x, np.int64).reshape(len(n), -1) for x in (sizes, n_steiner, length))
    if sizes.shape[1] < 2:
        raise ValueError("table_stats: the null holds no sample")
    empty = n < 2
    return {"steiner_stats": lower_tail_stats(n_steiner[:, 0], n_steiner[:, 1:], empty),
            "length_stats": lower_tail_stats(length[:, 0], length[:, 1:], empty),
            "short": (sizes[:, 1:] < sizes[:, :1]).sum(axis=1)}


def tree_edges(steiner, parent, bridge):
    """one tree's edge list [(a, b, kind)]: the parent edges (a the Steiner node, kind "path") and then the bridges ("bridge")"""
    return [(int(x), int(p), "path") for x, p in zip(steiner, parent)] + [(int(a), int(b), "bridge") for a, b in bridge]


class SteinerEngine(NetworkEngine):
    """the network's device CSR and nothing else"""

    def check(self, max_size, max_add=0):
        """the refusals that need no device, in the engine's words"""
        self._open("trees")
        if int(max_add) < 0:
            raise ProximityError(f"max_add={max_add} must be >= 0")
        if not 1 <= self.net.n <= MAX_NODES:
            raise ProximityError(f"a network of {self.net.n} nodes; between 1 and {MAX_NODES} are supported")
        if max_size > MAX_SEEDS:
            raise ProximityError(f"a set has {max_size} seeds; at most {MAX_SEEDS} are supported")
        need = 4 * self.net.n + 16 * max_size
        if need > LDS_BUDGET:
            raise ProximityError(f"a network of {self.net.n} nodes with sets of up to {max_size} seeds needs {need} bytes of LDS; "
                                 f"4 n + 16 max_size may be {LDS_BUDGET} at the most")

    def run(self, seeds, sizes, max_add=0, lists=False):
        """seeds [U, max_size], sizes [U]: a device seed table.  All U units, in as many calls as keep one call's outputs within
        CHUNK_BYTES -> {the COUNT_FIELDS: int32 [U]} and with lists {"steiner", "parent": int32 [U, max_add], "bridge": int32
        [U, max_size - 1, 2]}, -1 past the counts, all host numpy"""
        from . import _lib
        torch = self._torch
        U, max_size = seeds.shape
        max_add = int(max_add)
        self.check(max_size, max_add)
        seeds, sizes = seeds.contiguous(), sizes.contiguous()
        per_unit = 4 * len(COUNT_FIELDS) + (8 * max_add + 8 * (max_size - 1) if lists else 0)
        chunk = int(max(1, min(U, CHUNK_BYTES // per_unit)))
        counts = [torch.empty(U, dtype=torch.int32, device=self._dev) for _ in COUNT_FIELDS]
        shapes = {"steiner": (chunk, max_add), "parent": (chunk, max_add), "bridge": (chunk, max_size - 1, 2)}
        bufs = {f: torch.empty(shape, dtype=torch.int32, device=self._dev) for f, shape in shapes.items()} if lists else {}
        kept = {f: [] for f in bufs}
        for lo in range(0, U, chunk):
            hi = min(U, lo + chunk)
            for x in bufs.values():
                x.fill_(-1)
            _lib.check(self.lib.gss_steiner_trees(self.net.n, _lib.ptr(self._rowptr), _lib.ptr(self._col), self.max_deg, hi - lo, max_size,
                                                  _lib.ptr(seeds[lo:]), _lib.ptr(sizes[lo:]), max_add, *(_lib.ptr(x[lo:]) for x in counts),
                                                  *(_lib.ptr(bufs[f]) if lists else None for f in shapes), _lib.current_stream()),
                       "gss_steiner_trees")
            for f, x in bufs.items():
                kept[f].append(x[:hi - lo].cpu().numpy())
        out = {f: x.cpu().numpy() for f, x in zip(COUNT_FIELDS, counts)}
        out.update({f: np.concatenate(v) for f, v in kept.items()})
        return out

    def trees(self, node_sets, max_add=4096):
        """node_sets: a list of node-index arrays (strictly ascending, as Network.node_set returns them) -> {"n_comp", "length",
        "n_steiner", "n_edges", "max_w": int32 [n_sets]; per set "terminals"; "steiner": the Steiner nodes in ascending order (the first
        max_add when there are more: "truncated" says where) and "parent": theirs; "bridge": int32 [k, 2] ascending; "edges": [(a, b,
        kind)], the parent edges ("path") and then the bridges ("bridge")}"""
        self._open("trees")
        seeds, sizes, sets = self.pack(node_sets)
        out = self.run(seeds, sizes, max_add, lists=True)
        listed = np.minimum(out["n_steiner"], int(max_add))
        n_bridge = np.array([len(s) for s in sets], np.int64) - out["n_comp"]
        steiner, parent, bridge = out["steiner"], out["parent"], out["bridge"]
        out["terminals"] = sets
        out["steiner"] = [steiner[i, :listed[i]] for i in range(len(sets))]
        out["parent"] = [parent[i, :listed[i]] for i in range(len(sets))]
        out["bridge"] = [bridge[i, :n_bridge[i]] for i in range(len(sets))]
        out["truncated"] = out["n_steiner"] > int(max_add)
        out["edges"] = [tree_edges(s, p, b) for s, p, b in zip(out["steiner"], out["parent"], out["bridge"])]
        return out

    def tree_table(self, gene_sets, side, n_random=1000, seed=452456, min_bin_size=100, max_add=4096):
        """gene_sets: a list of gene-id collections (intersected with the LCC here); side: 0 the drugs' random sets, 1 the diseases'.
        Every set and its n_random degree-matched random sets are connected -> {"n": genes on the LCC, "trees": trees()'s return for the
        sets themselves, "sizes", "n_comp", "length", "n_steiner": int32 [n_sets, n_random + 1] (sample 0 the set), and table_stats'
        entries (absent with n_random = 0): the lower tail, fewer connectors and a shorter tree than random being the signal}"""
        n_random = self.null_arguments("tree_table", gene_sets, side, n_random, min_bin_size, or_zero=True)
        self._open("tree_table")
        sets = [self.net.node_set(s) for s in gene_sets]
        self.check(max(1, max(len(s) for s in sets)), max_add)
        n = np.array([len(s) for s in sets], np.int64)
        out = {"n": n, "trees": self.trees(sets, max_add)}
        nodes, sizes = self.set_table(sets, side, n_random, seed, degree_bins(self.net.degree, min_bin_size))
        R, max_size = n_random + 1, nodes.shape[2]
        res = self.run(nodes.reshape(-1, max_size), sizes.reshape(-1))
        out["sizes"] = sizes.cpu().numpy()
        out.update({f: res[f].reshape(len(sets), R) for f in ("n_comp", "length", "n_steiner")})
        if n_random:
            out.update(table_stats(n, out["sizes"], out["n_steiner"], out["length"]))
        return out
