"""NetworkEngine: what the engines over a table of node sets share (set_modules.ModuleEngine, diamond.DiamondEngine,
connectors.ConnectorEngine).  It owns the device CSR of one proximity.Network, packs lists of node sets into the -1-padded table the
kernels take (csrc/seed_units.h has the table's contract), draws the degree-matched random sets, and searches the components of a table.
"""
from __future__ import annotations

import numpy as np

from .proximity import ProximityError, random_set_table

MAX_SET = 4096                   # members of one set the component kernel holds in LDS


class NetworkEngine:
    """owns the device CSR of `network` (a proximity.Network)"""

    def __init__(self, network):
        import torch
        from . import _lib
        self.lib = _lib.load()
        self.net = network
        self._torch = torch
        self._dev = torch.device("cuda")
        self.max_deg = int(np.diff(network.rowptr).max()) if network.n else 0
        self._rowptr = torch.from_numpy(network.rowptr).to(self._dev)
        self._col = torch.from_numpy(network.col if len(network.col) else np.zeros(1, np.int32)).to(self._dev)

    def close(self):
        self._rowptr = self._col = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _open(self, what):
        if self._rowptr is None:
            raise ProximityError(f"{what}: the engine is closed")

    @staticmethod
    def null_arguments(what, gene_sets, side, n_random, min_bin_size, or_zero=False):
        """the refusals every table against random sets shares -> int(n_random); with or_zero, n_random = 0 asks for no null"""
        if int(n_random) < 2 and not (or_zero and int(n_random) == 0):
            raise ProximityError(f"n_random={n_random}: need at least 2 random samples for a standard deviation"
                                 + (" (or 0 for no null)" if or_zero else ""))
        if int(min_bin_size) < 1:
            raise ProximityError(f"min_bin_size={min_bin_size} must be >= 1")
        if side not in (0, 1):
            raise ProximityError(f"side={side} must be 0 (drugs) or 1 (diseases)")
        if not gene_sets:
            raise ProximityError(f"{what}: gene_sets must not be empty")
        return int(n_random)

    @staticmethod
    def node_arrays(node_sets):
        """a list of node sets -> (flat int32 arrays, the table's row length: the largest set's, at least 1)"""
        sets = [np.asarray(s, np.int32).reshape(-1) for s in node_sets]
        if not sets:
            raise ProximityError("grow: node_sets must not be empty")
        return sets, max(1, max(len(s) for s in sets))

    def pack(self, node_sets):
        """a list of node-index arrays (strictly ascending) -> (nodes [n_sets, max_size], -1 past every size, and sizes [n_sets], device
        int32, and the arrays)"""
        sets, max_size = self.node_arrays(node_sets)
        nodes = np.full((len(sets), max_size), -1, np.int32)
        for i, s in enumerate(sets):
            nodes[i, :len(s)] = s
        sizes = np.array([len(s) for s in sets], np.int32)
        return self._torch.from_numpy(nodes).to(self._dev), self._torch.from_numpy(sizes).to(self._dev), sets

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
        self._open("components")
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
