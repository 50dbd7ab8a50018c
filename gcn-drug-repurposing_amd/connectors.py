"""The seed connector algorithm (Wang and Loscalzo 2018, "Network-based disease module discovery by a novel seed connector algorithm with
pathobiological implications"): join the fragments of a disease's gene set -- or a drug's target set -- on the interactome.  Starting
from the set, every step adds the one node outside the module that most enlarges the largest connected component (LCC) of the subgraph
the module induces, until no node joins anything to it.  set_modules.py asks whether a set forms a module and diamond.py grows one by
connectivity significance; this names the connector proteins that hold the set together, and asks whether they join more of it than
they join of degree-matched random sets: the very sets, bit for bit, that proximity.py and set_modules.py score against.

Every seed set, and every random set of the null, is one unit of one kernel (csrc/seed_connect.hip; include/gssgcn.h has the
definition and the tie rule, DESIGN.md section 9.19 the cost model).  No CPU fallback: without the library or a GPU this raises.  Host
code is setup and the statistics over the integers that come back (table_stats).
"""
from __future__ import annotations

import numpy as np

from ._network_engine import NetworkEngine
from .proximity import ProximityError, degree_bins
from .set_modules import null_stats

MAX_NODES = 30720                # per node a 32-bit label in LDS
MAX_SEEDS = 4096                 # the seed table's row length
MAX_MEMBERS = 8192               # seeds + added nodes of one unit: 4 bytes each in LDS
STEP_FIELDS = ("node", "lcc", "merged", "deg")
UNIT_FIELDS = ("steps", "first_lcc", "final_lcc", "seeds_in", "added_in")
CHUNK_BYTES = 256 << 20          # the step outputs of one call: n_add x 16 bytes per unit


def table_stats(n, sizes, steps, final_lcc, seeds_in):
    """n int [n_sets] (genes on the LCC) and, per (set, sample) with sample 0 the set itself, the sizes and the growth's integers
    [n_sets, n_random + 1] -> {"joined_stats", "fraction_stats", "lcc_stats": null_stats of the seeds in the final LCC, of that count
    over the sample's size, and of the final LCC's size (more than random is the interesting side); "connectors": the set's steps,
    "connectors_null_mean", "connectors_null_sd": the random sets' (ddof = 0), reported beside it without a p-value; "short": random sets
    that came out a member short}.  A set with fewer than 2 genes has NaN statistics and takes no part in q."""
    n = np.asarray(n, np.int64)
    sizes, steps, final_lcc, seeds_in = (np.asarray(x, np.int64).reshape(len(n), -1) for x in (sizes, steps, final_lcc, seeds_in))
    if sizes.shape[1] < 2:
        raise ValueError("table_stats: the null holds no sample")
    empty = n < 2
    fraction = seeds_in / np.maximum(sizes, 1)
    null_steps = steps[:, 1:]
    mean = null_steps.sum(axis=1) / null_steps.shape[1]
    sd = np.sqrt(((null_steps - mean[:, None]) ** 2).sum(axis=1) / null_steps.shape[1])
    mean[empty] = sd[empty] = np.nan
    return {"joined_stats": null_stats(seeds_in[:, 0], seeds_in[:, 1:], empty),
            "fraction_stats": null_stats(fraction[:, 0], fraction[:, 1:], empty, real=True),
            "lcc_stats": null_stats(final_lcc[:, 0], final_lcc[:, 1:], empty),
            "connectors": steps[:, 0].copy(), "connectors_null_mean": mean, "connectors_null_sd": sd,
            "short": (sizes[:, 1:] < sizes[:, :1]).sum(axis=1)}


class ConnectorEngine(NetworkEngine):
    """the network's device CSR and nothing else"""

    def check(self, max_size, n_add):
        """the refusals that need no device, in the engine's words"""
        self._open("grow")
        if int(n_add) < 1:
            raise ProximityError(f"n_add={n_add} must be >= 1")
        if not 1 <= self.net.n <= MAX_NODES:
            raise ProximityError(f"a network of {self.net.n} nodes; between 1 and {MAX_NODES} are supported")
        if max_size > MAX_SEEDS:
            raise ProximityError(f"a set has {max_size} seeds; at most {MAX_SEEDS} are supported")
        if max_size + int(n_add) > MAX_MEMBERS:
            raise ProximityError(f"{max_size} seeds + n_add={n_add} is over {MAX_MEMBERS} members of a module")

    def run(self, seeds, sizes, n_add, steps_of=None, labels=False):
        """seeds [U, max_size], sizes [U]: a device seed table.  All U units grow, in as many calls as keep one call's step outputs within
        CHUNK_BYTES -> {"steps", "first_lcc", "final_lcc", "seeds_in", "added_in": int32 [U]} and, for the units listed in steps_of (ascending; None =
        none), {"node", "lcc", "merged", "deg": int32 [len(steps_of), n_add]}, with labels also {"label": int32 [len(steps_of),
        max_size + n_add], -1 past size + steps}, all host numpy"""
        from . import _lib
        torch = self._torch
        U, max_size = seeds.shape
        n_add = int(n_add)
        self.check(max_size, n_add)
        seeds, sizes = seeds.contiguous(), sizes.contiguous()
        keep = np.zeros(0, np.int64) if steps_of is None else np.asarray(steps_of, np.int64)
        per_unit = 16 * n_add + (4 * (max_size + n_add) if labels else 0)
        chunk = int(max(1, min(U, CHUNK_BYTES // per_unit)))
        step = [torch.empty((chunk, n_add), dtype=torch.int32, device=self._dev) for _ in STEP_FIELDS]
        label = torch.empty((chunk, max_size + n_add), dtype=torch.int32, device=self._dev) if labels else None
        unit = [torch.empty(U, dtype=torch.int32, device=self._dev) for _ in UNIT_FIELDS]
        kept = {f: [] for f in STEP_FIELDS + (("label",) if labels else ())}
        for lo in range(0, U, chunk):
            hi = min(U, lo + chunk)
            if labels:
                label.fill_(-1)
            _lib.check(self.lib.gss_seed_connectors(self.net.n, _lib.ptr(self._rowptr), _lib.ptr(self._col), self.max_deg, hi - lo, max_size,
                                                    _lib.ptr(seeds[lo:]), _lib.ptr(sizes[lo:]), n_add, *(_lib.ptr(x) for x in step),
                                                    *(_lib.ptr(x[lo:]) for x in unit), _lib.ptr(label), _lib.current_stream()),
                       "gss_seed_connectors")
            rows = torch.from_numpy(keep[(keep >= lo) & (keep < hi)] - lo).to(self._dev)
            for f, x in zip(STEP_FIELDS, step):
                kept[f].append(x[rows].cpu().numpy())
            if labels:
                kept["label"].append(label[rows].cpu().numpy())
        out = {f: x.cpu().numpy() for f, x in zip(UNIT_FIELDS, unit)}
        if steps_of is not None:
            out.update({f: np.concatenate(v) for f, v in kept.items()})
        return out

    def seed_table(self, node_sets):
        """(seeds [n_sets, max_size], sizes [n_sets]) device int32 of a list of node-index arrays (strictly ascending), and the arrays"""
        return self.pack(node_sets)

    def grow(self, node_sets, n_add=500):
        """node_sets: a list of node-index arrays (strictly ascending, as Network.node_set returns them) -> {"node", "lcc", "merged", "deg":
        int32 [n_sets, n_add]: per step the connector added, the LCC after it, the components it joined and its degree (node = -1 and
        zeros once a set stopped); "steps", "first_lcc", "final_lcc", "seeds_in", "added_in": int32 [n_sets] (the LCC before and after); "members": per set the seeds and then the
        connectors in the order added; "label": per member the position of the smallest member of its component}"""
        self._open("grow")
        seeds, sizes, sets = self.seed_table(node_sets)
        out = self.run(seeds, sizes, n_add, steps_of=np.arange(len(sets)), labels=True)
        label = out.pop("label")
        out["members"] = [np.concatenate([s, out["node"][i, :out["steps"][i]]]).astype(np.int32) for i, s in enumerate(sets)]
        out["label"] = [label[i, :len(m)].astype(np.int64) for i, m in enumerate(out["members"])]
        return out

    def connector_table(self, gene_sets, side, n_add=500, n_random=1000, seed=452456, min_bin_size=100):
        """gene_sets: a list of gene-id collections (intersected with the LCC here); side: 0 the drugs' random sets, 1 the diseases'.
        Every set and its n_random degree-matched random sets grow -> {"n": genes on the LCC, "grow": grow()'s return for the sets themselves, "sizes", "steps", "final_lcc", "seeds_in": int32 [n_sets, n_random + 1]
        (sample 0 the set), and table_stats' entries (absent with n_random = 0)}"""
        n_random = self.null_arguments("connector_table", gene_sets, side, n_random, min_bin_size, or_zero=True)
        self._open("connector_table")
        sets = [self.net.node_set(s) for s in gene_sets]
        self.check(max(1, max(len(s) for s in sets)), n_add)
        n = np.array([len(s) for s in sets], np.int64)
        own = self.grow(sets, n_add)
        out = {"n": n, "grow": own}
        nodes, sizes = self.set_table(sets, side, n_random, seed, degree_bins(self.net.degree, min_bin_size))
        R, max_size = n_random + 1, nodes.shape[2]
        res = self.run(nodes.reshape(-1, max_size), sizes.reshape(-1), n_add)
        out["sizes"] = sizes.cpu().numpy()
        out.update({f: res[f].reshape(len(sets), R) for f in ("steps", "final_lcc", "seeds_in")})
        if n_random:
            out.update(table_stats(n, out["sizes"], out["steps"], out["final_lcc"], out["seeds_in"]))
        return out
