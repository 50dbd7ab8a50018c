"""DIAMOnD (Ghiassian, Menche and Barabasi 2015, "A DIseAse MOdule Detection (DIAMOnD) algorithm derived from a systematic analysis of
connectivity patterns of disease proteins in the human interactome"): grow a module from a disease's seed genes, one node per step, each
step the node whose number of links into the module is the most significant under the hypergeometric null.  set_modules.py asks whether
a gene set forms a module; this grows one, and its result is what proximity.py and enrich.py take as a gene set.

Every seed set is one unit of one kernel launch (csrc/diamond.hip; include/gssgcn.h has the statistic, DESIGN.md section 9.18 the cost
model): the growth of all sets, and of all the reduced sets of a leave-out validation, runs side by side.  No CPU fallback: without the
library or a GPU this raises.  Host code is setup only: the lgamma table, the seed table, p = exp(min(logp, 0)).
"""
from __future__ import annotations

import math

import numpy as np

from ._network_engine import NetworkEngine
from .proximity import ProximityError

MAX_NODES = 30720                # per node a word of link counts and a membership bit in LDS, beside the 4,096-slot table
MAX_SEEDS = 4096                 # the seed table's row length
MAX_COUNT = 65535                # alpha x the largest degree: the link counts are 16 bits
SLOTS = 4096                     # weighted links into the module a node can have, + 1
FIELDS = ("node", "k", "kb", "lt0", "S", "logp", "p")


def lgamma_table(n):
    """lg[i] = lgamma(i) for i in [0, n) as fp64 (lg[0] = inf, never read): the table the kernel takes its binomials from"""
    lg = np.empty(int(n), np.float64)
    lg[0] = np.inf
    for i in range(1, int(n)):
        lg[i] = math.lgamma(i)
    return lg


def holdout_draws(node_sets, holdout, repeats, seed):
    """per set, `repeats` times (kept, held): numpy's default_rng(seed), sets in order and repeats in order, draws
    max(1, floor(holdout x size + 0.5)) members of a set of two or more without replacement (never all of them); a smaller set keeps
    what it has and holds nothing out.  Both arrays ascending int32"""
    if not 0.0 < float(holdout) < 1.0:
        raise ProximityError(f"holdout={holdout} must be in (0, 1)")
    if int(repeats) < 1:
        raise ProximityError(f"repeats={repeats} must be >= 1")
    rng = np.random.default_rng(int(seed))
    out = []
    for s in node_sets:
        s = np.asarray(s, np.int32)
        m = len(s)
        n_out = min(m - 1, max(1, int(math.floor(float(holdout) * m + 0.5)))) if m >= 2 else 0
        reps = []
        for _ in range(int(repeats)):
            gone = np.zeros(m, bool)
            gone[rng.choice(m, n_out, replace=False)] = True
            reps.append((s[~gone], s[gone]))
        out.append(reps)
    return out


class DiamondEngine(NetworkEngine):
    """the network's device CSR and the lgamma table"""

    def __init__(self, network):
        super().__init__(network)
        self._lg = None

    def close(self):
        super().close()
        self._lg = None

    def _table(self, n_lg):
        if self._lg is None or len(self._lg) < n_lg:
            self._lg = self._torch.from_numpy(lgamma_table(n_lg)).to(self._dev)
        return self._lg

    def check(self, node_sets, n_add, alpha):
        """the refusals that need no device, in the engine's words -> (seed arrays, max_size)"""
        n_add, alpha = int(n_add), int(alpha)
        if n_add < 1:
            raise ProximityError(f"n_add={n_add} must be >= 1")
        if alpha < 1:
            raise ProximityError(f"alpha={alpha} must be >= 1")
        sets, max_size = self.node_arrays(node_sets)
        if not 1 <= self.net.n <= MAX_NODES:
            raise ProximityError(f"a network of {self.net.n} nodes; between 1 and {MAX_NODES} are supported")
        big = max(len(s) for s in sets)
        if big > MAX_SEEDS:
            raise ProximityError(f"a set has {big} seeds; at most {MAX_SEEDS} are supported")
        if alpha * self.max_deg > MAX_COUNT:
            raise ProximityError(f"alpha={alpha} x the largest degree {self.max_deg} is over {MAX_COUNT}")
        top = min(alpha * self.max_deg, alpha * max_size + n_add - 1)
        if top >= SLOTS:
            raise ProximityError(f"a node can have {top} weighted links into a module (alpha={alpha}, largest degree {self.max_deg}, {big} seeds, "
                                 f"n_add={n_add}); at most {SLOTS - 1} are supported")
        return sets, max_size

    def grow(self, node_sets, n_add=200, alpha=1):
        """node_sets: a list of node-index arrays (strictly ascending, as Network.node_set returns them) -> {"node", "k", "kb": int32,
        "lt0", "S", "logp", "p": fp64}, each [n_sets, n_add]: per step the node added, its k' and kb', the log of the leading
        hypergeometric term, the tail sum relative to it, logp = lt0 + log(S) and p = exp(min(logp, 0)).  Once a set's surroundings are
        used up, node = -1 and p = NaN for the rest of its steps."""
        from . import _lib
        torch = self._torch
        self._open("grow")
        n_add, alpha = int(n_add), int(alpha)
        sets, max_size = self.check(node_sets, n_add, alpha)
        U = len(sets)
        d_seeds, d_sizes, _ = self.pack(sets)
        lg = self._table(self.net.n + (alpha - 1) * max_size + 2)
        ints = [torch.empty((U, n_add), dtype=torch.int32, device=self._dev) for _ in range(3)]
        reals = [torch.empty((U, n_add), dtype=torch.float64, device=self._dev) for _ in range(3)]
        _lib.check(self.lib.gss_diamond_grow(self.net.n, _lib.ptr(self._rowptr), _lib.ptr(self._col), self.max_deg, _lib.ptr(lg), len(lg), U,
                                             max_size, _lib.ptr(d_seeds), _lib.ptr(d_sizes), n_add, alpha, *(_lib.ptr(x) for x in ints),
                                             *(_lib.ptr(x) for x in reals), _lib.current_stream()), "gss_diamond_grow")
        out = {f: x.cpu().numpy() for f, x in zip(FIELDS, ints + reals)}
        out["p"] = np.where(out["node"] >= 0, np.exp(np.minimum(out["logp"], 0.0)), np.nan)
        return out

    def recovery(self, node_sets, holdout=0.25, repeats=100, seed=0, n_add=200, alpha=1):
        """leave-out validation: holdout_draws removes a fraction of every set `repeats` times, all n_sets x repeats reduced sets grow in
        one call -> {"recovered": int64 [n_sets, n_add], over the repeats the held-out nodes among the first r + 1 nodes added;
        "held": int64 [n_sets], the nodes held out over the repeats; "draws": what holdout_draws returned}"""
        draws = holdout_draws(node_sets, holdout, repeats, seed)
        flat = [kept for reps in draws for kept, _ in reps]
        node = self.grow(flat, n_add=n_add, alpha=alpha)["node"].reshape(len(draws), int(repeats), int(n_add))
        rec = np.zeros((len(draws), int(n_add)), np.int64)
        for i, reps in enumerate(draws):
            for j, (_, held) in enumerate(reps):
                rec[i] += np.cumsum(np.isin(node[i, j], held) & (node[i, j] >= 0))
        return {"recovered": rec, "held": np.array([sum(len(h) for _, h in reps) for reps in draws], np.int64), "draws": draws}
