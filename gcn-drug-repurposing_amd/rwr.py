"""Random walk with restart (network propagation; Koehler et al. 2008, the comparator of the DIAMOnD paper): the walk restarts on a gene
set with probability `restart`, every other gene is ranked by its steady-state visit probability, and the hub bias of that ranking is
measured against the degree-matched random sets proximity.py draws.  diamond.py grows a module from a set; this ranks the whole network
from it, and its recovery table is what DIAMOnD's is read against.

Every seed set -- and every random set of the null, and every reduced set of a leave-out validation -- is one unit of one kernel launch
(csrc/rwr.hip; include/gssgcn.h has the iteration and the order of its sums, DESIGN.md section 9.21 the cost model).  No CPU fallback:
without the library or a GPU this raises.  Host code is setup only: the seed table, the batches of the null, the empirical p."""
from __future__ import annotations

import numpy as np

from ._network_engine import NetworkEngine
from .diamond import holdout_draws
from .proximity import ProximityError, degree_bins

MAX_NODES = 20000                # q of every node lives in LDS: 8 bytes each of the 163,840 a workgroup may declare
MAX_SEEDS = 4096                 # the seed table's row length
MAX_ADD = 1024                   # the selection's length
SCRATCH_BYTES = 256 << 20        # the null's vectors of one batch of sets (proximity.hip's default)
NOT_CONVERGED = -34              # GSS_ENOTCONV
STAT_FIELDS = ("p", "mean", "sd", "z", "ge", "emp_p")


class RwrEngine(NetworkEngine):
    """the network's device CSR and nothing else"""

    def check(self, node_sets, n_add, restart, tol, max_iter):
        """the refusals that need no device, in the engine's words -> (seed arrays, max_size)"""
        if not 1 <= int(n_add) <= MAX_ADD:
            raise ProximityError(f"n_add={n_add} must be in [1, {MAX_ADD}]")
        if not 0.0 < float(restart) < 1.0:
            raise ProximityError(f"restart={restart} must be in (0, 1)")
        if not float(tol) >= 0.0:
            raise ProximityError(f"tol={tol} must be >= 0")
        if int(max_iter) < 1:
            raise ProximityError(f"max_iter={max_iter} must be >= 1")
        sets, max_size = self.node_arrays(node_sets)
        if not 2 <= self.net.n <= MAX_NODES:
            raise ProximityError(f"a network of {self.net.n} nodes; between 2 and {MAX_NODES} are supported")
        if max_size > MAX_SEEDS:
            raise ProximityError(f"a set has {max_size} seeds; at most {MAX_SEEDS} are supported")
        return sets, max_size

    def _walk(self, what, nodes, sizes, n_add, restart, tol, max_iter, rank, p_out):
        """one gss_rwr_rank over a device table nodes [U, max_size], sizes [U] -> (node, score, iters) device tensors (the first two None
        without `rank`); p_out None or a device fp64 [U, n]"""
        from . import _lib
        torch = self._torch
        U, max_size = nodes.shape
        node = torch.empty((U, n_add), dtype=torch.int32, device=self._dev) if rank else None
        score = torch.empty((U, n_add), dtype=torch.float64, device=self._dev) if rank else None
        iters = torch.empty(U, dtype=torch.int32, device=self._dev)
        rc = self.lib.gss_rwr_rank(self.net.n, _lib.ptr(self._rowptr), _lib.ptr(self._col), self.max_deg, U, max_size, _lib.ptr(nodes),
                                   _lib.ptr(sizes), float(restart), float(tol), int(max_iter), int(n_add), _lib.ptr(node), _lib.ptr(score),
                                   _lib.ptr(iters), _lib.ptr(p_out), _lib.current_stream())
        if rc == NOT_CONVERGED:
            raise ProximityError(f"{what}: {self.lib.gss_last_error().decode(errors='replace')}")
        _lib.check(rc, "gss_rwr_rank")
        return node, score, iters

    def rank(self, node_sets, n_add=200, restart=0.75, tol=1e-6, max_iter=1000):
        """node_sets: a list of node-index arrays (strictly ascending, as Network.node_set returns them) -> {"node": int32, "score": fp64,
        both [n_sets, n_add]: the nodes outside the set by (visit probability descending, node ascending) and their probabilities, -1 and
        NaN past the candidates and for an empty set; "iters": int32 [n_sets]}"""
        self._open("rank")
        self.check(node_sets, n_add, restart, tol, max_iter)
        nodes, sizes, _ = self.pack(node_sets)
        node, score, iters = self._walk("rank", nodes, sizes, int(n_add), restart, tol, max_iter, True, None)
        return {"node": node.cpu().numpy(), "score": score.cpu().numpy(), "iters": iters.cpu().numpy()}

    def profiles(self, node_sets, restart=0.75, tol=1e-6, max_iter=1000):
        """-> {"p": fp64 [n_sets, n], every set's visit probabilities (a NaN row for an empty set); "iters": int32 [n_sets]}"""
        self._open("profiles")
        self.check(node_sets, 1, restart, tol, max_iter)
        nodes, sizes, _ = self.pack(node_sets)
        p = self._torch.empty((len(node_sets), self.net.n), dtype=self._torch.float64, device=self._dev)
        _, _, iters = self._walk("profiles", nodes, sizes, 1, restart, tol, max_iter, False, p)
        return {"p": p.cpu().numpy(), "iters": iters.cpu().numpy()}

    def recovery(self, node_sets, holdout=0.25, repeats=100, seed=0, n_add=200, restart=0.75, tol=1e-6, max_iter=1000):
        """leave-out validation on DiamondEngine.recovery's draws (diamond.holdout_draws): all n_sets x repeats reduced sets walk in one
        call -> the same dictionary, {"recovered": int64 [n_sets, n_add], over the repeats the held-out nodes among the first r + 1
        ranked; "held": int64 [n_sets]; "draws"}"""
        draws = holdout_draws(node_sets, holdout, repeats, seed)
        flat = [kept for reps in draws for kept, _ in reps]
        node = self.rank(flat, n_add=n_add, restart=restart, tol=tol, max_iter=max_iter)["node"].reshape(len(draws), int(repeats), int(n_add))
        rec = np.zeros((len(draws), int(n_add)), np.int64)
        for i, reps in enumerate(draws):
            for j, (_, held) in enumerate(reps):
                rec[i] += np.cumsum(np.isin(node[i, j], held) & (node[i, j] >= 0))
        return {"recovered": rec, "held": np.array([sum(len(h) for _, h in reps) for reps in draws], np.int64), "draws": draws}

    def score_table(self, gene_sets, side, n_random=1000, seed=452456, min_bin_size=100, n_add=200, rank_by="p", restart=0.75, tol=1e-6,
                    max_iter=1000, batch_sets=None, scratch_bytes=SCRATCH_BYTES):
        """gene_sets: a list of gene-id collections (intersected with the LCC here); side: 0 the drugs' random sets, 1 the diseases' --
        NetworkEngine.set_table's, the very sets proximity.py draws.  Every set and its n_random random sets walk; per node the null's
        mean and population sd, z = (p - mean) / sd (0 where sd = 0) and ge = #{null >= p}.  The nodes outside the set are ranked by
        rank_by: "p" (p descending, node ascending) or "z" (z descending, then p, then node).
        -> {"node": int32 [n_sets, n_add] (-1 past the candidates); "p", "mean", "sd", "z", "emp_p" = (1 + ge) / (n_random + 1): fp64, and
        "ge": int32, all [n_sets, n_add], NaN (ge -1) beside node = -1; "iters": int32 [n_sets], the set's own walk; "members"}.
        The sets are walked in batches whose vectors fit scratch_bytes (one set's are (n_random + 1) n 8 bytes), batch_sets at the most;
        the random sets are drawn once for the whole list, so no bit of the result depends on the batches."""
        from . import _lib
        torch = self._torch
        self._open("score_table")
        n_random = self.null_arguments("score_table", gene_sets, side, n_random, min_bin_size)
        if rank_by not in ("p", "z"):
            raise ProximityError(f"rank_by={rank_by!r} must be 'p' or 'z'")
        if batch_sets is not None and int(batch_sets) < 1:
            raise ProximityError(f"batch_sets={batch_sets} must be >= 1")
        sets = [self.net.node_set(s) for s in gene_sets]
        self.check(sets, n_add, restart, tol, max_iter)
        n, n_add, R, S = self.net.n, int(n_add), n_random + 1, len(sets)
        nodes, sizes = self.set_table(sets, side, n_random, seed, degree_bins(self.net.degree, min_bin_size))
        nodes, sizes = nodes.contiguous(), sizes.contiguous()
        max_size = nodes.shape[2]
        batch = max(1, int(scratch_bytes) // (R * n * 8))
        if batch_sets is not None:
            batch = min(batch, int(batch_sets))
        batch = min(batch, S)
        p = torch.empty((batch, R, n), dtype=torch.float64, device=self._dev)
        mean, sd, z = (torch.empty((batch, n), dtype=torch.float64, device=self._dev) for _ in range(3))
        ge = torch.empty((batch, n), dtype=torch.int32, device=self._dev)
        node = torch.empty((batch, n_add), dtype=torch.int32, device=self._dev)
        out = {"node": np.full((S, n_add), -1, np.int32), "ge": np.full((S, n_add), -1, np.int32), "iters": np.zeros(S, np.int32)}
        out.update({f: np.full((S, n_add), np.nan) for f in ("p", "mean", "sd", "z", "emp_p")})
        for s0 in range(0, S, batch):
            b = min(batch, S - s0)
            _, _, iters = self._walk("score_table", nodes[s0:s0 + b].reshape(b * R, max_size), sizes[s0:s0 + b].reshape(b * R), 1, restart, tol,
                                     max_iter, False, p)
            _lib.check(self.lib.gss_rwr_null_stats(n, b, R, _lib.ptr(p), max_size, _lib.ptr(nodes[s0:]), _lib.ptr(sizes[s0:]), n_add,
                                                   int(rank_by == "z"), _lib.ptr(mean), _lib.ptr(sd), _lib.ptr(z), _lib.ptr(ge), _lib.ptr(node),
                                                   _lib.current_stream()), "gss_rwr_null_stats")
            got = node[:b].cpu().numpy()
            at = torch.from_numpy(np.maximum(got, 0).astype(np.int64)).to(self._dev)
            cols = {"p": p[:b, 0], "mean": mean[:b], "sd": sd[:b], "z": z[:b], "ge": ge[:b]}
            out["node"][s0:s0 + b] = got
            out["iters"][s0:s0 + b] = iters.reshape(b, R)[:, 0].cpu().numpy()
            for f, x in cols.items():
                v = torch.gather(x, 1, at).cpu().numpy()
                out[f][s0:s0 + b] = np.where(got >= 0, v, -1 if f == "ge" else np.nan)
        out["emp_p"] = np.where(out["node"] >= 0, (1 + out["ge"]) / (n_random + 1.0), np.nan)
        out["members"] = sets
        return out
