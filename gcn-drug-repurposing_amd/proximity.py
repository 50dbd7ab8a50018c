"""Drug-disease network proximity (Guney et al. 2016, "Network-based in silico drug efficacy screening") on the device: what
method/test_proximity.py computes through toolbox.wrappers.calculate_proximity, one pair at a time, here for a whole table at once.

Host code is setup only: the loaders, the largest connected component (LCC), the degree bins and the set tables.  The all-pairs hop
distances, the degree-matched random sets, the per-set statistics and all five measures with their z-scores run in csrc/proximity.hip;
no CPU fallback: without the library or a GPU this raises.
"""
from __future__ import annotations

import pickle
import re

import numpy as np

MEASURES = ("closest", "shortest", "kernel", "center", "separation")
MEASURE_BIT = {m: 1 << i for i, m in enumerate(MEASURES)}
FIELDS = ("d", "m", "s", "z", "pval")
DEFAULT_MAX_BYTES = 1 << 30      # budget of the uint8 distance matrix (N <= 32768)
MAX_DISEASE_SET = 4096           # to-side set size the scoring kernel holds in LDS


class ProximityError(ValueError):
    pass


# ---- loaders ------------------------------------------------------------------------------------------------------------------------

class _SetPickle(pickle.Unpickler):
    """the drug target pickle is Python 2 protocol 0 ({DrugBank id: set(gene id)}): only the builtin set and dict may be named"""
    ALLOWED = {("__builtin__", "set"): set, ("builtins", "set"): set, ("__builtin__", "dict"): dict, ("builtins", "dict"): dict}

    def find_class(self, module, name):
        try:
            return self.ALLOWED[(module, name)]
        except KeyError:
            raise pickle.UnpicklingError(f"global {module}.{name} is not allowed in a drug target pickle (only set and dict)") from None


def load_drug_targets(path):
    """{drug id: set of gene ids (str)} from drug_to_geneids.pcl.all"""
    with open(path, "rb") as f:
        d = _SetPickle(f, encoding="latin1").load()
    if not isinstance(d, dict):
        raise ProximityError(f"{path}: not a dict of drug -> gene set")
    return {str(k): {str(g) for g in v} for k, v in d.items()}


def disease_key(name):
    """the proximity tables' disease column: the name lower-cased, every run of non-alphanumerics replaced by '.'"""
    return re.sub(r"[^0-9a-z]+", ".", name.lower())


def load_disease_genes(path):
    """{disease key: set of gene ids (str)} from disease_genes.tsv (`<empty>\\t<name>\\t<gene>...`)"""
    out = {}
    with open(path) as f:
        for line in f:
            p = line.rstrip("\n").split("\t")
            if len(p) < 2 or not p[1]:
                continue
            out.setdefault(disease_key(p[1]), set()).update(g for g in p[2:] if g)
    return out


def read_table_pairs(path):
    """(group, disease) columns of a proximity .dat table, in row order"""
    with open(path) as f:
        head = f.readline().split()
        gi, di = head.index("group"), head.index("disease")
        return [(p[gi], p[di]) for p in (line.split() for line in f) if p]


# ---- the network --------------------------------------------------------------------------------------------------------------------

class Network:
    """the LCC of an undirected gene network: `names` (LCC order = order of first appearance), `index`, the symmetric CSR without self
    loops (`rowptr`, `col`, columns ascending) and the networkx degree (a self loop adds 2)"""

    def __init__(self, src, dst, names):
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        n_all = len(names)
        loop = np.zeros(n_all, bool)
        loop[src[src == dst]] = True
        keep = src != dst
        a, b = np.concatenate([src[keep], dst[keep]]), np.concatenate([dst[keep], src[keep]])
        key = np.unique(a * n_all + b)
        a, b = key // n_all, key % n_all
        comp = _components(n_all, a, b)
        big = np.bincount(comp).argmax() if n_all else 0
        lcc = np.flatnonzero(comp == big)
        remap = np.full(n_all, -1, np.int64)
        remap[lcc] = np.arange(len(lcc))
        m = (remap[a] >= 0) & (remap[b] >= 0)
        a, b = remap[a[m]], remap[b[m]]
        self.n = len(lcc)
        self.n_total = n_all
        self.names = [names[i] for i in lcc]
        self.index = {g: i for i, g in enumerate(self.names)}
        order = np.lexsort((b, a))
        self.col = b[order].astype(np.int32)
        self.rowptr = np.zeros(self.n + 1, np.int32)
        np.cumsum(np.bincount(a, minlength=self.n), out=self.rowptr[1:])
        self.degree = (np.diff(self.rowptr) + 2 * loop[lcc]).astype(np.int64)

    def node_set(self, genes):
        """LCC node indices of the genes that are in the LCC, ascending"""
        return np.array(sorted(self.index[g] for g in genes if g in self.index), np.int32)


def _components(n, a, b):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    g = sp.csr_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n))
    return connected_components(g, directed=False)[1]


def read_network(path):
    """network.sif (`gene rel gene`), read as undirected by embio.read_edgelist -> Network (the LCC)"""
    from .embio import read_edgelist
    src, dst, _, names = read_edgelist(str(path))
    return Network(src, dst, names)


def degree_bins(degree, min_bin_size=100):
    """the toolbox's get_degree_binning: distinct degrees ascending, consecutive groups merged until a bin holds >= min_bin_size nodes, a
    smaller remainder merged into the previous bin -> list of node-index arrays (ascending)"""
    degree = np.asarray(degree)
    values = np.unique(degree)
    bins, i = [], 0
    while i < len(values):
        val = list(np.flatnonzero(degree == values[i]))
        while len(val) < min_bin_size:
            i += 1
            if i == len(values):
                break
            val += list(np.flatnonzero(degree == values[i]))
        i += 1
        if len(val) < min_bin_size and bins:
            bins[-1] = bins[-1] + val
        else:
            bins.append(val)
    return [np.array(sorted(b), np.int32) for b in bins]


def bin_tables(bins, n):
    """(node_bin [n], bin_ptr, bin_nodes) of degree_bins"""
    node_bin = np.full(n, -1, np.int32)
    for k, b in enumerate(bins):
        node_bin[b] = k
    bin_ptr = np.zeros(len(bins) + 1, np.int32)
    bin_ptr[1:] = np.cumsum([len(b) for b in bins])
    return node_bin, bin_ptr, np.concatenate(bins).astype(np.int32)


def random_set_table(call, what, n, dev, node_sets, side, n_random, seed, bins):
    """the set table of `node_sets` (sample 0 = the set, samples 1.. its degree-matched random sets) on device `dev`, by `call`:
    gss_prox_random_sets behind its handle or gss_random_sets behind n, both taking (side, n_sets, set_ptr, ...) from there on
    -> (nodes [n_sets, R, max_size], sizes [n_sets, R]) device int32"""
    import torch
    from . import _lib
    sets = [np.asarray(s, np.int32) for s in node_sets]
    max_size = max(1, max(len(s) for s in sets))
    ptr = np.zeros(len(sets) + 1, np.int32)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    flat = np.concatenate(sets + [np.zeros(1, np.int32)]).astype(np.int32)
    node_bin, bin_ptr, bin_nodes = (torch.from_numpy(x).to(dev) for x in bin_tables(bins, n))
    d_ptr, d_flat = torch.from_numpy(ptr).to(dev), torch.from_numpy(flat).to(dev)
    R = n_random + 1
    nodes = torch.full((len(sets), R, max_size), -1, dtype=torch.int32, device=dev)
    sizes = torch.empty((len(sets), R), dtype=torch.int32, device=dev)
    _lib.check(call(side, len(sets), _lib.ptr(d_ptr), _lib.ptr(d_flat), max_size, _lib.ptr(node_bin), _lib.ptr(bin_ptr), _lib.ptr(bin_nodes),
                    n_random, _lib.seed64(seed), _lib.ptr(nodes), _lib.ptr(sizes), _lib.current_stream()), what)
    return nodes, sizes


# ---- the device engine --------------------------------------------------------------------------------------------------------------

class ProximityEngine:
    """owns the device distance matrix of `network` (a Network) and scores set pairs against it"""

    def __init__(self, network, max_bytes=DEFAULT_MAX_BYTES):
        import ctypes as C

        import torch
        from . import _lib
        self.lib = _lib.load()
        self.net = network
        self._torch = torch
        self._dev = torch.device("cuda")
        self._rowptr = torch.from_numpy(network.rowptr).to(self._dev)
        self._col = torch.from_numpy(network.col if len(network.col) else np.zeros(1, np.int32)).to(self._dev)
        h = C.c_void_p()
        _lib.check(self.lib.gss_prox_create(C.byref(h), network.n, _lib.ptr(self._rowptr), _lib.ptr(self._col), int(max_bytes),
                                            _lib.current_stream()), "gss_prox_create")
        self._h = h
        self.diameter = self.lib.gss_prox_diameter(h)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.gss_prox_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def distances(self):
        """the device matrix as a torch uint8 [n, n] tensor (a copy)"""
        n = self.net.n
        out = self._torch.empty((n, n), dtype=self._torch.uint8, device=self._dev)
        from . import _lib
        _lib.check(self.lib.gss_memcpy_d2d(_lib.ptr(out), self.lib.gss_prox_distances(self._h), n * n, _lib.current_stream()),
                   "gss_memcpy_d2d")
        return out

    def set_table(self, node_sets, side, n_random, seed, bins):
        """random sets of every set (sample 0 = the set) -> (nodes [n_sets, R, max_size], sizes [n_sets, R]) device int32"""
        return random_set_table(lambda *args: self.lib.gss_prox_random_sets(self._h, *args), "gss_prox_random_sets", self.net.n, self._dev,
                                node_sets, side, n_random, seed, bins)

    def set_stats(self, nodes, sizes, centres=True):
        from . import _lib
        torch = self._torch
        n_sets, R, max_size = nodes.shape
        inner = torch.empty((n_sets, R), dtype=torch.float64, device=self._dev)
        cen = torch.full_like(nodes, -1) if centres else None
        ncen = torch.empty_like(sizes) if centres else None
        _lib.check(self.lib.gss_prox_set_stats(self._h, n_sets, R, max_size, _lib.ptr(nodes), _lib.ptr(sizes), _lib.ptr(inner),
                                               _lib.ptr(cen), _lib.ptr(ncen), _lib.current_stream()), "gss_prox_set_stats")
        return inner, cen, ncen

    def score(self, from_sets, to_sets, pairs=None, measures=("closest",), n_random=1000, seed=452456, min_bin_size=100):
        """from_sets / to_sets: lists of gene-id collections (intersected with the LCC here).  pairs: None for all len(from_sets) x
        len(to_sets) pairs (q = i * len(to_sets) + j), else a sequence of (from index, to index).  Returns {measure: {"d", "z", "m", "s",
        "pval": fp64 [n_pairs] (NaN where a set is empty after the LCC intersection), "n_from", "n_to": int [n_pairs]}}."""
        import ctypes as C

        from . import _lib
        torch = self._torch
        measures = tuple(measures)
        bad = [m for m in measures if m not in MEASURE_BIT]
        if bad or not measures:
            raise ProximityError(f"unknown measure(s) {bad or measures}: choose from {', '.join(MEASURES)}")
        if int(n_random) < 2:
            raise ProximityError(f"n_random={n_random}: need at least 2 random samples for a standard deviation")
        if int(min_bin_size) < 1:
            raise ProximityError(f"min_bin_size={min_bin_size} must be >= 1")
        if not from_sets or not to_sets:
            raise ProximityError("score: from_sets and to_sets must not be empty")
        n_random = int(n_random)
        fs = [self.net.node_set(s) for s in from_sets]
        ts = [self.net.node_set(s) for s in to_sets]
        big = max(len(s) for s in ts)
        if big > MAX_DISEASE_SET:
            raise ProximityError(f"a to-set has {big} genes in the LCC; at most {MAX_DISEASE_SET} are supported")
        if pairs is None:
            n_pairs, pf, pt = len(fs) * len(ts), None, None
            pi, pj = np.divmod(np.arange(n_pairs), len(ts))
        else:
            pr = np.asarray(pairs, np.int64).reshape(-1, 2)
            if len(pr) and (pr[:, 0].min() < 0 or pr[:, 0].max() >= len(fs) or pr[:, 1].min() < 0 or pr[:, 1].max() >= len(ts)):
                raise ProximityError("score: a pair names a set index out of range")
            n_pairs, pi, pj = len(pr), pr[:, 0], pr[:, 1]
            pf = torch.from_numpy(pi.astype(np.int32)).to(self._dev)
            pt = torch.from_numpy(pj.astype(np.int32)).to(self._dev)
        bins = degree_bins(self.net.degree, min_bin_size)
        fn, fsz = self.set_table(fs, 0, n_random, seed, bins)
        tn, tsz = self.set_table(ts, 1, n_random, seed, bins)
        want_sep = "separation" in measures
        f_inner = self.set_stats(fn, fsz, centres=False)[0] if want_sep else torch.zeros(fsz.shape, dtype=torch.float64, device=self._dev)
        t_inner, t_cen, t_ncen = self.set_stats(tn, tsz, centres="center" in measures)
        mask = sum(MEASURE_BIT[m] for m in measures)
        F = _lib.ProxSets(len(fs), fn.shape[2], _lib.ptr(fn), _lib.ptr(fsz), _lib.ptr(f_inner), None, None)
        T = _lib.ProxSets(len(ts), tn.shape[2], _lib.ptr(tn), _lib.ptr(tsz), _lib.ptr(t_inner), _lib.ptr(t_cen), _lib.ptr(t_ncen))
        out = torch.empty((max(n_pairs, 1), len(MEASURES), len(FIELDS)), dtype=torch.float64, device=self._dev)
        _lib.check(self.lib.gss_prox_score(self._h, C.byref(F), C.byref(T), n_random + 1, n_pairs, _lib.ptr(pf), _lib.ptr(pt), mask,
                                           _lib.ptr(out), _lib.current_stream()), "gss_prox_score")
        res = out[:n_pairs].cpu().numpy()
        nf = np.array([len(s) for s in fs], np.int64)[pi]
        nt = np.array([len(s) for s in ts], np.int64)[pj]
        return {m: dict({f: res[:, MEASURES.index(m), k].copy() for k, f in enumerate(FIELDS)}, n_from=nf, n_to=nt) for m in measures}
