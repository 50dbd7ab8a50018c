"""node2vec input embeddings on the device: multiscale/openne/node2vec.py:7-47 (Node2vec) with its two stages as HIP kernels --
second-order biased walks (csrc/walk.hip, walker.py:58-207) and skip-gram with negative sampling (csrc/sgns.hip, gensim 3.x Word2Vec
as node2vec.py:34 calls it: sg=1, hs=0, negative=5, sample=1e-3, min_count=0, alpha 0.025 -> 1e-4, iter=5, ns_exponent 0.75).

Host code here is setup only (argument checks, the per-iteration start order, gensim's two tables from the device token counts); no
CPU fallback: without the library or a GPU this raises.  Rows are in graph order (MsiGraph.names / the CSR's row order), the order the
trainer's input, its output graph_embs.txt and every consumer share.
"""
from __future__ import annotations

import math
import time

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
TAG_PERM = 2
DOMAIN = 2 ** 31 - 1      # gensim make_cum_table
MAX_EXP = 6.0
DIMS = (64, 128, 256, 512)


def _mix64(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _rng_key(seed, tag, a, b, c):
    """csrc/counter_rng.h rng_key on uint64 arrays (wrapping arithmetic)"""
    k = np.uint64(GOLDEN)
    u = lambda v: np.asarray(v, dtype=np.uint64)  # noqa: E731
    with np.errstate(over="ignore"):
        h = _mix64(u(seed) + u(tag) + k)
        h = _mix64(h + u(a) + k)
        h = _mix64(h + u(b) + k)
        return _mix64(h + u(c) + k)


def start_nodes(n, num_walks, seed):
    """iteration r starts one walk at every node, in the order of the counter-RNG keys (seed, r, node) -- the reference's
    random.shuffle(nodes) per iteration (walker.py:95-104) -> int32 [num_walks * n]"""
    nodes = np.arange(n, dtype=np.uint64)
    out = np.empty(num_walks * n, np.int32)
    for r in range(num_walks):
        keys = _rng_key(seed, TAG_PERM, np.uint64(r), nodes, np.uint64(0))
        out[r * n:(r + 1) * n] = np.argsort(keys, kind="stable")
    return out


def sgns_tables(counts, sample=1e-3, ns_exponent=0.75):
    """gensim 3.x Word2VecVocab: the negative-sampling table (make_cum_table) and the per-word downsampling threshold
    (prepare_vocab: sample_int = round(keep probability * 2^32)) from the token counts, vocabulary in graph order"""
    counts = np.asarray(counts, np.int64)
    pw = counts.astype(np.float64) ** ns_exponent
    total_pow = float(np.sum(pw))
    cum_table = np.round(np.cumsum(pw) / total_pow * DOMAIN).astype(np.uint32)
    retain_total = float(counts.sum())
    if sample == 0 or retain_total == 0:
        prob = np.ones(len(counts))
    elif sample < 1.0:
        threshold = sample * retain_total
        with np.errstate(divide="ignore", invalid="ignore"):
            prob = (np.sqrt(counts / threshold) + 1) * (threshold / counts)
    else:
        threshold = float(int(sample * (3 + math.sqrt(5)) / 2))
        with np.errstate(divide="ignore", invalid="ignore"):
            prob = (np.sqrt(counts / threshold) + 1) * (threshold / counts)
    prob = np.where(np.isfinite(prob) & (prob < 1.0), prob, 1.0)
    sample_int = np.round(prob * 2.0 ** 32).astype(np.int64)
    return cum_table, sample_int


def check_walk_args(p, q, walk_length, num_walks):
    for name, v in (("p", p), ("q", q)):
        if not (isinstance(v, (int, float, np.floating)) and math.isfinite(v) and v > 0):
            raise ValueError(f"node2vec: {name}={v!r} must be positive and finite (the return / in-out parameters divide the weights)")
    if int(walk_length) < 1:
        raise ValueError(f"node2vec: walk_length={walk_length} must be >= 1")
    if int(num_walks) < 1:
        raise ValueError(f"node2vec: num_walks={num_walks} must be >= 1")


def prepare_csr(adj):
    """-> scipy CSR fp64 with duplicates summed and columns sorted; refuses (by name) weights that are not positive and finite"""
    import scipy.sparse as sp
    a = sp.csr_matrix(adj, dtype=np.float64)
    a.sum_duplicates()
    a.sort_indices()
    if a.shape[0] != a.shape[1]:
        raise ValueError(f"node2vec: the adjacency must be square, got {a.shape}")
    bad = ~(np.isfinite(a.data) & (a.data > 0))
    if bad.any():
        e = int(np.flatnonzero(bad)[0])
        row = int(np.searchsorted(a.indptr, e, side="right") - 1)
        raise ValueError(f"node2vec: edge weight {a.data[e]!r} of edge {row} -> {int(a.indices[e])} is not positive and finite")
    return a


def random_walks(adj, num_walks, walk_length, p=1.0, q=1.0, seed=0, device="cuda"):
    """-> (walks int32 [num_walks * N, walk_length] (unused tail -1), lengths int32 [num_walks * N]) as device tensors"""
    import torch

    from . import _lib
    check_walk_args(p, q, walk_length, num_walks)
    a = prepare_csr(adj)
    n = a.shape[0]
    lib = _lib.load()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.GssError("node2vec walks run on the GPU only (walk.hip); there is no CPU fallback")
    rowptr = torch.from_numpy(a.indptr.astype(np.int32)).to(dev)
    col = torch.from_numpy(a.indices.astype(np.int32)).to(dev)
    val = torch.from_numpy(a.data).to(dev)
    cum = torch.empty(max(a.nnz, 1), dtype=torch.float64, device=dev)
    starts = torch.from_numpy(start_nodes(n, int(num_walks), seed)).to(dev)
    n_walks = int(num_walks) * n
    walks = torch.empty((n_walks, int(walk_length)), dtype=torch.int32, device=dev)
    lengths = torch.empty(n_walks, dtype=torch.int32, device=dev)
    stream = _lib.current_stream()
    if a.nnz:
        _lib.check(lib.gss_walk_prefix(n, _lib.ptr(rowptr), _lib.ptr(val), _lib.ptr(cum), stream), "gss_walk_prefix")
    _lib.check(lib.gss_node2vec_walks(n, _lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), _lib.ptr(cum), n_walks, _lib.ptr(starts),
                                      int(walk_length), float(p), float(q), _lib.seed64(seed), _lib.ptr(walks), _lib.ptr(lengths),
                                      stream), "gss_node2vec_walks")
    return walks, lengths


def token_counts(walks, lengths, n):
    import torch

    from . import _lib
    counts = torch.zeros(n, dtype=torch.int64, device=walks.device)
    _lib.check(_lib.load().gss_sgns_counts(walks.shape[0], walks.shape[1], _lib.ptr(walks), _lib.ptr(lengths), _lib.ptr(counts),
                                           _lib.current_stream()), "gss_sgns_counts")
    return counts


def train_sgns(walks, lengths, n, dim=128, window=10, epochs=5, negative=5, sample=1e-3, alpha=0.025, min_alpha=1e-4, seed=0,
               concurrency=None, ns_exponent=0.75):
    """skip-gram negative sampling over the walks (one sentence per walk) -> (syn0, syn1neg) fp32 device tensors [n, dim]"""
    import torch

    from . import _lib
    if dim not in DIMS:
        raise ValueError(f"node2vec: dim={dim} unsupported by the SGNS kernel (one of {DIMS})")
    if not 1 <= negative <= 63:
        raise ValueError(f"node2vec: negative={negative} must be in [1, 63] (hs=0 needs negative sampling)")
    if window < 1 or epochs < 1:
        raise ValueError(f"node2vec: window={window} and epochs={epochs} must be >= 1")
    lib = _lib.load()
    dev = walks.device
    stream = _lib.current_stream()
    counts = token_counts(walks, lengths, n).cpu().numpy()
    cum_table, sample_int = sgns_tables(counts, sample, ns_exponent)
    d_cum = torch.from_numpy(cum_table.view(np.int32)).to(dev)
    d_keep = torch.from_numpy(sample_int).to(dev)
    syn0 = torch.empty((n, dim), dtype=torch.float32, device=dev)
    syn1 = torch.empty((n, dim), dtype=torch.float32, device=dev)
    _lib.check(lib.gss_sgns_init(n, dim, _lib.seed64(seed), _lib.ptr(syn0), _lib.ptr(syn1), stream), "gss_sgns_init")
    if concurrency is None:
        concurrency = lib.gss_sgns_default_concurrency()
        if concurrency < 1:
            _lib.check(concurrency, "gss_sgns_default_concurrency")
    desc = _lib.SgnsDesc(n=n, d=dim, walk_length=walks.shape[1], window=int(window), negative=int(negative), epochs=int(epochs),
                         n_walks=walks.shape[0], walks=_lib.ptr(walks), lengths=_lib.ptr(lengths), cum_table=_lib.ptr(d_cum),
                         sample_int=_lib.ptr(d_keep), cum_last=int(cum_table[-1]), alpha=float(alpha), min_alpha=float(min_alpha),
                         seed=_lib.seed64(seed), concurrency=int(concurrency))
    for ep in range(int(epochs)):
        _lib.check(lib.gss_sgns_epoch(desc, ep, _lib.ptr(syn0), _lib.ptr(syn1), stream), "gss_sgns_epoch")
    return syn0, syn1


def _graph_csr(graph, names):
    if hasattr(graph, "to_csr"):          # msi.MsiGraph
        adj, gnames, _ = graph.to_csr()
        return adj, list(gnames)
    if isinstance(graph, tuple) and len(graph) == 2:
        return graph[0], list(graph[1])
    if names is None:
        raise ValueError("node2vec: a CSR graph needs its node names (names=[...] or graph=(csr, names))")
    return graph, list(names)


class Node2vec:
    """OpenNE's Node2vec(graph, path_length, num_paths, dim, p, q, dw, **word2vec kwargs) -> .vectors (name -> vector, graph order),
    .save_embeddings(path).  graph: an msi.MsiGraph (weighted first), a (scipy CSR, names) pair, or a CSR with names=."""

    def __init__(self, graph, path_length, num_paths, dim, p=1.0, q=1.0, dw=False, window=10, epochs=5, negative=5, sample=1e-3,
                 seed=0, concurrency=None, names=None, alpha=0.025, min_alpha=1e-4, workers=None, device="cuda"):
        if dw:
            raise ValueError("node2vec: dw=True (DeepWalk with hierarchical softmax) is not supported; this build does node2vec "
                             "with negative sampling only")
        check_walk_args(p, q, path_length, num_paths)
        if dim not in DIMS:
            raise ValueError(f"node2vec: dim={dim} unsupported by the SGNS kernel (one of {DIMS})")
        adj, self.names = _graph_csr(graph, names)
        adj = prepare_csr(adj)
        if adj.shape[0] != len(self.names):
            raise ValueError(f"node2vec: {adj.shape[0]} rows but {len(self.names)} names")
        import torch
        self.size = int(dim)
        t0 = time.perf_counter()
        walks, lengths = random_walks(adj, num_paths, path_length, p, q, seed, device)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        syn0, _ = train_sgns(walks, lengths, adj.shape[0], dim, window, epochs, negative, sample, alpha, min_alpha, seed, concurrency)
        self.embeddings = syn0.cpu().numpy()
        t2 = time.perf_counter()
        self.timings = {"walks_s": t1 - t0, "sgns_s": t2 - t1}
        self.vectors = {name: self.embeddings[i] for i, name in enumerate(self.names)}

    def save_embeddings(self, filename):
        """node2vec.py:40-47: '<N> <dim>' then '<node> v1 ... vd' per node, graph order"""
        from .embio import write_embs
        write_embs(filename, self.names, self.embeddings)
