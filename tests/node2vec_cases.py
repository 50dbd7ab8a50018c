"""Inputs of the op-by-op tests of the node2vec kernels (tests/test_node2vec_mirror.py on the CPU, tests/test_gpu_node2vec_ops.py on the
GPU): small, built from seeded numpy, each with the property it exists for (`why`).  tests/test_node2vec_mirror.py asserts those
properties on the mirror alone -- a seed that loses one fails there, not on the GPU.

Walk cases (walk_case(name) -> adjacency, walks per node, length, p, q, seed):
  fallback_*   the suite's graph with sinks at (p, q) whose acceptance probability is 1/16, 1/64 and 1e-6: the direct draw after 64
               refused candidates (walk.hip's last branch), which the three (p, q) of tests/test_gpu_node2vec.py never reach;
  tiny_*       12 nodes, one self-loop, one sink: few enough states that 18,000 walks test every transition's frequency against the law
               from its definition (exact_transitions) at the same extreme (p, q);
  hub_ties_*   a row of 5,200 entries with weights over 18 decades: its fp64 prefix sums hold runs of equal values, and the binary
               search and the direct draw's scan cross them;
  len_1, len_2, walks_255 / 256 / 257, single_self_loop, single_no_edge   the launch and length edges.

SGNS cases (sgns_case(name)): a vocabulary of 24 to 26 nodes, start rows randn * s / sqrt(d) (s = 1: unit-scale rows, on which one
missed or wrong pair update moves a value by 1e-3 to 1e-1), sentences from the mirror's walks on a 24-node digraph with a sink or
written by hand, gensim's negative table from the token counts and every token kept unless the case says otherwise.  The case list
with each case's reason is SGNS_CASES; `ABLATION_CASE` names, for every wrong rule of node2vec_mirror.ABLATIONS, the case that shows it.
Mirror results are computed once per (case, dtype, ablation) and shared; treat every array as read-only."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import node2vec_mirror as M

KEEP_ALL = 2 ** 32            # gensim's sample_int of a word that is never dropped: every uint32 draw is <= it


def sinks_graph():
    """random weighted digraph with sink rows (no out-edges), self-loops and isolated nodes"""
    rng = np.random.RandomState(7)
    n = 300
    a = sp.random(n, n, density=0.03, random_state=rng, format="lil")
    for i in range(0, n, 17):
        a[i, i] = 0.5
    for i in range(3, n, 23):
        a[i, :] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    a.data = rng.gamma(2.0, 1.0, a.nnz) + 1e-3
    return a


def random_digraph(n, density, seed, self_loop=None, sink=None, sink_in_scale=1.0):
    """gamma-weighted random digraph; row `sink` emptied (its in-edges scaled by sink_in_scale), a self-loop on `self_loop`"""
    rng = np.random.RandomState(seed)
    a = (rng.rand(n, n) < density) * (rng.gamma(2.0, 1.0, (n, n)) + 1e-3)
    np.fill_diagonal(a, 0.0)
    for i in range(n):                       # no accidental sinks: every row keeps an edge
        if not a[i].any():
            a[i, (i + 1) % n] = 1.0
    if self_loop is not None:
        a[self_loop, self_loop] = 0.7
    if sink is not None:
        a[sink, :] = 0.0
        a[:, sink] *= sink_in_scale
        if not a[:, sink].any():
            a[(sink + 1) % n, sink] = sink_in_scale
    return sp.csr_matrix(a)


@functools.lru_cache(maxsize=None)
def tiny_digraph():
    return random_digraph(12, 0.35, seed=21, self_loop=4, sink=9)


HUB_N, HUB_DEGREE, HUB = 5400, 5200, 0


@functools.lru_cache(maxsize=None)
def hub_graph():
    """a ring (i <-> i + 1, weight 1) with node 0 joined to 5,200 nodes by weights 10^U(-9, 9) in random order; every 8th node
    leads back to the hub, so the hub's row is left from many different previous nodes"""
    rng = np.random.RandomState(31)
    n = HUB_N
    ring = np.arange(n)
    rows = [ring, ring]
    cols = [(ring + 1) % n, (ring - 1) % n]
    vals = [np.ones(n), np.ones(n)]
    to = np.sort(rng.choice(np.arange(2, n - 1), HUB_DEGREE, replace=False))      # besides the hub's two ring edges
    rows.append(np.full(HUB_DEGREE, HUB)); cols.append(to); vals.append(10.0 ** rng.uniform(-9, 9, HUB_DEGREE))
    back = np.arange(8, n - 1, 8)
    rows.append(back); cols.append(np.full(len(back), HUB)); vals.append(np.full(len(back), 2.0))
    a = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    a.sum_duplicates()
    a.sort_indices()
    return a


def _walk(name, why, adj, nw, L, p, q, seed=123):
    return types.SimpleNamespace(name=name, why=why, adj=adj, nw=nw, L=L, p=p, q=q, seed=seed)


_WALK_CASES = [
    _walk("fallback_q16", "acceptance 1/16: some steps refuse 64 candidates and draw directly", sinks_graph, 4, 16, 1.0, 16.0),
    _walk("fallback_q64", "acceptance 1/64: about one step in eight draws directly", sinks_graph, 4, 16, 1.0, 64.0),
    _walk("fallback_p1e-6", "acceptance 1e-6 for all but the way back: most steps draw directly", sinks_graph, 4, 16, 1e-6, 1.0),
    _walk("tiny_q64", "12 nodes: every state's frequencies against the exact law, direct draws at q = 64", tiny_digraph, 1500, 16, 1.0, 64.0),
    _walk("tiny_p1e-6", "12 nodes: the exact law where nearly every later step is a direct draw", tiny_digraph, 1500, 16, 1e-6, 1.0),
    _walk("tiny_q16", "12 nodes: the exact law where rejection and the direct draw mix", tiny_digraph, 1500, 16, 1.0, 16.0),
    _walk("hub_ties_pq", "binary search over prefix sums with runs of equal values (5,200 weights over 18 decades)", hub_graph, 2, 8, 4.0, 0.5),
    _walk("hub_ties_q64", "the direct draw's sequential sum and scan over the same row", hub_graph, 1, 8, 1.0, 64.0),
    _walk("len_1", "walk_length 1: lengths all 1, only column 0 written", tiny_digraph, 3, 1, 1.0, 16.0),
    _walk("len_2", "walk_length 2: only the first-order step runs", tiny_digraph, 3, 2, 1.0, 16.0),
    _walk("walks_255", "255 walks: one block, its last thread idle", lambda: random_digraph(85, 0.08, 41, self_loop=2, sink=7), 3, 12, 1.0, 16.0),
    _walk("walks_256", "256 walks: exactly one block", lambda: random_digraph(128, 0.06, 42, self_loop=2, sink=7), 2, 12, 1.0, 16.0),
    _walk("walks_257", "257 walks: a second block with one live thread", lambda: random_digraph(257, 0.03, 43, self_loop=2, sink=7), 1, 12, 1.0, 16.0),
    _walk("single_self_loop", "one node with a self-loop: every step goes back to prev", lambda: sp.csr_matrix(np.array([[2.5]])), 3, 5, 0.5, 2.0),
    _walk("single_no_edge", "one node, no edge at all: an empty CSR, lengths 1", lambda: sp.csr_matrix((1, 1)), 3, 5, 0.5, 2.0),
]
WALK_CASES = [c.name for c in _WALK_CASES]
FALLBACK_CASES = [n for n in WALK_CASES if n.startswith("fallback_")]
TINY_CASES = [n for n in WALK_CASES if n.startswith("tiny_")]
SUITE_PQ = [(1.0, 1.0), (0.25, 0.25), (4.0, 0.5)]           # the (p, q) of tests/test_gpu_node2vec.py


def walk_case(name):
    return next(c for c in _WALK_CASES if c.name == name)


@functools.lru_cache(maxsize=None)
def mirror_walks(name):
    """-> (walks, lengths, stats) of the mirror on the case"""
    c = walk_case(name)
    stats = {}
    w, ln = M.walks(c.adj(), c.nw, c.L, c.p, c.q, c.seed, stats=stats)
    return w, ln, stats


# ------------------------------------------------------------------------------------------------------------------------ SGNS
VOCAB = 24


@functools.lru_cache(maxsize=None)
def vocab_graph():
    """24-node digraph whose node 23 is a sink that is entered rarely: most walks run to their full length, some end early"""
    return random_digraph(VOCAB, 0.3, seed=5, self_loop=3, sink=23, sink_in_scale=0.02)


@functools.lru_cache(maxsize=None)
def _sentences(L, nw=1, seed=77):
    return M.walks(vocab_graph(), nw, L, 1.0, 1.0, seed)


def _rows(rng, n, d, s=1.0):
    return (rng.randn(n, d) * (s / np.sqrt(d))).astype(np.float32)


def _case(name, why, walks, lengths, n=VOCAB, d=64, window=3, negative=5, epochs=1, first_epoch=0, alpha=0.025, min_alpha=1e-4, seed=0,
          s=1.0, rows_seed=None, cum_table=None, sample_int=None, syn0=None, syn1=None, moved_min=1e-2, **extra):
    walks = np.ascontiguousarray(walks, np.int32)
    lengths = np.ascontiguousarray(lengths, np.int32)
    valid = np.arange(walks.shape[1])[None, :] < lengths[:, None]
    assert (lengths >= 1).all() and (lengths <= walks.shape[1]).all() and ((walks[valid] >= 0) & (walks[valid] < n)).all(), name
    rng = np.random.RandomState(seed + 1000 if rows_seed is None else rows_seed)
    r0, r1 = _rows(rng, n, d, s), _rows(rng, n, d, s)
    if cum_table is None:
        cum_table = M.tables(np.bincount(walks[valid], minlength=n))[0]
    if sample_int is None:
        sample_int = np.full(n, KEEP_ALL, np.int64)
    return types.SimpleNamespace(name=name, why=why, walks=walks, lengths=lengths, n=n, d=d, window=window, negative=negative, epochs=epochs,
                                 first_epoch=first_epoch, alpha=alpha, min_alpha=min_alpha, seed=seed, syn0=r0 if syn0 is None else syn0,
                                 syn1=r1 if syn1 is None else syn1, cum_table=np.asarray(cum_table, np.uint32),
                                 sample_int=np.asarray(sample_int, np.int64), moved_min=moved_min, **extra)


def keep_draw(seed, epoch, token):
    return int(M.u32(M.rng_key(seed, M.TAG_KEEP, epoch, token, 0)))


PARTITION_S = 10007
SGNS_CASES = {
    "dims_64": "VPL 1: one float per lane",
    "dims_128": "VPL 2, on unit-scale rows",
    "dims_256": "VPL 4",
    "dims_512": "VPL 8",
    "long_80": "walk_length 80: a second pass of the 64-lane ballot compaction, a third of the tokens dropped",
    "long_130": "walk_length 130: three passes, kept and dropped tokens on both sides of positions 64 and 128",
    "window_1": "window 1: the reduced window r % 1 is always 0",
    "window_wider_than_sentence": "window 200 at walk_length 20: lo and hi clamp at the sentence's ends",
    "negative_1": "one negative: lane 1 alone draws",
    "negative_63": "63 negatives: lanes 1..63 draw, the lane bound lane <= negative",
    "f_skip": "rows of scale 6: hundreds of targets with |f| >= 6, skipped",
    "keep_boundary": "a token whose keep draw equals its sample_int (kept: <=) and one whose draw is sample_int + 1 (dropped)",
    "table_ties": "cum_table = 1..n: every draw r >= 1 equals a table entry (bisect_left, not bisect_right)",
    "epochs_3_e0": "epoch 0 of 3",
    "epochs_3_e1": "epoch 1 of 3 alone, from the fp32 mirror's state after epoch 0: the epoch term of alpha and of the draws' keys",
    "epochs_3_e2": "epoch 2 of 3 alone, from the state after epoch 1",
    "min_alpha_clamp": "min_alpha 0.03 above alpha 0.025: the clamp decides alpha in every sentence (epoch 1 of 3)",
    "degenerate_sentences": "sentences of 1 and 2 tokens, some nodes always dropped: kept lengths 0, 1 and 2",
    "partition": "10,007 two-token sentences over distinct nodes, syn0 = 0: a result independent of the order of the sentences",
}
SERIAL_CASES = list(SGNS_CASES)
# the wrong rule -> the case on which it moves the fp64 result by >= 100 x 8 x d32(case) (tests/test_node2vec_mirror.py)
ABLATION_CASE = {"keep_lt": "keep_boundary", "bisect_right": "table_ties", "tail_tokens": "long_80", "window_hi": "window_1",
                 "last_negative": "negative_1", "neg_eq_center": "dims_64", "alpha_epoch": "epochs_3_e1", "f_skip": "f_skip"}


@functools.lru_cache(maxsize=None)
def sgns_case(name):
    why = SGNS_CASES[name]
    if name.startswith("dims_"):
        w, ln = _sentences(20)
        return _case(name, why, w, ln, d=int(name[5:]), seed=11)
    if name.startswith("long_"):
        L = int(name[5:])
        w, ln = _sentences(L)
        w, ln = w[:12], ln[:12]
        keep = np.full(VOCAB, KEEP_ALL, np.int64)
        keep[::2] = 2 ** 32 // 3                    # every other node kept one time in three: a third of the tokens go
        return _case(name, why, w, ln, sample_int=keep, seed=12)
    if name == "window_1":
        w, ln = _sentences(20)
        return _case(name, why, w, ln, window=1, seed=13)
    if name == "window_wider_than_sentence":
        w, ln = _sentences(20)
        return _case(name, why, w[:12], ln[:12], window=200, seed=14)
    if name == "negative_1":
        w, ln = _sentences(20)
        return _case(name, why, w, ln, negative=1, seed=15)
    if name == "negative_63":
        w, ln = _sentences(12)
        return _case(name, why, w, ln, negative=63, seed=16)
    if name == "f_skip":
        w, ln = _sentences(20)
        return _case(name, why, w[:8], ln[:8], s=6.0, seed=17)
    if name == "keep_boundary":
        w, ln = _sentences(20)
        w = w.copy()
        seed, n = 18, VOCAB + 2
        v, u, tv, tu = VOCAB, VOCAB + 1, 5 * 20 + 7, 11 * 20 + 9       # each node at exactly one token, inside its sentence
        assert ln[5] > 9 and ln[11] > 11
        w.reshape(-1)[tv], w.reshape(-1)[tu] = v, u
        keep = np.full(n, KEEP_ALL, np.int64)
        keep[v], keep[u] = keep_draw(seed, 0, tv), keep_draw(seed, 0, tu) - 1
        return _case(name, why, w, ln, n=n, sample_int=keep, seed=seed, v=v, u=u, tv=tv, tu=tu)
    if name == "table_ties":
        w, ln = _sentences(20)
        return _case(name, why, w, ln, cum_table=np.arange(1, VOCAB + 1), seed=19)
    if name.startswith("epochs_3_e"):
        e = int(name[-1])
        w, ln = _sentences(20)
        if e == 0:
            return _case(name, why, w, ln, epochs=3, first_epoch=0, seed=20)
        before = "epochs_3_e%d" % (e - 1)
        s0, s1, _ = sgns_mirror(before, np.float32)
        return _case(name, why, w, ln, epochs=3, first_epoch=e, seed=20, syn0=s0, syn1=s1)
    if name == "min_alpha_clamp":
        w, ln = _sentences(20)
        return _case(name, why, w, ln, epochs=3, first_epoch=1, alpha=0.025, min_alpha=0.03, seed=21)
    if name == "degenerate_sentences":
        rng = np.random.RandomState(22)
        never = np.arange(8)                        # sample_int 0: kept only on a draw of 0
        rest = np.arange(8, VOCAB)
        sent = []
        for _ in range(15):
            sent += [[rng.choice(never), rng.choice(never)], [rng.choice(never), rng.choice(rest)], [rng.choice(rest), rng.choice(never)],
                     [rng.choice(rest)], [rng.choice(never)]]
        for _ in range(90):
            sent.append(list(rng.choice(rest, 2)))
        sent = [sent[i] for i in rng.permutation(len(sent))]
        ln = np.array([len(x) for x in sent])
        w = np.array([x + [-1] * (2 - len(x)) for x in sent])
        keep = np.full(VOCAB, KEEP_ALL, np.int64)
        keep[never] = 0
        return _case(name, why, w, ln, sample_int=keep, seed=22)
    if name == "partition":
        S = PARTITION_S
        n = 2 * S
        w = np.random.RandomState(23).permutation(n).reshape(S, 2)
        return _case(name, why, w, np.full(S, 2), n=n, seed=23, syn0=np.zeros((n, 64), np.float32), moved_min=1e-3)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def sgns_mirror(name, dtype=np.float64, ablate=None, reverse=False):
    """the mirror on the case's one epoch, from its start state and tables -> (syn0, syn1neg, stats); reverse: the sentences in
    reversed order, each with its own tokens, alpha and draws (another serial order of the same updates)"""
    c = sgns_case(name)
    stats = {}
    s0, s1 = M.sgns(c.walks, c.lengths, c.n, c.d, window=c.window, epochs=c.epochs, negative=c.negative, alpha=c.alpha, min_alpha=c.min_alpha,
                    seed=c.seed, run_epochs=c.first_epoch + 1, dtype=dtype, syn0=c.syn0, syn1=c.syn1, cum_table=c.cum_table,
                    sample_int=c.sample_int, first_epoch=c.first_epoch, stats=stats, ablate=ablate,
                    order=range(len(c.walks) - 1, -1, -1) if reverse else None)
    return s0, s1, stats


def d32(name):
    """max |fp32 mirror - fp64 mirror| over syn0 and syn1neg: the rounding of the kernel's arithmetic in numpy's order, the unit of
    the GPU comparison's bound"""
    a0, a1, _ = sgns_mirror(name, np.float32)
    b0, b1, _ = sgns_mirror(name, np.float64)
    return float(max(np.abs(a0 - b0).max(), np.abs(a1 - b1).max()))


# ---------------------------------------------------------------------------------------------------------------------- counts
@functools.lru_cache(maxsize=None)
def counts_case():
    """-> (walks [37][7] int32, lengths, n): 259 tokens (not a multiple of 256), -1 tails, garbage past `lengths` that names a node
    no valid token names (counting it would show), one node that never occurs"""
    rng = np.random.RandomState(29)
    n, S, L = 30, 37, 7
    absent = 13
    ids = np.setdiff1d(np.arange(n), [absent])
    w = rng.choice(ids, (S, L)).astype(np.int32)
    ln = rng.randint(1, L + 1, S).astype(np.int32)
    ln[:6] = [1, L, L, L, L, L]
    w[1:6].reshape(-1)[:len(ids)] = ids          # every other node occurs
    past = np.arange(L)[None, :] >= ln[:, None]
    w[past] = np.where(rng.rand(int(past.sum())) < 0.5, -1, absent)
    w[0, 1:] = -1
    return w, ln, n
