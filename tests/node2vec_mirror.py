"""Numpy statement of the node2vec kernels (csrc/counter_rng.h, csrc/walk.hip, csrc/sgns.hip), for tests only.

  * rng_key: the counter-based generator, on uint64 arrays;
  * walks(): the walk kernel's algorithm vectorised over walks -- first-order candidate by binary search in the row's fp64 prefix
    sums, acceptance b / max(1/p, 1, 1/q), the direct draw after 64 refused candidates -- with the same keys, so the device walks
    must equal these bit for bit;
  * sgns(): serial skip-gram negative sampling in the order of the kernel at concurrency 1 (sentence by sentence, center by center,
    context by context), fp32, exact sigmoid with gensim's |f| >= 6 skip.  The kernel reduces dot products across a wave, numpy
    in its own order: the two agree to that rounding, not bitwise.  sgns() also runs in fp64 (the reference of
    tests/test_gpu_node2vec_ops.py), from a given state and given tables, over a range of epochs, counts what it did (stats=) and can
    swap one rule for the plausible wrong one (ablate=), which is how tests/test_node2vec_mirror.py shows that a comparison can fail;
  * exact_transitions(): the walk's transition law from its definition, in fp64, in the form transition_chi2 tests against.
"""
from __future__ import annotations

import math

import numpy as np

K = np.uint64(0x9E3779B97F4A7C15)
TAG_WALK, TAG_PERM, TAG_WINDOW, TAG_KEEP, TAG_NEG, TAG_INIT = 1, 2, 3, 4, 5, 6
REJECT_TRIES = 64


def _mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rng_key(seed, tag, a, b, c):
    u = lambda v: np.asarray(v).astype(np.uint64)  # noqa: E731
    with np.errstate(over="ignore"):
        h = _mix(u(seed) + u(tag) + K)
        h = _mix(h + u(a) + K)
        h = _mix(h + u(b) + K)
        return _mix(h + u(c) + K)


def unit_f64(h):
    return (h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def unit_f32(h):
    return (h >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)


def u32(h):
    return (h >> np.uint64(32)).astype(np.int64)


def csr(adj):
    import scipy.sparse as sp
    a = sp.csr_matrix(adj, dtype=np.float64)
    a.sum_duplicates()
    a.sort_indices()
    return a


def row_prefix(a):
    """inclusive prefix sums of each row, left to right (the device's sequential fp64 sums)"""
    cum = np.zeros(a.nnz)
    b, deg = a.indptr[:-1], np.diff(a.indptr)
    for k in range(int(deg.max()) if len(deg) else 0):
        rows = np.flatnonzero(deg > k)
        e = b[rows] + k
        cum[e] = a.data[e] if k == 0 else cum[e - 1] + a.data[e]
    return cum


def start_nodes(n, num_walks, seed):
    out = []
    for r in range(num_walks):
        keys = rng_key(seed, TAG_PERM, r, np.arange(n), 0)
        out.append(np.argsort(keys, kind="stable"))
    return np.concatenate(out).astype(np.int64)


def _pick(cum, b, e, t, stats=None):
    lo, hi = b.copy(), e - 1
    while True:
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi) >> 1
        if stats is not None:       # probes of an entry whose prefix sum equals the one before it (its weight was absorbed)
            m = np.where(act & (mid > b), mid, 0)
            stats["prefix_ties"] += int((act & (mid > b) & (cum[m] == cum[np.maximum(m - 1, 0)])).sum())
        gt = cum[np.where(act, mid, 0)] > t
        hi = np.where(act & gt, mid, hi)
        lo = np.where(act & ~gt, mid + 1, lo)


def direct_draw_scalar(col, val, b, e, prev, has_edge, inv_p, inv_q, u):
    """the direct draw of one walk, entry by entry as walk.hip's last branch reads: the biased row summed left to right, u * sum located by a scan"""
    xs = col[b:e]
    bias = np.where(xs == prev, inv_p, np.where(has_edge(xs, np.full(len(xs), prev)), 1.0, inv_q))
    terms = val[b:e] * bias
    s = 0.0
    for tv in terms:
        s += tv
    tt = float(u) * s
    run, pick = 0.0, xs[-1]
    for xv, tv in zip(xs, terms):
        run += tv
        if run > tt:
            pick = xv
            break
    return pick


def _direct_draws(col, val, b, e, prev, has_edge, inv_p, inv_q, u):
    """direct_draw_scalar for many walks at once: entry k of every row in one numpy operation, so each walk's sums keep their
    left-to-right order (tests/test_node2vec_mirror.py holds the two to the same picks)"""
    deg = e - b
    m = len(b)
    terms = np.zeros((int(deg.max()), m))
    total = np.zeros(m)
    for k in range(terms.shape[0]):
        act = np.flatnonzero(deg > k)
        ek = b[act] + k
        xs = col[ek]
        bias = np.where(xs == prev[act], inv_p, np.where(has_edge(xs, prev[act]), 1.0, inv_q))
        terms[k, act] = val[ek] * bias
        total[act] = total[act] + terms[k, act]
    tt = u * total
    run = np.zeros(m)
    pick = col[e - 1].copy()
    open_ = np.ones(m, bool)
    for k in range(terms.shape[0]):
        act = np.flatnonzero(open_ & (deg > k))
        if len(act) == 0:
            break
        run[act] = run[act] + terms[k, act]
        hit = act[run[act] > tt[act]]
        pick[hit] = col[b[hit] + k]
        open_[hit] = False
    return pick


def walks(adj, num_walks, walk_length, p, q, seed, stats=None, scalar_direct=False):
    """-> (walks int32 [num_walks * N, walk_length] with -1 after the end, lengths int32).  stats: a dict that receives "steps",
    "direct_draws" (steps that fell through the 64 candidates) and "prefix_ties" (binary-search probes of an entry whose prefix sum
    equals its left neighbour's)"""
    a = csr(adj)
    n = a.shape[0]
    ptr, col, val = a.indptr.astype(np.int64), a.indices.astype(np.int64), a.data
    cum = row_prefix(a)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    edge_keys = rows * n + col          # sorted (rows ascending, columns sorted within a row)
    inv_p, inv_q = 1.0 / p, 1.0 / q
    bmax = max(inv_p, 1.0, inv_q)
    acc_p, acc_1, acc_q = inv_p / bmax, 1.0 / bmax, inv_q / bmax
    if stats is not None:
        stats.update(steps=0, direct_draws=0, prefix_ties=0)

    def has_edge(u, v):
        k = u * n + v
        i = np.minimum(np.searchsorted(edge_keys, k), max(len(edge_keys) - 1, 0))
        return (edge_keys[i] == k) if len(edge_keys) else np.zeros(len(u), bool)

    starts = start_nodes(n, num_walks, seed)
    W = len(starts)
    out = np.full((W, walk_length), -1, np.int32)
    out[:, 0] = starts
    lengths = np.ones(W, np.int32)
    cur, prev = starts.copy(), np.full(W, -1, np.int64)
    alive = np.ones(W, bool)
    wid = np.arange(W, dtype=np.int64)
    for step in range(1, walk_length):
        b, e = ptr[cur], ptr[cur + 1]
        alive &= b < e
        idx = np.flatnonzero(alive)
        if len(idx) == 0:
            break
        nxt = np.full(W, -1, np.int64)
        if stats is not None:
            stats["steps"] += len(idx)
        if step == 1:
            u = unit_f64(rng_key(seed, TAG_WALK, wid[idx], step, 0))
            nxt[idx] = col[_pick(cum, b[idx], e[idx], u * cum[e[idx] - 1], stats)]
        else:
            pend = idx
            for t in range(REJECT_TRIES):
                bb, ee = b[pend], e[pend]
                u = unit_f64(rng_key(seed, TAG_WALK, wid[pend], step, 2 * t))
                x = col[_pick(cum, bb, ee, u * cum[ee - 1], stats)]
                acc = np.where(x == prev[pend], acc_p, np.where(has_edge(x, prev[pend]), acc_1, acc_q))
                v = unit_f64(rng_key(seed, TAG_WALK, wid[pend], step, 2 * t + 1))
                ok = v < acc
                nxt[pend[ok]] = x[ok]
                pend = pend[~ok]
                if len(pend) == 0:
                    break
            if len(pend):               # the direct draw from the biased row, sequential sums
                if stats is not None:
                    stats["direct_draws"] += len(pend)
                u = unit_f64(rng_key(seed, TAG_WALK, wid[pend], step, 2 * REJECT_TRIES))
                if scalar_direct:
                    nxt[pend] = [direct_draw_scalar(col, val, b[w], e[w], prev[w], has_edge, inv_p, inv_q, uw) for w, uw in zip(pend, u)]
                else:
                    nxt[pend] = _direct_draws(col, val, b[pend], e[pend], prev[pend], has_edge, inv_p, inv_q, u)
        out[idx, step] = nxt[idx]
        prev[idx] = cur[idx]
        cur[idx] = nxt[idx]
        lengths[idx] += 1
    return out, lengths


def tables(counts, sample=1e-3, ns_exponent=0.75):
    """gensim 3.x make_cum_table / prepare_vocab sample_int, vocabulary in node order"""
    counts = np.asarray(counts, np.int64)
    pw = counts.astype(np.float64) ** ns_exponent
    cum = np.zeros(len(counts), np.uint32)
    total = float(pw.sum())
    run = 0.0
    for i, v in enumerate(pw):
        run += v
        cum[i] = round(run / total * (2 ** 31 - 1))
    thr = sample * float(counts.sum())
    keep = np.empty(len(counts), np.int64)
    for i, v in enumerate(counts):
        prob = (math.sqrt(v / thr) + 1) * (thr / v) if v > 0 else 1.0
        keep[i] = int(round(min(prob, 1.0) * 2 ** 32))
    return cum, keep


def init_vectors(n, dim, seed):
    node, comp = np.divmod(np.arange(n * dim, dtype=np.int64), dim)
    u = unit_f32(rng_key(seed, TAG_INIT, node, comp, 0))
    syn0 = ((u - np.float32(0.5)) / np.float32(dim)).astype(np.float32).reshape(n, dim)
    return syn0, np.zeros((n, dim), np.float32)


def _sig(f):
    one = type(f)(1.0)
    return one / (one + np.exp(-f))


ABLATIONS = ("keep_lt", "bisect_right", "tail_tokens", "window_hi", "last_negative", "neg_eq_center", "alpha_epoch", "f_skip")


def sgns(walks_, lengths, n, dim, window=10, epochs=5, negative=5, sample=1e-3, alpha=0.025, min_alpha=1e-4, seed=0, run_epochs=None,
         dtype=np.float32, syn0=None, syn1=None, cum_table=None, sample_int=None, first_epoch=0, stats=None, ablate=None, order=None):
    """serial skip-gram negative sampling (the kernel's order at concurrency 1) -> (syn0, syn1neg) after the epochs
    [first_epoch, run_epochs) (default: all) of `epochs`.

    dtype: np.float32 does the kernel's arithmetic (numpy's summation order); np.float64 is the same serial algorithm in fp64 (alpha
    stays the fp32 number the kernel is given).  syn0 / syn1: the start state (copied) in place of init_vectors; cum_table /
    sample_int: gensim's two tables in place of tables(counts, sample).  stats: a dict that receives "pairs" (pair updates), "f_abs"
    (every |f| a |f| < 6 decision was taken on, in order), "neg_eq_center", "kept_len" ((epoch, sentence) -> kept length), "kept_pos"
    and "dropped_pos" (walk positions of the valid tokens kept / dropped, all epochs).  ablate: one of ABLATIONS, the named rule
    replaced by the plausible wrong one (for tests that show a comparison can fail).  order: the sentence indices in the order to run
    them (default 0 .. S-1, the kernel's at concurrency 1); a sentence keeps its tokens, alpha and draws wherever it runs."""
    assert ablate is None or ablate in ABLATIONS, ablate
    T = np.dtype(dtype).type
    W, L = walks_.shape
    tok = walks_.reshape(-1)
    valid = (np.arange(L)[None, :] < lengths[:, None]).reshape(-1)
    if cum_table is None or sample_int is None:
        counts = np.bincount(tok[valid], minlength=n)
        cum_d, keep_d = tables(counts, sample)
    cum = cum_d if cum_table is None else np.asarray(cum_table)
    keep_int = keep_d if sample_int is None else np.asarray(sample_int, np.int64)
    cum_last = int(cum[-1])
    i0, i1 = init_vectors(n, dim, seed) if syn0 is None or syn1 is None else (None, None)
    syn0 = (i0 if syn0 is None else np.asarray(syn0)).astype(T)
    syn1 = (i1 if syn1 is None else np.asarray(syn1)).astype(T)
    a0, amin = float(np.float32(alpha)), float(np.float32(min_alpha))
    tok_ids = np.arange(W * L)
    side = "right" if ablate == "bisect_right" else "left"
    n_neg = negative - 1 if ablate == "last_negative" else negative
    if stats is not None:
        stats.update(pairs=0, f_abs=[], neg_eq_center=0, kept_len={}, kept_pos=[], dropped_pos=[])
    for ep in range(first_epoch, epochs if run_epochs is None else run_epochs):
        draw = u32(rng_key(seed, TAG_KEEP, ep, tok_ids, 0))
        thr = keep_int[np.where(valid, tok, 0)]
        keep = valid & ((draw < thr) if ablate == "keep_lt" else (draw <= thr))
        if ablate == "tail_tokens":
            keep &= (tok_ids % L) < 64
        bwin = u32(rng_key(seed, TAG_WINDOW, ep, tok_ids, 0)) % window
        if stats is not None:
            stats["kept_pos"] += list(tok_ids[keep] % L)
            stats["dropped_pos"] += list(tok_ids[valid & ~keep] % L)
        for s in (range(W) if order is None else order):
            prog = ((0 if ablate == "alpha_epoch" else ep) + s / W) / epochs
            al = T(np.float32(max(amin, a0 - (a0 - amin) * prog)))
            pos = np.flatnonzero(keep[s * L:(s + 1) * L])
            kn = tok[s * L + pos]
            kt = s * L + pos
            klen = len(pos)
            if stats is not None:
                stats["kept_len"][ep, s] = klen
            for i in range(klen):
                c = kn[i]
                b = int(bwin[kt[i]])
                h = syn1[c].copy()
                hi = min(klen, i + window + 1 - b)
                if ablate == "window_hi":
                    hi = min(klen, i + window - b)
                for j in range(max(0, i - window + b), hi):
                    if j == i:
                        continue
                    x = kn[j]
                    ks = np.arange(1, n_neg + 1)
                    r = u32(rng_key(seed, TAG_NEG, ep, kt[i], np.uint64(kt[j]) * np.uint64(64) + ks.astype(np.uint64))) % cum_last
                    tg = np.searchsorted(cum, r, side=side)
                    l1 = syn0[x].copy()
                    neu = np.zeros(dim, T)
                    f = T(np.dot(l1, h))
                    if stats is not None:
                        stats["pairs"] += 1
                        stats["f_abs"].append(abs(float(f)))
                    if abs(f) < 6 or ablate == "f_skip":
                        g = T((T(1) - _sig(f)) * al)
                        neu += g * h
                        h += g * l1
                    for t in tg:
                        if t == c:
                            if stats is not None:
                                stats["neg_eq_center"] += 1
                            if ablate != "neg_eq_center":
                                continue
                        row = h if t == c else syn1[t]
                        f = T(np.dot(l1, row))
                        if stats is not None:
                            stats["f_abs"].append(abs(float(f)))
                        if abs(f) >= 6 and ablate != "f_skip":
                            continue
                        g = T((T(0) - _sig(f)) * al)
                        neu += g * row
                        if t == c:
                            h += g * l1
                        else:
                            syn1[t] = row + g * l1
                    syn0[x] += neu
                syn1[c] = h
    return syn0, syn1


def msi_small_graph():
    """the weighted, directed msi_small graph (tests/golden/msi_small) -> (MsiGraph, CSR, names)"""
    import os

    from gcn_drug_repurposing_amd.msi import COVID_WEIGHTS, MsiGraph
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msi_small")
    g = MsiGraph().load({f[:-4]: os.path.join(d, f) for f in os.listdir(d) if f.endswith(".tsv")}).weight_graph(COVID_WEIGHTS)
    adj, names, _ = g.to_csr()
    return g, adj, names


def fixture_transitions(fix, case):
    """the reference walker's probabilities of fixture case `case` -> (first {cur: {next: prob}}, second {(prev, cur): {next: prob}})"""
    first = {}
    for c, x, pr in zip(fix[f"node_cur_{case}"], fix[f"node_next_{case}"], fix[f"node_prob_{case}"]):
        first.setdefault(int(c), {})[int(x)] = float(pr)
    second = {}
    for a, c, x, pr in zip(fix[f"edge_prev_{case}"], fix[f"edge_cur_{case}"], fix[f"edge_next_{case}"], fix[f"edge_prob_{case}"]):
        second.setdefault((int(a), int(c)), {})[int(x)] = float(pr)
    return first, second


def exact_transitions(adj, p, q):
    """node2vec's transition law from its definition, fp64, in fixture_transitions' form: step 1 from cur is w(cur, x) / sum w; a later
    step from (prev, cur) is w(cur, x) b(x) / sum w b with b = 1/p if x == prev, 1 if the edge x -> prev exists, else 1/q.  One state
    per node with out-edges and one per edge prev -> cur whose head has out-edges."""
    a = csr(adj)
    n = a.shape[0]
    ptr, col, val = a.indptr, a.indices, a.data
    edges = set(zip(np.repeat(np.arange(n), np.diff(ptr)).tolist(), col.tolist()))
    first, second = {}, {}
    for c in range(n):
        xs, w = col[ptr[c]:ptr[c + 1]].tolist(), val[ptr[c]:ptr[c + 1]]
        if not xs:
            continue
        first[c] = dict(zip(xs, (w / math.fsum(w)).tolist()))
    for prev in range(n):
        for c in col[ptr[prev]:ptr[prev + 1]].tolist():
            if c not in first:
                continue
            xs, w = col[ptr[c]:ptr[c + 1]].tolist(), val[ptr[c]:ptr[c + 1]]
            bias = np.array([1.0 / p if x == prev else (1.0 if (x, prev) in edges else 1.0 / q) for x in xs])
            wb = w * bias
            second[prev, c] = dict(zip(xs, (wb / math.fsum(wb)).tolist()))
    return first, second


def transition_chi2(walks_, lengths, fix=None, case=None, min_visits=200, laws=None, n=None):
    """chi-square goodness of fit of the walks' transitions against the reference's probabilities (fixture case `case`), or against
    laws = (first, second) over n nodes given directly (exact_transitions): step 1 per node cur (alias_nodes), later steps per state
    (prev, cur) (alias_edges).  Cells with an expected count below 5 are pooled.
    -> (p-values of the states with >= min_visits visits, transitions the reference gives probability 0)"""
    from scipy.stats import chi2
    if laws is None:
        laws, n = fixture_transitions(fix, case), len(fix["names"])
    first, second = laws
    walks_ = np.asarray(walks_, np.int64)
    lengths = np.asarray(lengths)
    obs1, obs2 = {}, {}
    m = lengths >= 2
    keys, cnt = np.unique(walks_[m, 0] * n + walks_[m, 1], return_counts=True)
    for k, v in zip(keys, cnt):
        obs1.setdefault(int(k // n), {})[int(k % n)] = int(v)
    for s in range(2, walks_.shape[1]):
        m = lengths > s
        keys, cnt = np.unique((walks_[m, s - 2] * n + walks_[m, s - 1]) * n + walks_[m, s], return_counts=True)
        for k, v in zip(keys, cnt):
            st = (int(k // (n * n)), int(k // n % n))
            obs2.setdefault(st, {})[int(k % n)] = obs2.get(st, {}).get(int(k % n), 0) + int(v)
    pvals, impossible = [], 0
    for obs, ref in ((obs1, first), (obs2, second)):
        for st, o in obs.items():
            probs = ref.get(st, {})
            impossible += sum(v for x, v in o.items() if probs.get(x, 0.0) <= 0)
            total = sum(o.values())
            if total < min_visits:
                continue
            xs = sorted(probs)
            e = np.array([probs[x] * total for x in xs])
            ob = np.array([o.get(x, 0) for x in xs], np.float64)
            small = e < 5
            if small.any():
                e = np.append(e[~small], e[small].sum())
                ob = np.append(ob[~small], ob[small].sum())
            if len(e) < 2:
                continue
            stat = float(((ob - e) ** 2 / e).sum())
            pvals.append(float(chi2.sf(stat, len(e) - 1)))
    return np.asarray(pvals), impossible
