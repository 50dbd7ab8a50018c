"""Inputs of tests/test_gpu_paths_ops.py -- the shortest-path tree, count and between ops (csrc/paths.hip, csrc/trace.hip) at the C ABI.
Every builder is deterministic and small (n <= ~700).  What each case is for is stated at the builder; that the cases have those
properties is asserted on the CPU in tests/test_paths_ops_cases.py.  Test-side only."""
import numpy as np
import scipy.sparse as sp

WAVE = 64
SHORT_ROW = 32          # paths.hip / trace.hip: a row of up to this many entries is read by one lane, a longer one by the whole wave
FILL_NODES = 256        # trace_fill_kernel compacts this many nodes per iteration


def _csr(n, edges):
    rows = np.array([e[0] for e in edges], np.int64)
    cols = np.array([e[1] for e in edges], np.int64)
    a = sp.csr_matrix((np.ones(len(edges)), (rows, cols)), shape=(n, n))
    a.sort_indices()
    assert a.nnz == len(edges), "an edge twice"
    return a


# ---- counts at the 2^53 boundary ------------------------------------------------------------------------------------------------------

def boundary_count_graph(widths, extra, chain_first=False):
    """Node 0 is the target; layer j (widths[j - 1] nodes) is fully connected to layer j - 1 (layer 1 to the target); one top node points
    at every node of the last layer, so it has prod(widths) shortest paths.  extra: a chain of len(widths) nodes from the target whose
    head the top node points at as well -- same distance, one path more.  chain_first: the chain has the lowest node indices after the
    target (its entry is the first of the top row), otherwise the highest (the last entry).
    -> dict(adj, n, top, head (or None), layers (list of index arrays), product (Python int))"""
    k = len(widths)
    at = 1
    chain = []
    if extra and chain_first:
        chain = list(range(at, at + k))
        at += k
    layers = []
    for w in widths:
        layers.append(np.arange(at, at + w))
        at += w
    top = at
    at += 1
    if extra and not chain_first:
        chain = list(range(at, at + k))
        at += k
    n = at
    edges = []
    for j, lay in enumerate(layers):
        below = [0] if j == 0 else layers[j - 1].tolist()
        edges += [(int(v), u) for v in lay for u in below]
    edges += [(top, int(u)) for u in layers[-1]]
    if extra:
        edges += [(chain[0], 0)] + [(chain[i], chain[i - 1]) for i in range(1, k)] + [(top, chain[-1])]
    product = 1
    for w in widths:
        product *= w
    return dict(adj=_csr(n, edges), n=n, top=top, head=chain[-1] if extra else None, layers=layers, product=product)


ONE_LANE_WIDTHS = [32] * 10 + [8]        # the top row has 8 (9) entries; every row is read by one lane
WHOLE_WAVE_WIDTHS = [32] + [64] * 8      # the top row has 64 (65) entries; it and the layers above the second are read by the whole wave
FAR_ABOVE_WIDTHS = [64] * 10             # 2^60 at the top, 2^54 already in the last layer


def lane_local_overcount_graph():
    """The whole-wave row in which ONE lane alone sees the overflow: the row of the apex is [T, 63 sinks, H] -- T the top node of
    boundary_count_graph(WHOLE_WAVE_WIDTHS) with exactly 2^53 paths at position 0, H the head of a chain (1 path, same distance) at
    position 64, and between them 63 sinks that cannot reach the target (dist 255, skipped).  Lane 0 reads positions 0 and 64 and sums
    2^53 + 1, which rounds to 2^53; every other lane holds 0, so the butterfly's sums (2^53 + 0) are exact everywhere and only lane 0's
    verdict tells.  The apex is owned by lane 43: the verdict reaches it through the ballot alone.
    -> dict(adj, n, apex, top, head, sinks)"""
    g = boundary_count_graph(WHOLE_WAVE_WIDTHS, False)
    a = g["adj"].tocoo()
    edges = list(zip(a.row.tolist(), a.col.tolist()))
    top = g["top"]
    depth = len(WHOLE_WAVE_WIDTHS) + 1                     # the distance of T
    sinks = list(range(top + 1, top + 1 + (WAVE - 1)))
    chain = list(range(sinks[-1] + 1, sinks[-1] + 1 + depth))
    apex = chain[-1] + 1
    n = apex + 1
    edges += [(chain[0], 0)] + [(chain[i], chain[i - 1]) for i in range(1, depth)]
    edges += [(apex, top)] + [(apex, s) for s in sinks] + [(apex, chain[-1])]
    return dict(adj=_csr(n, edges), n=n, apex=apex, top=top, head=chain[-1], sinks=sinks)


# ---- the tie rule of next at the row-length boundaries --------------------------------------------------------------------------------

TIE_LATER = (1, 64, 70, 130)             # carriers of a target after its first one: the next entry, the next chunk, the third chunk
TIE_UNREACHED = (61, 62)                 # targets nothing reaches: a hub's row is read to its end
TIE_DIRECT = 60                          # the target that is itself a successor of the hubs


def tie_first_carriers(L):
    """p(q) for q = 0 .. 63 (None: nothing carries q).  The positions 0, 31, 32, 63, 64, 65 and L - 1 (those below L) are all taken;
    bit 63 sits at lane 63 of a chunk when the row has one"""
    must = [p for p in (0, 31, 32, 63, 64, 65, L - 1) if p < L]
    must = list(dict.fromkeys(must))
    first = []
    for q in range(WAVE):
        if q in TIE_UNREACHED or q == TIE_DIRECT:
            first.append(None)
        elif q == 63:
            first.append(63 if L >= 64 else L - 1)
        elif q < len(must):
            first.append(must[q])
        else:
            first.append((7 * q + 3) % L)
    return first


def tie_rule_graph(L, hub_lanes, last_wave=False):
    """Nodes 0 .. 63 are targets (target q of the pass is node q, except q = TIE_DIRECT, which is the successor u_{L // 2}); nodes
    64 .. 64 + L - 1 are the successors u_0 < ... < u_{L-1}; the hubs' row is exactly the L successors.  u_{p(q)} and the successors
    TIE_LATER after it point at target q, no earlier one does, so next[q][hub] = u_{p(q)} and dist = 2 (1 and u_{L // 2} for TIE_DIRECT,
    255 / -1 for TIE_UNREACHED).  hub_lanes: the lanes of one wave that own a hub; that wave starts at the first multiple of 64 behind
    the successors.  last_wave: the hubs' wave is the last, partial one; otherwise a partial wave of 3 isolated nodes follows it.
    n is no multiple of 4.
    -> dict(adj, n, L, targets (int32 [64]), succ, hubs, first (p(q)), dist uint8 [64, n], next int32 [64, n] -- the closed form)"""
    succ = np.arange(WAVE, WAVE + L)
    base = -(-(WAVE + L) // WAVE) * WAVE
    hubs = [base + l for l in sorted(hub_lanes)]
    if last_wave:
        assert max(hub_lanes) <= WAVE - 4
        n = hubs[-1] + 1
        n += (1 if n % 4 == 0 else 0)
    else:
        n = base + WAVE + 3
    assert n % 4 and n % WAVE and (n - 1) // WAVE == (hubs[-1] // WAVE if last_wave else hubs[-1] // WAVE + 1)
    first = tie_first_carriers(L)
    targets = np.arange(WAVE, dtype=np.int32)
    direct = int(succ[L // 2])
    targets[TIE_DIRECT] = direct
    dist = np.full((WAVE, n), 255, np.uint8)
    nxt = np.full((WAVE, n), -1, np.int32)
    edges = [(h, int(u)) for h in hubs for u in succ]
    for q in range(WAVE):
        dist[q, targets[q]] = 0
        if first[q] is None:
            continue
        for i in [first[q]] + [first[q] + d for d in TIE_LATER if first[q] + d < L]:
            edges.append((int(succ[i]), q))
            dist[q, succ[i]] = 1
            nxt[q, succ[i]] = q
        for h in hubs:
            dist[q, h] = 2
            nxt[q, h] = succ[first[q]]
    for h in hubs:
        dist[TIE_DIRECT, h] = 1
        nxt[TIE_DIRECT, h] = direct
    return dict(adj=_csr(n, edges), n=n, L=L, targets=targets, succ=succ, hubs=hubs, first=first, dist=dist, next=nxt)


# (L, hub_lanes, last_wave): over the cases an owner at lane 0, at lane 63, two owners in one wave, an owner in the last, partial wave
TIE_CASES = [(32, (0,), False), (33, (0,), False), (64, (63,), False), (65, (5, 40), False), (128, (0, 63), False),
             (129, (17,), True), (200, (3, 9), True)]


def tie_weight_graph():
    """Rows of 33, 64 and 65 successors that are ALL one hop closer, for the ties of best / best_next: nodes 0 and 1 are targets, the 65
    nodes of layer A point at both, the hubs h33 / h64 / h65 point at the first 33 / 64 / 65 nodes of A (h64 and h65 in one wave, h33 at
    lane 0 of the next), and three nodes above point at all the hubs.
    -> dict(adj, n, targets, layer, hubs (dict by row length), above)"""
    layer = np.arange(2, 2 + 65)
    hubs = {64: 100, 65: 127, 33: 128}
    above = [190, 191, 197]
    n = 199
    edges = [(int(u), t) for u in layer for t in (0, 1)]
    for k, h in hubs.items():
        edges += [(h, int(u)) for u in layer[:k]]
    edges += [(v, h) for v in above for h in hubs.values()]
    return dict(adj=_csr(n, edges), n=n, targets=np.array([0, 1], np.int32), layer=layer, hubs=hubs, above=above)


def tie_weights(kind, q, n):
    """zero: only +0.0 and -0.0; int: small integers (many equal sums)"""
    rng = np.random.RandomState(5)
    if kind == "zero":
        return np.where(rng.rand(q, n) < 0.5, 0.0, -0.0)
    return rng.randint(-2, 3, size=(q, n)).astype(np.float64)


def tie_weight_tables(g, kind):
    """the weight tables [2, n] of tie_weight_graph.  zero: only +0.0 / -0.0.  int: integers -2 .. 1 with the one larger value 2 placed
    where the lanes meet: for target 0 at positions 63 and 64 of layer A (lane 63 against lane 0's second entry: the smaller index wins
    through the butterfly; the row of 33 sees neither), for target 1 at position 64 alone (only the row of 65 sees it)"""
    if kind == "zero":
        return tie_weights("zero", 2, g["n"])
    w = np.random.RandomState(6).randint(-2, 2, size=(2, g["n"])).astype(np.float64)
    w[0, g["layer"][[63, 64]]] = 2.0
    w[1, g["layer"][64]] = 2.0
    return w


# ---- the nodes between pairs ----------------------------------------------------------------------------------------------------------

BETWEEN_WIDTHS = [4, 40, 60, 80, 60, 40, 4]


def between_graph():
    """A directed layered graph with many equal-length routes: node a of layer j points at node b of layer j + 1 when (3 a + 5 b) % 7 < 3
    (positions within the layers); behind the layers a chain of 6 nodes (one route) and 9 isolated nodes.  n = 303: the layers alone
    span both 256-node iterations of the fill kernel.  The first sources and targets are the pairs the tests name:
      (0, 0) first layer -> last layer, many routes over every layer;  (1, 1) the chain's ends, one route;  (2, 2) source = target;
      (0, 3) / (1, 0) unreachable (an isolated target; the chain reaches no layer);  (2, 0) from the middle layer on.
    -> dict(adj, n, sources int32 [64], targets int32 [64], layers, chain, isolated)"""
    at = 0
    layers = []
    for w in BETWEEN_WIDTHS:
        layers.append(np.arange(at, at + w))
        at += w
    chain = list(range(at, at + 6))
    at += 6
    isolated = list(range(at, at + 9))
    n = at + 9
    edges = []
    for j in range(len(layers) - 1):
        for a, v in enumerate(layers[j]):
            for b, u in enumerate(layers[j + 1]):
                if (3 * a + 5 * b) % 7 < 3:
                    edges.append((int(v), int(u)))
    edges += [(chain[i], chain[i + 1]) for i in range(5)]
    mid = int(layers[3][11])
    sources = [int(layers[0][0]), chain[0], mid, isolated[0]] + layers[0][1:].tolist() + layers[1].tolist() + layers[2][:17].tolist()
    targets = [int(layers[-1][0]), chain[-1], mid, isolated[1], int(layers[5][7])] + layers[-1][1:].tolist() + layers[5][8:].tolist() \
        + layers[4][:24].tolist()
    assert len(sources) == 64 and len(targets) == 64 and len(set(sources)) == 64 and len(set(targets)) == 64
    return dict(adj=_csr(n, edges), n=n, sources=np.array(sources, np.int32), targets=np.array(targets, np.int32), layers=layers,
                chain=chain, isolated=isolated)


BETWEEN_PASSES = [(1, 1), (3, 5), (64, 64)]
PAIR_MANY, PAIR_SINGLE, PAIR_SAME, PAIR_UNREACHABLE, PAIR_HALF = (0, 0), (1, 1), (2, 2), (0, 3), (2, 0)


# ---- the duplicate-column check at the row boundaries ---------------------------------------------------------------------------------

ROW_BOUNDARY_ROWS = {2: [3, 7], 3: [7, 9], 7: [9, 12], 9: [12, 13, 19], 12: [19], 13: [19], 19: [0, 2]}
ROW_BOUNDARY_REPEATS = {            # variant -> {row: its entries with a column twice}; the row the refusal names is the largest key
    "first": {2: [3, 7, 7]},
    "last": {19: [0, 2, 2]},
    "after_empty": {7: [9, 9, 12]},
    "two": {2: [3, 3, 7], 13: [19, 19]},
}
ROW_BOUNDARY_TARGETS = np.array([19, 12, 0], np.int32)


def row_boundary_graph(variant=None):
    """20 rows with runs of empty ones (0-1, 4-6, 8, 10-11, 14-18).  The last column of a row equals the first column of the next
    non-empty row directly (rows 2 | 3: 7, rows 12 | 13: 19) and across empty rows (3 | 7: 9, 7 | 9: 12, 9 | 12: 19): equal neighbours
    in col[] that are no repeat.  variant None: no row holds a column twice.  Otherwise ROW_BOUNDARY_REPEATS: a true repeat in the
    first non-empty row, in the last row, in a row that follows empty rows (and whose first entry also equals the entry before it),
    and in two rows at once.  -> (rowptr int32 [21], col int32)"""
    rows = dict(ROW_BOUNDARY_ROWS)
    rows.update(ROW_BOUNDARY_REPEATS[variant] if variant else {})
    n = 20
    rowptr = np.zeros(n + 1, np.int32)
    col = []
    for v in range(n):
        col += rows.get(v, [])
        rowptr[v + 1] = len(col)
    return rowptr, np.array(col, np.int32)


def csr_of(rowptr, col):
    n = len(rowptr) - 1
    return sp.csr_matrix((np.ones(len(col)), col.astype(np.int64), rowptr.astype(np.int64)), shape=(n, n))
