"""Inputs of the op-by-op tests of the network proximity kernels (tests/test_proximity_mirror.py on the CPU,
tests/test_gpu_proximity_ops.py on the GPU): named, tiny, deterministic, each with the property it exists for.
tests/test_proximity_mirror.py asserts those properties on the mirror alone -- a seed that loses one fails there, not on the GPU.

Graphs (graph(name) -> n, rowptr, col of the symmetric CSR; distances(name) -> scipy's BFS as the uint8 matrix apsp_kernel must equal):
  single                 one node, no edge;
  split_511 / 512 / 513  sparse random, two components and isolated nodes, n around apsp_kernel's 512-thread stride;
  star_600               a hub of degree 599 (above one pass of the 512 threads), the hub in the middle of the numbering;
  path_255, path_256     254 hops (accepted, the corner byte is 254) and 255 hops (refused);
  web_300, web_132       a ring with random chords: connected, the general-purpose graphs of the set and score cases;
  web_4100               the same at the size the ns = 4096 case needs;
  cycle_150, complete_130, complete_40, double_star      symmetric graphs for the tied centres and the zero spread.

Random-set cases (RANDOM_CASES): bins and sets stated directly, as the C entry point takes them.
Set-stats cases (SET_CASES): lists of sets on a graph; the table is padded with empty sets to n_samples = 3 and to a max_size above every size.
Score cases (SCORE_CASES): a from table and a to table (hand-made here, or the mirror's random tables), a pair list or None, a measure mask.
Every set stays inside one component.  Mirror results are computed once and shared; treat every array as read-only."""
import functools
import types

import numpy as np

import proximity_mirror as M

SEED = 452456
ALL = M.MEASURES
MASK = {m: 1 << i for i, m in enumerate(M.MEASURES)}


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------

def _csr(n, edges):
    """undirected edge list -> (n, rowptr, col) int32, symmetric, no self loops, no duplicates, columns ascending"""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    a, b = np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]])
    key = np.unique(a * n + b)
    a, b = key // n, key % n
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(a, minlength=n), out=rowptr[1:])
    return types.SimpleNamespace(n=n, rowptr=rowptr, col=b.astype(np.int32))


def _web(n, chords, seed):
    rng = np.random.RandomState(seed)
    ring = np.arange(n)
    return _csr(n, np.concatenate([np.stack([ring, (ring + 1) % n], 1), rng.randint(0, n, (chords, 2))]))


def _split(n, seed):
    """two random components (a spanning tree each + a few more edges) over a shuffled numbering; every 37th node isolated"""
    rng = np.random.RandomState(seed)
    isolated = np.arange(5, n, 37)
    rest = rng.permutation(np.setdiff1d(np.arange(n), isolated))
    cut = len(rest) * 2 // 3
    edges = []
    for part in (rest[:cut], rest[cut:]):
        for i in range(1, len(part)):
            edges.append((part[i], part[rng.randint(0, i)]))
        edges += [(part[a], part[b]) for a, b in rng.randint(0, len(part), (len(part) // 3, 2))]
    g = _csr(n, edges)
    g.isolated, g.parts = isolated, (np.sort(rest[:cut]), np.sort(rest[cut:]))
    return g


STAR_HUB = 301
DS_A, DS_B, DS_FIRST = 68, 69, 5     # double_star: the hubs' node numbers; its tie set starts at node 5, so they sit at positions 63 and 64


def _double_star():
    """hubs a - b, every other node a leaf of one of them.  The tie set (nodes 5 .. 106) holds 50 leaves of each hub, so a and b --
    and no other member -- have the smallest summed distance; nodes 0 .. 4 and 107 .. 111 are leaves outside the set"""
    n = 112
    leaves = [v for v in range(n) if v not in (DS_A, DS_B)]
    inside = [v for v in leaves if DS_FIRST <= v <= 106]
    assert len(inside) == 100
    edges = [(DS_A, DS_B)]
    for k, v in enumerate(inside):
        edges.append((v, DS_A if k % 2 == 0 else DS_B))
    for v in leaves:
        if v not in inside:
            edges.append((v, DS_A))
    return _csr(n, edges)


_GRAPHS = {
    "single": lambda: _csr(1, np.zeros((0, 2))),
    "split_511": lambda: _split(511, 11),
    "split_512": lambda: _split(512, 12),
    "split_513": lambda: _split(513, 13),
    "star_600": lambda: _csr(600, [(STAR_HUB, v) for v in range(600) if v != STAR_HUB]),
    "path_255": lambda: _csr(255, [(i, i + 1) for i in range(254)]),
    "path_256": lambda: _csr(256, [(i, i + 1) for i in range(255)]),
    "web_300": lambda: _web(300, 150, 21),
    "web_132": lambda: _web(132, 40, 22),
    "web_4100": lambda: _web(4100, 4100, 23),
    "cycle_150": lambda: _csr(150, [(i, (i + 1) % 150) for i in range(150)]),
    "complete_130": lambda: _csr(130, [(i, j) for i in range(130) for j in range(i)]),
    "complete_40": lambda: _csr(40, [(i, j) for i in range(40) for j in range(i)]),
    "double_star": _double_star,
}
APSP_CASES = ["single", "split_511", "split_512", "split_513", "star_600", "path_255", "web_132"]
APSP_REFUSED = "path_256"


@functools.lru_cache(maxsize=None)
def graph(name):
    return _GRAPHS[name]()


@functools.lru_cache(maxsize=None)
def distances(name):
    g = graph(name)
    D = np.concatenate([M.bfs_rows(g.rowptr, g.col, np.arange(c, min(c + 512, g.n))) for c in range(0, g.n, 512)])
    D.setflags(write=False)
    return D


def diameter(name):
    """the largest FINITE hop count"""
    D = distances(name)
    return int(D[D != 255].max())


def dist(name):
    return M.matrix_dist(distances(name))


# ---- random sets ------------------------------------------------------------------------------------------------------------------------

def _bins(n, groups):
    """bins stated as node lists -> (bin_list ascending int64 arrays, node_bin)"""
    bl = [np.array(sorted(g), np.int64) for g in groups]
    assert sorted(np.concatenate(bl).tolist()) == list(range(n))
    return bl, M.bin_of(bl, n)


def _exhaust_bins():
    a = np.arange(3, 132, 4)[:32]                                   # 32 nodes scattered over the numbering
    return _bins(132, [a, np.setdiff1d(np.arange(132), a)])


def _mixed_bins():
    rng = np.random.RandomState(5)
    rest = rng.permutation(np.setdiff1d(np.arange(132), [17]))
    return _bins(132, [[17], rest[:30], rest[30:70], rest[70:]])


def _random_case(name, why, bins, sets, n_random):
    bl, nb = bins
    sets = [np.array(sorted(s), np.int64) for s in sets]
    return types.SimpleNamespace(name=name, why=why, graph="web_132", n=132, bin_list=bl, node_bin=nb, sets=sets, n_random=n_random,
                                 max_size=max(1, max(len(s) for s in sets)), seed=SEED)


def _random_cases():
    eb, mb = _exhaust_bins(), _mixed_bins()
    b0, b1 = eb[0]
    exhaust_sets = [b0, b1[[2, 30, 31, 64, 99]], [], b0[5:25], b1[::2]]
    m = mb[0]
    mixed_sets = [[17], m[1][[0, 7]], [], np.concatenate([m[1][[3, 9, 20]], m[2][[0, 1, 17, 39]], m[3][[5, 6, 7, 8, 60]]]),
                  np.concatenate([[17], m[1][[4, 5]]])]
    return [
        _random_case("exhaust", "set 0 holds all 32 nodes of a 32-node bin: most samples run out of redraws and shrink, some keep all 32; "
                     "5 sets x 65 samples = 325 threads, a second block", eb, exhaust_sets, 64),
        _random_case("mixed", "a bin of one node that is the member, an empty set between two others, a set over three bins", mb, mixed_sets, 20),
        _random_case("n_random_0", "only the sets themselves are written", mb, mixed_sets, 0),
    ]


_RANDOM = {c.name: c for c in _random_cases()}
RANDOM_CASES = list(_RANDOM)


def random_case(name):
    return _RANDOM[name]


@functools.lru_cache(maxsize=None)
def random_table(name, side, ablate=None):
    c = random_case(name)
    return M.random_table(c.sets, c.node_bin, c.bin_list, c.seed, side, c.n_random, ablate)


# ---- set stats --------------------------------------------------------------------------------------------------------------------------

SET_SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 200)


def _set_cases():
    rng = np.random.RandomState(9)
    sizes = [np.sort(rng.choice(300, k, replace=False)) for k in SET_SIZES]
    hub_in = np.concatenate([np.arange(200, 270), [STAR_HUB], np.arange(400, 430)])       # the hub at position 70: the second ballot chunk
    mk = lambda name, why, g, sets: types.SimpleNamespace(name=name, why=why, graph=g, sets=[np.asarray(s, np.int64) for s in sets])  # noqa: E731
    return [
        mk("sizes", "0, 1, 2 members and both sides of 64 and 128", "web_300", sizes),
        mk("cycle_tied", "the whole cycle: every member a centre, 150 over three ballot chunks", "cycle_150", [np.arange(150)]),
        mk("complete_tied", "129 of 130 mutually adjacent nodes: every member a centre, inner = 1", "complete_130",
           [np.setdiff1d(np.arange(130), [40]), np.arange(3, 68)]),
        mk("star", "one centre, the hub, in the second ballot chunk; a set of leaves only (all tied)", "star_600", [hub_in, np.arange(10, 80)]),
        mk("tie_63_64", "exactly two tied centres, at positions 63 and 64: either side of the ballot chunks' boundary", "double_star",
           [np.arange(DS_FIRST, 107)]),
    ]


_SETS = {c.name: c for c in _set_cases()}
SET_CASES = list(_SETS)
SET_SAMPLES = 3


def set_case(name):
    return _SETS[name]


def table_arrays(table, max_size, pad=-1):
    """set table (list of lists of arrays) -> (nodes [n_sets, R, max_size] int32 padded with `pad`, sizes [n_sets, R] int32)"""
    R = len(table[0])
    nodes = np.full((len(table), R, max_size), pad, np.int32)
    sizes = np.zeros((len(table), R), np.int32)
    for i, rows in enumerate(table):
        assert len(rows) == R
        for r, x in enumerate(rows):
            nodes[i, r, :len(x)] = x
            sizes[i, r] = len(x)
    return nodes, sizes


def set_table(name):
    """the case's sets as a table of SET_SAMPLES samples per row (padded with empty sets) and its max_size (above every size)"""
    sets = list(set_case(name).sets)
    while len(sets) % SET_SAMPLES:
        sets.append(np.zeros(0, np.int64))
    table = [sets[i:i + SET_SAMPLES] for i in range(0, len(sets), SET_SAMPLES)]
    return table, max(len(s) for s in sets) + 10


@functools.lru_cache(maxsize=None)
def set_mirror(name, ablate=None):
    table, _ = set_table(name)
    return M.stats_table(dist(set_case(name).graph), table, ablate)


# ---- score ------------------------------------------------------------------------------------------------------------------------------

FROM_SIZES, TO_SIZES = (1, 26, 64, 65, 130), (1, 63, 64, 65, 257)
BIG_TO = (4096, 2500, 1500)       # lds_4096: the to set and its two samples (sizes far apart, so that two samples give a spread)
GRID_PAIRS = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (4, 0), (2, 3), (3, 2), (1, 4), (4, 1)]


def _subsets(rng, n, size, samples):
    """sample 0 and `samples` - 1 further random subsets of [0, n); every second further one a member short (a size of its own)"""
    out = []
    for r in range(samples):
        k = size - 1 if (r % 2 == 0 and r > 0 and size > 1) else size
        out.append(np.sort(rng.choice(n, k, replace=False)).astype(np.int64))
    return out


def _score(name, why, g, ftab, ttab, pairs, which=ALL, to_max_size=None, from_max_size=None):
    fm = from_max_size or max(1, max(len(x) for rows in ftab for x in rows))
    tm = to_max_size or max(1, max(len(x) for rows in ttab for x in rows))
    return types.SimpleNamespace(name=name, why=why, graph=g, ftab=ftab, ttab=ttab, pairs=pairs, which=tuple(which), from_max_size=fm,
                                 to_max_size=tm, n_samples=len(ftab[0]))


def _score_cases():
    rng = np.random.RandomState(33)
    gf = [_subsets(rng, 300, k, 6) for k in FROM_SIZES]
    gt = [_subsets(rng, 300, k, 6) for k in TO_SIZES]
    big_f = [_subsets(rng, 4100, k, 3) for k in (3, 70)]
    big_t = [[np.sort(rng.choice(4100, k, replace=False)).astype(np.int64) for k in BIG_TO]]
    ex_f, ex_t = random_table("exhaust", 0), random_table("exhaust", 1)
    keep = [0, 1, 3, 4]                                                # without the empty set
    emp = np.zeros(0, np.int64)
    e_f = [gf[1][:3], [emp] * 3, gf[2][:3]]
    e_t = [[emp] * 3, gt[1][:3], gt[3][:3]]
    c40 = random_sd0_tables()
    return [
        _score("grid", "nt in 1..130 against ns in 1..257 over both sides of the 64-lane stride, sizes that differ between samples; "
               "11 pairs x 6 samples = 66 waves, a tail block half idle", "web_300", gf, gt, GRID_PAIRS, to_max_size=260, from_max_size=131),
        _score("grid_all", "pairs = NULL: every from set against every to set, q = i * n_to + j; 3 x 2 x 3 = 18 waves", "web_300",
               [rows[:3] for rows in gf[:3]], [rows[:3] for rows in gt[2:4]], None),
        _score("pairs_unordered", "a pair list out of order that repeats a pair", "web_300", gf, gt, [(4, 1), (0, 0), (4, 1), (2, 3), (1, 0)],
               to_max_size=260),
        _score("lds_4096", "ns = 4096 at max_size = 4096: the whole of a wave's column minima in LDS, then 2500 and 1500; 6 waves", "web_4100",
               big_f, big_t, None,
               to_max_size=4096),
        _score("exhaust", "the random tables of the `exhaust` sets: per-sample sizes differ from sample 0's", "web_132",
               [ex_f[i] for i in keep], [ex_t[i] for i in keep], [(0, 0), (0, 1), (1, 0), (2, 3), (3, 2), (1, 1), (3, 0)]),
        _score("empties", "an empty from set and an empty to set among others: NaN in exactly their pairs", "web_300", e_f, e_t, None),
        _score("sd0", "complete graph, from bin and to bin disjoint: every cross distance is 1, so closest, shortest and center are 1 and "
               "separation 0 in every sample", "complete_40", c40[0], c40[1], None, which=("closest", "shortest", "center", "separation")),
        _score("batch7", "7 pairs for the batch loop (prox_batch_pairs 1, 2, 3, 7)", "web_300", gf, gt, GRID_PAIRS[:7]),
    ]


def random_sd0_tables():
    bl, nb = _bins(40, [np.arange(20), np.arange(20, 40)])
    f = M.random_table([np.array([1, 4, 9, 12, 18]), np.array([0, 19])], nb, bl, SEED, 0, 8)
    t = M.random_table([np.array([20, 22, 25, 29, 33, 36, 39]), np.array([21, 30, 38])], nb, bl, SEED, 1, 8)
    return f, t


_SCORE = {c.name: c for c in _score_cases()}
SCORE_CASES = list(_SCORE)


def score_case(name):
    return _SCORE[name]


def pair_list(c):
    if c.pairs is not None:
        return list(c.pairs)
    return [(i, j) for i in range(len(c.ftab)) for j in range(len(c.ttab))]


@functools.lru_cache(maxsize=None)
def score_stats(name, ablate=None):
    """(from statistics, to statistics) of the case's tables from the set-stats mirror"""
    c = score_case(name)
    d = dist(c.graph)
    return M.stats_table(d, c.ftab, ablate), M.stats_table(d, c.ttab, ablate)


@functools.lru_cache(maxsize=None)
def score_values(name, ablate=None, which=None):
    c = score_case(name)
    fs, ts = score_stats(name, ablate if ablate in ("first_centre", "inner_self", "inner_single", "stats_first64") else None)
    v = M.score_values(dist(c.graph), c.ftab, c.ttab, fs, ts, pair_list(c), which or c.which, ablate, c.to_max_size)
    v.setflags(write=False)
    return v


def score_mirror(name, ablate=None, which=None, batch=None, fill=np.nan):
    """out [n_pairs, 5, 5] of the mirror"""
    return M.score_out(score_values(name, ablate, which), batch, ablate, fill)


# which case shows which wrong rule, and in which output (tests/test_proximity_mirror.py measures the margins)
ABLATION_CASE = {
    "first_centre": ("set", "cycle_tied"),
    "inner_self": ("set", "sizes"),
    "inner_single": ("set", "sizes"),
    "stats_first64": ("set", "sizes"),
    "colmin_first64": ("score", "grid"),
    "kernel_max_size": ("score", "grid"),
    "redraws_19": ("random", "exhaust"),
    "redraws_21": ("random", "exhaust"),
    "add_taken": ("random", "exhaust"),
    "unsorted": ("random", "exhaust"),
    "pair_sample0": ("score", "grid"),
    "sample_sd": ("score", "grid"),
    "drop_p0": ("score", "batch7"),
}
