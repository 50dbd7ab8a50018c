"""Seeded inputs shared by tests/test_halo_ops_mirror.py (CPU) and tests/test_gpu_halo_ops.py (GPU): the bitmaps, range layouts, row lists,
batches and shard layouts at which the halo bookkeeping of a sharded plan is held to tests/halo_ops_mirror.py.  The smallest shapes that
reach each edge: empty ranges first / in the middle / last, slot counts that are no multiple of 32, ranges of 1023 / 1024 / 1025 / 2049
words (bits_compact cuts ranges into blocks of 1024 words, never across a range), one bitmap of more than 1024 blocks (the second trip of
the block scan), listed rows of 0 / 1 / 63 / 64 / 65 / 200 entries (one wave of 64 lanes walks a row), batches around the 256 threads of
batch_prepare's workgroups and the 1024 of the SpMM workgroup that does the same job."""
import functools
import threading
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

import halo_ops_mirror as M

GUARD = 0xA5A5A5A5              # the word behind a bitmap's last one (buffers are woff[P] + 1 words): no kernel writes it
COMPACT_BLOCK_WORDS = 1024      # csrc/elementwise.hip kCompactWords
SPMM_THREADS = 1024             # csrc/spmm.hip kBalThreads

# slot counts per peer
LAYOUTS = {
    "one_word": (20,),
    "empty_first": (0, 33, 64, 1),
    "empty_middle": (33, 0, 64, 1),
    "empty_last": (33, 64, 1, 0),
    "all_empty": (0, 0, 0, 0),
    "block_edges": (1023 * 32 - 3, 1024 * 32, 1025 * 32 - 31, 2049 * 32 - 17),
}
PATTERNS = ("zero", "one", "bit0", "bit31", "random")
FORMS = ("map", "add")
CLEAR_EDGES = (0, 1, 31, 32, 33, 63, 64, 95)
CLEAR_SPANS = ((5, 5 + 257 * 32 + 9), (37, 37 + 8193), (64, 64 + 8192 + 32 * 300))     # 257 words; 8193 bits; several workgroups, whole words
COPY_WIDTHS = (16, 48, 256, 1024)
COPY_COUNTS = (0, 1, 17, 1000)
PREP_BATCHES = tuple(sorted({1, 255, 256, 257, SPMM_THREADS - 1, SPMM_THREADS, SPMM_THREADS + 1, 2048}))


def layout(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return off, M.word_offsets(off)


def with_guard(words):
    return np.concatenate([np.asarray(words, np.uint32), np.array([GUARD], np.uint32)])


def pattern_words(off, woff, pattern, seed=0):
    """a bitmap over the ranges with clear padding bits"""
    rng = np.random.RandomState(9100 + seed)
    words = np.zeros(int(woff[-1]), np.uint32)
    for q in range(len(off) - 1):
        nb, nw = int(off[q + 1] - off[q]), int(woff[q + 1] - woff[q])
        pos = np.arange(nw * 32)
        b = {"zero": np.zeros(nw * 32, bool), "one": np.ones(nw * 32, bool), "bit0": pos % 32 == 0, "bit31": pos % 32 == 31,
             "random": rng.rand(nw * 32) < 0.5}[pattern]
        words[woff[q]:woff[q + 1]] = M.from_bool(b & (pos < nb), nw)
    return words


@functools.lru_cache(maxsize=None)
def compact_case(name, pattern, form):
    off, woff = layout(LAYOUTS[name])
    words = pattern_words(off, woff, pattern, seed=len(name))
    n_slots = int(off[-1])
    rng = np.random.RandomState(9200)
    slot_map = rng.permutation(max(n_slots, 1)).astype(np.int32) + 7 if form == "map" else None      # (a non-null map for no slots)
    return SimpleNamespace(P=len(off) - 1, off=off, woff=woff, words=words, slot_map=slot_map, add=0 if form == "map" else 1000, n_slots=n_slots)


@functools.lru_cache(maxsize=None)
def compact_big():
    """P = 2, 1024 * 1024 + 1 words + 3 words: 1025 + 1 blocks, so the scan takes two trips and carries the first trip's total.  The first
    block and the last two (the one-word tail of range 0, range 1) are dense, about one bit per thousand elsewhere: ~67 k entries."""
    n0 = COMPACT_BLOCK_WORDS * 1024 + 1
    off, woff = layout((n0 * 32 - 5, 70))
    rng = np.random.RandomState(9300)
    words = np.zeros(int(woff[-1]), np.uint32)
    at = rng.randint(0, n0 * 32 - 5, size=n0 * 32 // 1000)
    np.bitwise_or.at(words, at >> 5, (np.uint32(1) << (at & 31).astype(np.uint32)))
    words[:COMPACT_BLOCK_WORDS] = 0xFFFFFFFF
    words[n0 - 1] = (1 << 27) - 1                     # 32 - 5 slots
    words[n0:] = M.from_bool(np.ones(70, bool), 3)
    return SimpleNamespace(P=2, off=off, woff=woff, words=words, slot_map=None, add=12345, n_slots=int(off[-1]))


def background(n_words, seed):
    return np.random.RandomState(9400 + seed).randint(0, 2 ** 32, size=n_words, dtype=np.uint64).astype(np.uint32)


# ---- halo_need_mark ------------------------------------------------------------------------------------------------------------------
NEED_LAYOUTS = {"empty_first": (0, 33, 64, 1), "empty_middle": (33, 0, 64, 1), "empty_last": (33, 64, 1, 0)}
NEED_ROW_LENS = (0, 1, 63, 64, 65, 200)           # rows 0 .. 5
NEED_N = 300


@functools.lru_cache(maxsize=None)
def need_case(name, halo=True):
    """300 own rows x (300 + 98) columns.  Rows 0-5 hold NEED_ROW_LENS entries (halo columns at every lane position, also in the second
    and fourth trip of the wave's loop); row 6 the first and last slot of every owner; row 7 only the first slot behind an empty range
    (or slot 0); the others 0-8 random entries.  halo=False: no column behind the own ones."""
    off, woff = layout(NEED_LAYOUTS[name])
    n, H = NEED_N, int(off[-1])
    rng = np.random.RandomState(9500 + len(name))
    n_cols = n + H
    rows = []
    for r in range(n):
        if r < len(NEED_ROW_LENS):
            k = NEED_ROW_LENS[r]
            c = np.sort(rng.choice(n_cols, k, replace=False)) if k != 1 else np.array([n + off[-1] - 1])
        elif r == 6:
            c = np.unique(np.concatenate([[n + off[q], n + off[q + 1] - 1] for q in range(len(off) - 1) if off[q + 1] > off[q]]))
        elif r == 7:
            empty = [q for q in range(len(off) - 1) if off[q + 1] == off[q] and off[q] < H]
            c = np.array([n + (off[empty[0]] if empty else 0)])
        else:
            c = np.sort(rng.choice(n_cols, rng.randint(0, 9), replace=False))
        rows.append(np.asarray(c, np.int64))
    if not halo:
        rows = [c[c < n] for c in rows]
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(c) for c in rows])
    indices = np.concatenate(rows).astype(np.int32)
    a = sp.csr_matrix((np.ones(len(indices), np.float32), indices, indptr), shape=(n, n_cols))
    lists = {"b1": np.array([6]), "b1_far": np.array([7]), "b5": np.array([1, -1, 4, 0, 6]), "b8": np.array([2, 3, -1, 5, 7, -1, 0, 1]),
             "b8_peers": np.full(8, -1), "b301": np.where(rng.rand(301) < 0.2, -1, rng.randint(0, n, 301))}
    return SimpleNamespace(a=a, n=n, H=H, P=len(off) - 1, off=off, woff=woff, lists={k: v.astype(np.int32) for k, v in lists.items()})


# ---- row copies ----------------------------------------------------------------------------------------------------------------------
def odd_floats(rng, *shape):
    """fp32 rows whose bit patterns a copy must keep: normal numbers, NaNs with payloads, infinities, denormals, both zeros"""
    x = rng.randn(*shape).astype(np.float32)
    u = x.view(np.uint32).reshape(-1)
    k = rng.randint(0, 6, size=u.size)
    pay = rng.randint(1, 1 << 22, size=u.size).astype(np.uint32)
    u[k == 0] = np.uint32(0x7FC00000) | pay[k == 0]          # quiet NaNs with payloads
    u[k == 1] = np.uint32(0xFF800001) + pay[k == 1]          # signalling NaNs, negative
    u[k == 2] = pay[k == 2]                                  # denormals
    u[(k == 3) & (pay < 1 << 20)] = 0x80000000               # -0
    return x


# ---- batch preparation ---------------------------------------------------------------------------------------------------------------
PREP_N = 5000                     # nodes of the whole graph
PREP_WINDOWS = {"window": (1200, 1500), "empty": (1200, 0), "whole": (0, PREP_N)}


@functools.lru_cache(maxsize=None)
def prep_case(b, window="window", mapped=True, with_gid2op=True):
    """b distinct node ids with members below lo, inside [lo, lo + nl) -- its first and last row among them -- and at or above lo + nl (from
    3 members on); a node map that permutes the ids; gid2op: own rows -> [0, nl), a third of the others -> halo rows behind them, -1 for the
    rest.  n_op = rows of the position map."""
    lo, nl = PREP_WINDOWS[window]
    rng = np.random.RandomState(9600 + b)
    ids = rng.choice(PREP_N, b, replace=False)
    must = list(dict.fromkeys(v for v in (lo, lo + nl - 1, lo - 1, lo + nl, 0, PREP_N - 1) if 0 <= v < PREP_N))
    must = [lo - 1, lo + nl - 1, lo + nl][:b] if 3 <= b < len(must) and nl > 0 else must
    if b >= len(must):
        rest = ids[~np.isin(ids, must)]
        ids = rng.permutation(np.concatenate([must, rest[:b - len(must)]]))
    elif nl > 0:
        ids[0] = lo + nl - 1
    node_map = rng.permutation(PREP_N).astype(np.int32) if mapped else None
    idx = (np.argsort(node_map)[ids] if mapped else ids).astype(np.int32)        # node_map[idx] = ids
    gid2op, n_op = None, max(nl, 1)
    if with_gid2op:
        gid2op = np.full(PREP_N, -1, np.int32)
        gid2op[lo:lo + nl] = np.arange(nl)
        remote = np.flatnonzero((np.arange(PREP_N) < lo) | (np.arange(PREP_N) >= lo + nl))
        remote = remote[rng.rand(len(remote)) < 1 / 3]
        gid2op[remote] = nl + np.arange(len(remote))
        n_op = nl + len(remote)
    return SimpleNamespace(b=b, idx=idx, node_map=node_map, lo=lo, nl=nl, gid2op=gid2op, n_op=max(n_op, 1))


@functools.lru_cache(maxsize=None)
def prep_matrix():
    """the matrix of the SpMM launch that carries the batch preparation: 700 rows, one row of 500 entries, a tenth of the rows empty"""
    rng = np.random.RandomState(9700)
    n = 700
    deg = rng.randint(1, 9, size=n)
    deg[rng.rand(n) < 0.1] = 0
    deg[3] = 500
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum(deg)
    indices = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in deg]).astype(np.int32)
    return sp.csr_matrix(((rng.rand(indptr[-1]) + 0.1).astype(np.float32), indices, indptr), shape=(n, n))


# ---- scatter ----------------------------------------------------------------------------------------------------------------------------
SCATTER_MODES = ("neither", "negative", "keep", "both")


@functools.lru_cache(maxsize=None)
def scatter_case(d, b, mode):
    rng = np.random.RandomState(9800 + d + b)
    n = 400
    rows = rng.choice(n, b, replace=False).astype(np.int32)
    keep = np.ones(b, np.float32)
    pos_ids = rng.choice(n + 50, b, replace=False).astype(np.int32)
    if mode in ("negative", "both"):
        rows[rng.rand(b) < 0.4] = -1
        rows[0] = -1
    if mode in ("keep", "both"):
        keep[rng.rand(b) < 0.4] = 0.0
        keep[-1] = 0.0
    if b > 1:
        pos_ids[rng.rand(b) < 0.2] = -1
    return SimpleNamespace(d=d, b=b, n=n, n_pos=n + 50, rows=rows, keep=keep, pos_ids=pos_ids, src=rng.randn(b, d).astype(np.float32),
                           dst=rng.randn(n, d).astype(np.float32))


# ---- the product's own shard layouts, built on the CPU ---------------------------------------------------------------------------------
class ThreadComm:
    """dist.Comm's setup-time methods for ranks that are threads of one process; the exchange is halo_ops_mirror.exchange_rows"""
    handle = None

    def __init__(self, shared, rank):
        self.shared, self.rank, self.world = shared, rank, shared.world

    def sync(self, timeout_s=None):
        pass

    def _meet(self, item):
        self.shared.slot[self.rank] = item
        self.shared.barrier.wait()
        every = list(self.shared.slot)
        self.shared.barrier.wait()
        return every

    def allgather_bytes(self, src):
        import torch
        return torch.cat([t.reshape(-1) for t in self._meet(src.contiguous().clone())])

    def exchange_rows(self, d, send, send_off, recv, recv_off):
        import torch
        every = self._meet((send.numpy().copy(), np.asarray(send_off, np.int64), recv.numpy().copy(), np.asarray(recv_off, np.int64)))
        new = M.exchange_rows([e[0] for e in every], [e[1] for e in every], [e[2] for e in every], [e[3] for e in every], d)
        recv.copy_(torch.from_numpy(new[self.rank]))


@functools.lru_cache(maxsize=None)
def shard_layouts(world=3, n=240, seed=9900):
    """gcn_drug_repurposing_amd.shards.build_shard on `world` ranks (threads, numpy device ops of tests/cpu_ops.py) over a random symmetric
    graph -> per rank: a (scipy, local column ids: own rows first, then the halo), n = own rows, recv_off / send_off / send_rows of A_hat's
    halo and their word offsets"""
    from cpu_ops import NumpyShardOps
    from gcn_drug_repurposing_amd.shards import ScipySource, build_shard
    rng = np.random.RandomState(seed)
    r, c = rng.randint(0, n, 3 * n), rng.randint(0, n, 3 * n)
    adj = sp.csr_matrix((np.ones(len(r)), (r, c)), shape=(n, n))
    adj = ((adj + adj.T) > 0).astype(np.float64)
    shared = SimpleNamespace(world=world, slot=[None] * world, barrier=threading.Barrier(world, timeout=120))
    out, errors = [None] * world, []

    def run(rank):
        try:
            sh = build_shard(ScipySource(adj), ThreadComm(shared, rank), need_transpose=False, device="cpu", relabel=False, ops=NumpyShardOps(),
                             split=False, local_transpose=False)
            h = sh.layout.halo_a
            a = sp.csr_matrix(sh.a.m)
            a.sort_indices()
            n_send = int(h.send_off[-1])
            out[rank] = SimpleNamespace(rank=rank, a=a, n=h.nl, lo=h.lo, n_halo=h.n_halo, recv_off=h.recv_off.copy(), send_off=h.send_off.copy(),
                                        send_rows=h.send_rows.numpy()[:n_send].astype(np.int32), wrecv_off=M.word_offsets(h.recv_off),
                                        wsend_off=M.word_offsets(h.send_off), remote=h.remote.copy())
        except BaseException as e:          # a rank that fails must not leave the others at the barrier
            errors.append(e)
            shared.barrier.abort()

    threads = [threading.Thread(target=run, args=(k,)) for k in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return out
