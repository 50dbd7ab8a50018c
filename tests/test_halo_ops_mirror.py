"""CPU: tests/halo_ops_mirror.py -- the numpy contract that tests/test_gpu_halo_ops.py holds the halo bookkeeping kernels to -- is itself
held to brute force (bit-by-bit Python loops over the same seeded cases, tests/halo_ops_cases.py), to the contracts it must refuse to
mirror (a set padding bit, two writers of one row), and to the PRODUCT's shard layout: for a graph sharded by shards.build_shard on three
ranks, need bitmap -> exchange -> list must name exactly the boundary rows the listed rows reference, in slot order, on both sides."""
import numpy as np
import pytest

import halo_ops_cases as K
import halo_ops_mirror as M


def bit(words, i):
    return (int(words[i >> 5]) >> (i & 31)) & 1


# ================================================================ bitmaps
def test_bool_round_trip_and_word_offsets():
    w = K.background(7, 1)
    assert np.array_equal(M.from_bool(M.to_bool(w)), w)
    assert [int(M.to_bool(w)[i]) for i in range(224)] == [bit(w, i) for i in range(224)]
    assert M.word_offsets([0, 0, 33, 97, 98]).tolist() == [0, 0, 2, 4, 5]
    assert M.word_offsets([0, 32, 32, 33]).tolist() == [0, 1, 1, 2]


@pytest.mark.parametrize("form", K.FORMS)
@pytest.mark.parametrize("pattern", K.PATTERNS)
@pytest.mark.parametrize("name", list(K.LAYOUTS))
def test_compact_equals_a_walk_over_the_bits(name, pattern, form):
    cs = K.compact_case(name, pattern, form)
    lst, out_off = M.bits_compact(cs.words, cs.woff, cs.off, cs.slot_map, cs.add)
    want, want_off = [], [0]
    for q in range(cs.P):
        for j in range(int(cs.off[q + 1] - cs.off[q])):
            if bit(cs.words, int(cs.woff[q]) * 32 + j):
                slot = int(cs.off[q]) + j
                want.append(int(cs.slot_map[slot]) if cs.slot_map is not None else slot + cs.add)
        want_off.append(len(want))
    assert lst.dtype == np.int32 and out_off.dtype == np.int64
    assert lst.tolist() == want and out_off.tolist() == want_off
    if pattern == "one":
        assert len(want) == cs.n_slots          # every slot once: no padding bit, no slot of a neighbouring range
    if name == "all_empty":
        assert len(lst) == 0 and not out_off.any()


def test_compact_big_case_has_more_than_1024_blocks_and_a_short_list():
    cs = K.compact_big()
    nblk = int(((np.diff(cs.woff) + K.COMPACT_BLOCK_WORDS - 1) // K.COMPACT_BLOCK_WORDS).sum())
    assert nblk == 1026 and cs.woff[1] == 1024 * 1024 + 1 and len(cs.words) * 4 < 4.2e6
    lst, out_off = M.bits_compact(cs.words, cs.woff, cs.off, None, cs.add)
    assert 32768 + 27 + 70 < len(lst) < 120000 and out_off[2] - out_off[1] == 70
    assert (np.diff(lst) > 0).all() and lst[0] == cs.add and lst[-1] == cs.add + cs.n_slots - 1
    # the blocks of the scan's second trip hold entries, and so do blocks in the middle of the first
    assert lst[out_off[1] - 1] == cs.add + cs.off[1] - 1
    per_block = np.add.reduceat(M.to_bool(cs.words[:cs.woff[1] - 1]).reshape(-1, 32).sum(1), np.arange(0, 1024 * 1024, 1024))
    assert per_block[0] == 32768 and (per_block[1:] > 0).sum() > 1000


@pytest.mark.parametrize("op", ["clear", "fill"])
def test_clear_and_fill_equal_a_walk_over_the_bits(op):
    spans = [(f, l) for f in K.CLEAR_EDGES for l in K.CLEAR_EDGES] + list(K.CLEAR_SPANS)
    for k, (first, last) in enumerate(spans):
        bg = K.background(M.words_for(max(last, 96)) + 1, k)
        got = (M.bits_clear if op == "clear" else M.bits_fill)(bg, first, last)
        n_bits = len(bg) * 32
        probe = range(n_bits) if n_bits <= 512 else list(range(max(first - 70, 0), first + 70)) + list(range(last - 70, min(last + 70, n_bits)))
        for i in probe:
            assert bit(got, i) == ((1 if op == "fill" else 0) if first <= i < last else bit(bg, i)), (first, last, i)
        inside = np.zeros(n_bits, bool)
        inside[first:max(last, first)] = True
        assert np.array_equal(M.to_bool(got)[~inside], M.to_bool(bg)[~inside])
        assert (M.to_bool(got)[inside] == (op == "fill")).all()
        if last <= first:
            assert np.array_equal(got, bg)


def test_set_list_sets_exactly_the_listed_bits():
    bg = K.background(20, 3) & np.uint32(0x0F0F0F0F)
    for ids in ([], [0], [639], list(range(64, 96)), [5, 5, 5, 37, 5], list(np.random.RandomState(1).randint(0, 640, 257))):
        got = M.bits_set_list(bg, ids)
        for i in range(640):
            assert bit(got, i) == (1 if i in set(ids) else bit(bg, i))


@pytest.mark.parametrize("counts", [(33, 0, 64, 1), (0, 0), (32,), (1, 1, 1)])
def test_send_slot_bits_equals_a_walk_over_the_slots(counts):
    off, woff = K.layout(counts)
    rng = np.random.RandomState(sum(counts))
    bits = K.background(10, 5)
    send_rows = rng.randint(0, 320, size=int(off[-1]))           # rows repeat: one row goes to several peers
    got = M.send_slot_bits(bits, send_rows, off)
    assert len(got) == woff[-1]
    M.check_ranges(got, off, woff)
    for q in range(len(counts)):
        for j in range(counts[q]):
            assert bit(got, int(woff[q]) * 32 + j) == bit(bits, int(send_rows[off[q] + j]))


@pytest.mark.parametrize("name", list(K.NEED_LAYOUTS))
def test_need_marks_are_the_halo_columns_of_the_listed_rows(name):
    cs = K.need_case(name)
    for key, rows in cs.lists.items():
        need = M.halo_need_mark(cs.a.indptr, cs.a.indices, rows, cs.n, cs.off, np.zeros(int(cs.woff[-1]) + 1, np.uint32))
        M.check_ranges(need, cs.off, cs.woff)                # padding stays clear
        assert need[-1] == 0
        lst, out_off = M.bits_compact(need, cs.woff, cs.off, None, cs.n)
        cols = np.unique(np.concatenate([cs.a[r].indices for r in rows if r >= 0] + [np.zeros(0, np.int32)]))
        want = cols[cols >= cs.n]
        assert np.array_equal(lst, want), key                 # slot order = ascending column order
        assert out_off.tolist() == [int((want < cs.n + o).sum()) for o in cs.off], key
    # the edges the case is there for
    assert [len(cs.a[r].indices) for r in range(6)] == list(K.NEED_ROW_LENS)
    need = M.halo_need_mark(cs.a.indptr, cs.a.indices, [6], cs.n, cs.off, np.zeros(int(cs.woff[-1]), np.uint32))
    firsts_lasts = {int(cs.woff[q]) * 32 + j for q in range(cs.P) if cs.off[q + 1] > cs.off[q] for j in (0, int(cs.off[q + 1] - cs.off[q]) - 1)}
    assert set(np.flatnonzero(M.to_bool(need))) == firsts_lasts
    # marks accumulate: nothing is cleared
    again = M.halo_need_mark(cs.a.indptr, cs.a.indices, cs.lists["b5"], cs.n, cs.off, need)
    assert ((again & need) == need).all()
    flat = K.need_case(name, halo=False)
    assert not M.halo_need_mark(flat.a.indptr, flat.a.indices, flat.lists["b301"], flat.n, flat.off, np.zeros(int(flat.woff[-1]), np.uint32)).any()


# ================================================================ rows
def test_pack_and_unpack_copy_bits():
    rng = np.random.RandomState(4)
    src = K.odd_floats(rng, 50, 16)
    assert np.isnan(src).any() and (np.abs(src[np.isfinite(src)]) < 1e-38).any()
    rows = np.array([3, 3, 49, 0, 3])
    got = M.pack_rows(src, rows)
    for k, r in enumerate(rows):
        assert got[k].view(np.uint32).tolist() == src[r].view(np.uint32).tolist()
    dst = K.odd_floats(rng, 60, 16)
    back = M.unpack_rows(dst, got[:3], np.array([59, 0, 7]))
    for r in range(60):
        want = {59: got[0], 0: got[1], 7: got[2]}.get(r, dst[r])
        assert back[r].view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert M.pack_rows(src, np.zeros(0, np.int32)).shape == (0, 16)


def test_the_mirror_refuses_what_the_contracts_exclude():
    off, woff = K.layout((33, 1))
    words = K.pattern_words(off, woff, "one")
    M.check_ranges(words, off, woff)
    bad = words.copy()
    bad[1] |= np.uint32(2)                                       # bit 33 of range 0: padding
    with pytest.raises(AssertionError, match="padding"):
        M.bits_compact(bad, woff, off)
    with pytest.raises(AssertionError, match="padding"):
        M.halo_need_mark(np.zeros(2, np.int32), np.zeros(0, np.int32), [0], 1, off, bad)
    with pytest.raises(AssertionError, match="word-aligned"):
        M.bits_compact(words, np.array([0, 1, 2]), off)          # range 0 needs two words
    with pytest.raises(AssertionError, match="distinct"):
        M.unpack_rows(np.zeros((4, 4), np.float32), np.zeros((2, 4), np.float32), [1, 1])
    with pytest.raises(AssertionError, match="distinct"):
        M.scatter_add_rows(np.zeros((4, 4), np.float32), np.zeros((2, 4), np.float32), [1, 1], None)
    M.scatter_add_rows(np.zeros((4, 4), np.float32), np.zeros((2, 4), np.float32), [1, 1], np.array([1.0, 0.0]))     # one of them is skipped
    with pytest.raises(AssertionError, match="distinct"):
        M.batch_prepare([5, 5], None, 0, 10, None, np.full(10, -1, np.int32))
    M.batch_prepare([15, 15], None, 0, 10, None, np.full(10, -1, np.int32))        # members without a position may repeat


# ================================================================ batch preparation, scatter
@pytest.mark.parametrize("window", list(K.PREP_WINDOWS))
@pytest.mark.parametrize("with_gid2op", [False, True])
@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("b", [1, 5, 257])
def test_batch_prepare_equals_a_loop_over_the_members(b, mapped, with_gid2op, window):
    cs = K.prep_case(b, window, mapped, with_gid2op)
    pos0 = np.arange(cs.n_op, dtype=np.int32) - 10 ** 6
    got = M.batch_prepare(cs.idx, cs.node_map, cs.lo, cs.nl, cs.gid2op, pos0)
    pos = pos0.copy()
    regions = set()
    for i in range(b):
        node = int(cs.node_map[cs.idx[i]]) if mapped else int(cs.idx[i])
        rel = node - cs.lo
        mine = 0 <= rel < cs.nl
        regions.add("in" if mine else ("below" if rel < 0 else "above"))
        op = int(cs.gid2op[node]) if with_gid2op else (rel if mine else -1)
        assert got["rloc"][i] == (min(max(rel, 0), cs.nl - 1) if cs.nl else 0)
        assert got["pid"][i] == op and got["keep"][i] == float(mine) and got["rlist"][i] == (rel if mine else -1)
        if op >= 0:
            pos[op] = i
    assert np.array_equal(got["pos"], pos) and (pos0 < 0).all()
    assert (got["pos"] >= 0).sum() == (got["pid"] >= 0).sum()
    if b >= 5 and window == "window":
        assert regions == {"in", "below", "above"}
    if window == "empty":
        assert not got["keep"].any() and (got["rlist"] == -1).all() and not got["rloc"].any()


@pytest.mark.parametrize("mode", K.SCATTER_MODES)
def test_scatter_add_skips_members_but_resets_their_position(mode):
    cs = K.scatter_case(16, 333, mode)
    pos0 = np.arange(cs.n_pos, dtype=np.int32)
    dst, pos = M.scatter_add_rows(cs.dst, cs.src, cs.rows, cs.keep, pos0, cs.pos_ids)
    want, want_pos = cs.dst.copy(), pos0.copy()
    skipped_with_position = 0
    for r in range(cs.b):
        if cs.pos_ids[r] >= 0:
            want_pos[cs.pos_ids[r]] = -1
        if cs.rows[r] < 0 or cs.keep[r] == 0:
            skipped_with_position += int(cs.pos_ids[r] >= 0)
            continue
        want[cs.rows[r]] = want[cs.rows[r]] + cs.src[r]
    assert np.array_equal(dst.view(np.int32), want.view(np.int32)) and np.array_equal(pos, want_pos)
    assert (skipped_with_position > 0) == (mode != "neither")
    assert M.scatter_add_rows(cs.dst, cs.src, cs.rows, None)[1] is None


# ================================================================ the exchange, and the product's layout
def test_exchange_rows_moves_ranges_between_ranks():
    rng = np.random.RandomState(8)
    W, d = 3, 4
    counts = rng.randint(0, 5, size=(W, W))                      # counts[r][q]: r sends q
    np.fill_diagonal(counts, 0)
    send_off = [np.concatenate([[0], np.cumsum(counts[r])]) for r in range(W)]
    recv_off = [np.concatenate([[0], np.cumsum(counts[:, q])]) for q in range(W)]
    send = [rng.randn(int(send_off[r][-1]) + 2, d).astype(np.float32) for r in range(W)]
    recv = [np.full((int(recv_off[q][-1]) + 2, d), -7.0, np.float32) for q in range(W)]
    got = M.exchange_rows(send, send_off, recv, recv_off, d)
    for q in range(W):
        for r in range(W):
            for k in range(counts[r][q]):
                assert np.array_equal(got[q][recv_off[q][r] + k], send[r][send_off[r][q] + k])
        assert (got[q][recv_off[q][-1]:] == -7.0).all() and (recv[q] == -7.0).all()
    with pytest.raises(AssertionError, match="expects"):
        M.exchange_rows(send, send_off, recv, [recv_off[0], recv_off[1] + np.array([0, 0, 0, 1]), recv_off[2]], d)     # rank 1 expects a row more of rank 2


def lazy_request_phase(ranks, lists):
    """the receiver-driven request phase of every rank at once, by the mirror: -> per rank (recv_list, recv_cnt, send_list, send_cnt)"""
    need = [M.halo_need_mark(s.a.indptr, s.a.indices, lists[s.rank], s.n, s.recv_off, np.zeros(int(s.wrecv_off[-1]) + 1, np.uint32)) for s in ranks]
    req = M.exchange_words(need, [s.wrecv_off for s in ranks], [np.zeros(int(s.wsend_off[-1]) + 1, np.uint32) for s in ranks],
                           [s.wsend_off for s in ranks])
    out = []
    for s in ranks:
        recv_list, recv_cnt = M.bits_compact(need[s.rank], s.wrecv_off, s.recv_off, None, s.n)
        send_list, send_cnt = M.bits_compact(req[s.rank], s.wsend_off, s.send_off, s.send_rows, 0)
        out.append((recv_list, recv_cnt, send_list, send_cnt))
    return out


def test_request_phase_over_the_products_shard_layout_names_exactly_the_referenced_rows():
    ranks = K.shard_layouts(3)
    assert len(ranks) == 3 and all(s.n > 0 and s.n_halo > 0 for s in ranks)
    assert sum(s.n for s in ranks) == 240
    rng = np.random.RandomState(12)
    lists = [np.where(rng.rand(9) < 0.25, -1, rng.randint(0, s.n, 9)).astype(np.int32) for s in ranks]
    got = lazy_request_phase(ranks, lists)
    for s in ranks:
        recv_list, recv_cnt, send_list, send_cnt = got[s.rank]
        cols = np.unique(np.concatenate([s.a[r].indices for r in lists[s.rank] if r >= 0]))
        assert np.array_equal(recv_list, cols[cols >= s.n])                 # exactly the referenced boundary rows, in slot order
        assert 0 < len(recv_list) < s.n_halo                                # a true subset: over-fetching would show
        for q in ranks:
            # what q sends s is what s expects from q: the same count, and the same nodes in the same order
            n_sq = int(got[q.rank][3][s.rank + 1] - got[q.rank][3][s.rank])
            assert n_sq == int(recv_cnt[q.rank + 1] - recv_cnt[q.rank])
            sent = q.lo + got[q.rank][2][got[q.rank][3][s.rank]:got[q.rank][3][s.rank + 1]]
            want = s.remote[recv_list[recv_cnt[q.rank]:recv_cnt[q.rank + 1]] - s.n]
            assert np.array_equal(sent, want)
        assert recv_cnt[s.rank + 1] == recv_cnt[s.rank] and send_cnt[s.rank + 1] == send_cnt[s.rank]     # nothing from or to itself


def test_transfer_phase_lands_the_owners_rows_on_the_listed_boundary_rows():
    ranks = K.shard_layouts(3)
    rng = np.random.RandomState(13)
    d = 4
    lists = [rng.randint(0, s.n, 6).astype(np.int32) for s in ranks]
    got = lazy_request_phase(ranks, lists)
    # operand row = (global node id, feature) so that a row says where it came from
    op = [np.full((s.n + s.n_halo, d), -1.0, np.float32) for s in ranks]
    for s in ranks:
        op[s.rank][:s.n] = (s.lo + np.arange(s.n))[:, None] * 10 + np.arange(d)
    sendbuf = [M.pack_rows(op[s.rank], got[s.rank][2]) for s in ranks]
    recvbuf = M.exchange_rows(sendbuf, [g[3] for g in got], [np.zeros((len(g[0]), d), np.float32) for g in got], [g[1] for g in got], d)
    for s in ranks:
        new = M.unpack_rows(op[s.rank], recvbuf[s.rank], got[s.rank][0])
        fetched = np.zeros(s.n + s.n_halo, bool)
        fetched[got[s.rank][0]] = True
        assert not fetched[:s.n].any()
        assert np.array_equal(new[fetched], (s.remote[np.flatnonzero(fetched) - s.n])[:, None] * 10 + np.arange(d))
        assert (new[s.n:][~fetched[s.n:]] == -1.0).all() and np.array_equal(new[:s.n], op[s.rank][:s.n])
