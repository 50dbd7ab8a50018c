"""numpy mirror of the halo bookkeeping and the batch preparation of a sharded plan -- TEST INFRASTRUCTURE (tests/test_halo_ops_mirror.py
holds it to brute force and to the product's shard layout on the CPU; tests/test_gpu_halo_ops.py holds the HIP launchers to it, bit for
bit).  Written from the contracts in include/gssgcn.h ("FOR TESTS: the halo bookkeeping ..."), one function per op, not from the kernels:
everything is integers, bits and row copies, so every result is exact and there is no tolerance anywhere.

THE BITMAP CONTRACTS, asserted on every input (check_ranges, check_list ...):
  * a bitmap is uint32 words, bit i = word i >> 5, bit i & 31 (numpy: unpackbits(..., bitorder="little") of the little-endian words);
  * a bitmap over the slots of P peers is P word-aligned ranges: woff[q + 1] - woff[q] = ceil((off[q + 1] - off[q]) / 32);
  * the padding bits of a range's last word are clear -- a set one would be listed as a slot of the next peer;
  * bits are cleared bit by bit (bits_clear): the word-wise clear of gss_batch_bits, whose contract is "every set bit of the word is
    mine", is NOT used on these bitmaps -- the word that straddles the own rows and the halo is shared;
  * the ids of a batch that get a position (op >= 0) are distinct; the rows unpack_rows and scatter_add_rows write are distinct (two
    writers of one row would race on the device; a mirror would hide that by picking the last).
No function changes its arguments: each returns new arrays."""
import numpy as np


def words_for(n_bits):
    return (int(n_bits) + 31) // 32


def word_offsets(off):
    """word ranges of the slot ranges [off[q], off[q + 1]): every range starts on a word"""
    off = np.asarray(off, np.int64)
    assert off.ndim == 1 and len(off) >= 2 and off[0] == 0 and (np.diff(off) >= 0).all(), off
    woff = np.zeros(len(off), np.int64)
    woff[1:] = np.cumsum((np.diff(off) + 31) // 32)
    return woff


def to_bool(words, n_bits=None):
    """the bits of uint32 words as a bool array (bit i of the bitmap at [i])"""
    words = np.ascontiguousarray(words, dtype="<u4")
    b = np.unpackbits(words.view(np.uint8), bitorder="little").astype(bool)
    return b if n_bits is None else b[:n_bits]


def from_bool(b, n_words=None):
    b = np.asarray(b, bool)
    n_words = words_for(len(b)) if n_words is None else n_words
    full = np.zeros(n_words * 32, bool)
    full[:len(b)] = b
    return np.packbits(full, bitorder="little").view("<u4").astype(np.uint32)


def check_ranges(words, off, woff):
    """the contracts of a bitmap over P slot ranges"""
    off, woff = np.asarray(off, np.int64), np.asarray(woff, np.int64)
    assert (woff == word_offsets(off)).all(), ("ranges are word-aligned and exactly as long as their slots need", off, woff)
    assert len(words) >= woff[-1]
    for q in range(len(off) - 1):
        nb = int(off[q + 1] - off[q])
        assert not to_bool(words[woff[q]:woff[q + 1]])[nb:].any(), f"range {q}: a padding bit is set"


def check_distinct(rows, what):
    rows = np.asarray(rows)
    assert len(np.unique(rows)) == len(rows), f"{what}: rows are not distinct"


# ---- row copies ------------------------------------------------------------------------------------------------------------------
def pack_rows(src, rows):
    """out[k] = src[rows[k]]; rows may repeat (one row can go to several peers).  Bits are copied: NaN payloads and denormals survive."""
    rows = np.asarray(rows, np.int64)
    assert rows.size == 0 or (rows.min() >= 0 and rows.max() < len(src))
    return np.ascontiguousarray(src).view(np.uint32)[rows].view(src.dtype).copy()


def unpack_rows(dst, src, rows):
    """dst[rows[k]] = src[k]; unlisted rows of dst keep what they hold"""
    rows = np.asarray(rows, np.int64)
    check_distinct(rows, "unpack_rows")
    assert rows.size == 0 or (rows.min() >= 0 and rows.max() < len(dst))
    out = np.ascontiguousarray(dst).copy()
    out.view(np.uint32)[rows] = np.ascontiguousarray(src).view(np.uint32)[:len(rows)]
    return out


# ---- bitmaps ----------------------------------------------------------------------------------------------------------------------
def halo_need_mark(indptr, indices, rows, n, recv_off, needw):
    """needw |= for every listed row r >= 0 and every entry of it with a column c >= n: halo slot h = c - n belongs to the owner q with
    recv_off[q] <= h < recv_off[q + 1] (empty ranges own nothing) and is bit h - recv_off[q] of q's word range.  Nothing is cleared."""
    recv_off = np.asarray(recv_off, np.int64)
    woff = word_offsets(recv_off)
    check_ranges(needw, recv_off, woff)
    out = np.array(needw, dtype=np.uint32)
    for r in np.asarray(rows):
        if r < 0:
            continue                      # a member another shard owns
        for c in indices[indptr[r]:indptr[r + 1]]:
            if c < n:
                continue
            h = int(c) - n
            assert h < recv_off[-1], "a column behind the halo"
            q = int(np.searchsorted(recv_off, h, side="right")) - 1
            bit = int(woff[q]) * 32 + h - int(recv_off[q])
            out[bit >> 5] |= np.uint32(1 << (bit & 31))
    return out


def send_slot_bits(bits, send_rows, send_off):
    """words over the send slots: slot s of peer q carries bit send_rows[s] of `bits`; every word of every range is produced, padding clear"""
    send_off = np.asarray(send_off, np.int64)
    woff = word_offsets(send_off)
    have = to_bool(bits)
    out = np.zeros(int(woff[-1]), np.uint32)
    for q in range(len(send_off) - 1):
        s0, s1 = int(send_off[q]), int(send_off[q + 1])
        out[woff[q]:woff[q + 1]] = from_bool(have[np.asarray(send_rows[s0:s1], np.int64)], int(woff[q + 1] - woff[q]))
    return out


def bits_assign(bits, first, last, value):
    b = to_bool(bits)
    if last > first:
        assert 0 <= first and last <= len(b)
        b[first:last] = value
    return from_bool(b, len(bits))


def bits_clear(bits, first, last):
    """bits [first, last) := 0, every other bit unchanged; nothing for last <= first"""
    return bits_assign(bits, first, last, False)


def bits_fill(bits, first, last):
    """bits [first, last) := 1, every other bit unchanged; nothing for last <= first"""
    return bits_assign(bits, first, last, True)


def bits_set_list(bits, ids):
    """bits[ids[k]] := 1; ids may repeat, none is negative"""
    ids = np.asarray(ids, np.int64)
    b = to_bool(bits)
    assert ids.size == 0 or (ids.min() >= 0 and ids.max() < len(b))
    b[ids] = True
    return from_bool(b, len(bits))


def bits_compact(words, woff, slot_off, slot_map=None, add=0):
    """the set bits of the P ranges, ascending, as (list, out_off): bit j of range q is slot slot_off[q] + j, listed as slot_map[slot] or
    slot + add; out_off[q + 1] = entries up to and including range q"""
    woff, slot_off = np.asarray(woff, np.int64), np.asarray(slot_off, np.int64)
    check_ranges(words, slot_off, woff)
    P = len(woff) - 1
    out_off = np.zeros(P + 1, np.int64)
    parts = []
    for q in range(P):
        slots = slot_off[q] + np.flatnonzero(to_bool(words[woff[q]:woff[q + 1]]))
        parts.append(slots)
        out_off[q + 1] = out_off[q] + len(slots)
    slots = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    lst = np.asarray(slot_map)[slots] if slot_map is not None else slots + add
    return lst.astype(np.int32), out_off


# ---- batch preparation and its undoing -----------------------------------------------------------------------------------------------
def batch_prepare(idx, node_map, lo, nl, gid2op, pos):
    """-> dict(rloc, pid, keep, rlist, pos).  id = node_map[idx[i]] (idx[i] without a map), rel = id - lo, owned <=> 0 <= rel < nl,
    op = gid2op[id], or without gid2op rel when owned and -1 when not; rloc = rel clamped to [0, max(nl - 1, 0)]; pid = op; keep = owned;
    rlist = rel when owned, -1 when not; pos[op] = i where op >= 0 and nowhere else."""
    idx = np.asarray(idx, np.int64)
    ids = np.asarray(node_map, np.int64)[idx] if node_map is not None else idx
    rel = ids - lo
    mine = (rel >= 0) & (rel < nl)
    op = np.asarray(gid2op, np.int64)[ids] if gid2op is not None else np.where(mine, rel, -1)
    check_distinct(op[op >= 0], "batch_prepare (position ids)")
    out_pos = np.array(pos, dtype=np.int32)
    out_pos[op[op >= 0]] = np.flatnonzero(op >= 0).astype(np.int32)
    return dict(rloc=np.clip(rel, 0, max(nl - 1, 0)).astype(np.int32), pid=op.astype(np.int32), keep=mine.astype(np.float32),
                rlist=np.where(mine, rel, -1).astype(np.int32), pos=out_pos)


def scatter_add_rows(dst, src, rows, keep, pos=None, pos_ids=None):
    """-> (dst, pos).  Member r is skipped when rows[r] < 0 or keep[r] == 0 (keep may be None), else dst[rows[r]] += src[r] in fp32 (one
    addend per destination row: exact whatever the order).  pos[pos_ids[r]] = -1 for EVERY r with pos_ids[r] >= 0 -- a skipped member's
    position is reset too: the map must be all -1 again after the step, whoever owns the member."""
    rows = np.asarray(rows, np.int64)
    live = rows >= 0
    if keep is not None:
        live &= np.asarray(keep) != 0
    check_distinct(rows[live], "scatter_add_rows")
    out = np.array(dst, dtype=np.float32)
    out[rows[live]] = out[rows[live]] + np.asarray(src, np.float32)[live]
    out_pos = None
    if pos is not None:
        pos_ids = np.asarray(pos_ids, np.int64)
        out_pos = np.array(pos, dtype=np.int32)
        out_pos[pos_ids[pos_ids >= 0]] = -1
    return out, out_pos


# ---- the exchange between ranks (gss_comm::exchange_rows) ---------------------------------------------------------------------------
def exchange_rows(send, send_off, recv, recv_off, d=1):
    """Every rank at once: rows [send_off[r][q], send_off[r][q + 1]) of send[r] go to rank q and land at rows [recv_off[q][r],
    recv_off[q][r + 1]) of recv[q] (row = d elements; a rank's own range is empty).  -> the new recv buffers; everything outside the
    landing ranges is unchanged."""
    W = len(send)
    out = [np.array(r) for r in recv]
    for r in range(W):
        assert send_off[r][r + 1] == send_off[r][r] and recv_off[r][r + 1] == recv_off[r][r], "a rank sends itself nothing"
        for q in range(W):
            s0, s1 = int(send_off[r][q]), int(send_off[r][q + 1])
            r0, r1 = int(recv_off[q][r]), int(recv_off[q][r + 1])
            assert s1 - s0 == r1 - r0, f"rank {r} sends rank {q} {s1 - s0} rows, which expects {r1 - r0}"
            out[q].reshape(-1)[r0 * d:r1 * d] = np.asarray(send[r]).reshape(-1)[s0 * d:s1 * d]
    return out


def exchange_words(send, send_woff, recv, recv_woff):
    """bitmap ranges travel as they stand: word-aligned, one element per word"""
    return exchange_rows(send, send_woff, recv, recv_woff, 1)
