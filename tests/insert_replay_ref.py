"""The frozen-graph replay of ONE batched Insert, as plain numpy: a definition of what the GPU builder must leave behind that needs no
f32 oracle index, so it holds for every metric x quantisation x row layout (the oracle's Hnsw is f32 only and its cosine Insert re-normalises).

A graph G0 (tombstones allowed) receives one batch of B new vectors, every one of level 0, efConstruction >= m:

  own row    the new vertex's level-0 row is Hnsw.Search(x, k = m, ef = efConstruction) on G0: the answers ordered by slot, the stored edge
             distances are the search's score bits;
  back rows  an old vertex t keeps its G0 row plus (new slot, distance) for every new vertex that chose t; if that exceeds the row's width,
             the entries whose target is tombstoned are dropped, then the `width` smallest by (distance as f32, slot) stay; ordered by slot;
  the rest   levels, upper rows, the entrypoint and the tombstones do not change.

Graphs are dicts in the layout of Hnsw.Export() / the oracle's export(): ids, levels, deleted, row_offsets, nbr, nbr_dist, entry; the rows of a
slot are consecutive, level 0 first.  test_insert_replay_ref.py pins the replay against the oracle's batched Insert; link_bookkeeping counts,
from two exports of ANY reference index around one batch, what the batch's link pass had to do (fan-in, overflows, tombstones met, ties)."""
import numpy as np


def first_rows(g):
    """[slots + 1] index of every slot's level-0 row among the rows of an Export()-layout graph (the last entry = the row count)"""
    lv = np.asarray(g["levels"], np.int64)
    first = np.zeros(len(lv) + 1, np.int64)
    np.cumsum(lv + 1, out=first[1:])
    return first


def prune_row(slots, dists, deleted, width):
    """A row that received links: (slots, dists, overflowed, a tie decided).  Unchanged if it fits; otherwise without its tombstoned targets, cut to
    the `width` smallest by (distance, slot).  Always returned in slot order.  `a tie decided`: the last entry kept and the first one dropped
    have equal distances, so only the slot order chose between them."""
    slots = np.asarray(slots, np.int32); dists = np.asarray(dists, np.float32)
    over = len(slots) > width
    tie = False
    if over:
        live = np.asarray(deleted)[slots] == 0
        slots, dists = slots[live], dists[live]
        o = np.lexsort((slots, dists))          # primary key the distance, then the slot
        if len(o) > width:
            tie = bool(dists[o[width - 1]] == dists[o[width]])
            o = o[:width]
        slots, dists = slots[o], dists[o]
    o = np.argsort(slots, kind="stable")
    return slots[o], dists[o], over, tie


def replay_insert_batch(g0, new_ids, ans_slots, ans_dist, ans_count, m, width0, deleted=None):
    """The expected Export() after the batch, and the replay's bookkeeping.
    g0: the graph before the batch.  ans_slots / ans_dist [B, >= m], ans_count [B]: per new vector the answers of Hnsw.Search(k = m,
    ef = efConstruction) on g0, nearest first (slots, not ids).  m: neighbours a new vertex selects; width0: the level-0 row width (mMax0);
    deleted: the tombstones [slots] (default g0["deleted"]).
    Bookkeeping: max_fan_in (most requests one row received), full_own_rows (new vertices with m entries), overflow (old rows that exceeded
    width0), overflow_with_tombstone (of those, the ones that listed a tombstoned target in g0), tie_rows (prunes a tie decided)."""
    lv0 = np.asarray(g0["levels"], np.int32); n0 = len(lv0); B = len(new_ids)
    dele = np.asarray(g0["deleted"] if deleted is None else deleted, np.uint8)
    first = first_rows(g0); off = np.asarray(g0["row_offsets"], np.int64)
    nbr = np.asarray(g0["nbr"], np.int32); nd = np.asarray(g0["nbr_dist"], np.float32)
    R0 = int(first[-1])
    rows_s = [nbr[off[r]:off[r + 1]] for r in range(R0)]
    rows_d = [nd[off[r]:off[r + 1]] for r in range(R0)]
    book = {"max_fan_in": 0, "full_own_rows": 0, "overflow": 0, "overflow_with_tombstone": 0, "tie_rows": 0}
    dele1 = np.concatenate([dele, np.zeros(B, np.uint8)])   # the new vertices are alive
    asked = {}                                  # old slot -> [(new slot, distance)]
    for b in range(B):
        c = min(int(ans_count[b]), int(m))
        s = np.asarray(ans_slots[b][:c], np.int32); d = np.asarray(ans_dist[b][:c], np.float32)
        assert len(np.unique(s)) == c and (c == 0 or (0 <= s.min() and s.max() < n0)), "a search answer names a slot twice or a slot outside g0"
        o = np.argsort(s, kind="stable")
        rows_s.append(s[o]); rows_d.append(d[o])
        book["full_own_rows"] += int(c == m)
        for t, dd in zip(s.tolist(), d):
            asked.setdefault(t, []).append((n0 + b, dd))
    for t, reqs in asked.items():
        r = int(first[t])
        s = np.concatenate([rows_s[r], np.array([x[0] for x in reqs], np.int32)])
        d = np.concatenate([rows_d[r], np.array([x[1] for x in reqs], np.float32)])
        held_tomb = bool(dele[rows_s[r]].any())
        rows_s[r], rows_d[r], over, tie = prune_row(s, d, dele1, width0)
        book["max_fan_in"] = max(book["max_fan_in"], len(reqs))
        book["overflow"] += int(over); book["overflow_with_tombstone"] += int(over and held_tomb); book["tie_rows"] += int(tie)
    cnt = np.array([len(x) for x in rows_s], np.int64)
    out_off = np.zeros(len(cnt) + 1, np.int64); np.cumsum(cnt, out=out_off[1:])
    g1 = {"ids": np.concatenate([np.asarray(g0["ids"], np.uint64), np.asarray(new_ids, np.uint64)]),
          "levels": np.concatenate([lv0, np.zeros(B, np.int32)]),
          "deleted": dele1,
          "row_offsets": out_off,
          "nbr": np.concatenate(rows_s).astype(np.int32) if len(rows_s) else np.zeros(0, np.int32),
          "nbr_dist": np.concatenate(rows_d).astype(np.float32) if len(rows_d) else np.zeros(0, np.float32),
          "entry": int(g0["entry"])}
    return g1, book


def link_bookkeeping(before, after, width0, width_up):
    """What the link pass of ONE batch had to do, read off a reference index's exports before and after it (any levels; no slot was removed in
    between).  A new vertex's own rows are final when the batch ends (nobody else links to a vertex without in-edges, and they hold at most m
    entries), so they ARE the batch's requests: row (t, l) received one from every new vertex whose level-l row lists t.
    Returns max_fan_in, overflow (rows with existing + requests > width), overflow_with_tombstone (of those, the ones that listed a tombstoned
    target before the batch), tie_rows (overflowed rows whose cut fell between two equal distances)."""
    lb = np.asarray(before["levels"], np.int64); la = np.asarray(after["levels"], np.int64)
    n0 = len(lb)
    assert np.array_equal(la[:n0], lb), "the batch changed an old vertex's level"
    fa = first_rows(after); R0 = int(first_rows(before)[-1]); R1 = int(fa[-1])
    offb = np.asarray(before["row_offsets"], np.int64); offa = np.asarray(after["row_offsets"], np.int64)
    nbb = np.asarray(before["nbr"], np.int64); ndb = np.asarray(before["nbr_dist"], np.float32)
    nba = np.asarray(after["nbr"], np.int64); nda = np.asarray(after["nbr_dist"], np.float32)
    dele = np.asarray(after["deleted"], np.uint8)
    book = {"max_fan_in": 0, "overflow": 0, "overflow_with_tombstone": 0, "tie_rows": 0}
    if R1 == R0 or R0 == 0:
        return book
    row_slot = np.repeat(np.arange(len(la)), la + 1)
    row_level = np.arange(R1) - fa[:-1][row_slot]
    e0 = offa[R0]
    cnt_new = np.diff(offa[R0:])
    tgt = nba[e0:]; src = np.repeat(row_slot[R0:], cnt_new); lvl = np.repeat(row_level[R0:], cnt_new); dd = nda[e0:]
    assert (tgt < n0).all(), "vertices of one batch list each other"
    trow = fa[tgt] + lvl
    req = np.bincount(trow, minlength=R0)[:R0]
    cnt0 = np.diff(offb)
    W = np.where(row_level[:R0] == 0, width0, width_up)
    over = (req > 0) & (cnt0 + req > W)
    held = np.bincount(np.repeat(np.arange(R0), cnt0), weights=dele[nbb], minlength=R0)[:R0] > 0
    book["max_fan_in"] = int(req.max())
    book["overflow"] = int(over.sum())
    book["overflow_with_tombstone"] = int((over & held).sum())
    for r in np.nonzero(over)[0]:
        mk = trow == r
        s = np.concatenate([nbb[offb[r]:offb[r + 1]], src[mk]]); d = np.concatenate([ndb[offb[r]:offb[r + 1]], dd[mk]])
        book["tie_rows"] += int(prune_row(s, d, dele, int(W[r]))[3])
    return book


def add_books(total, book):
    """accumulate link_bookkeeping results: sums, and the maximum of max_fan_in"""
    for k, v in book.items():
        total[k] = max(total.get(k, 0), v) if k == "max_fan_in" else total.get(k, 0) + v
    return total


def del_bits(deleted):
    """Export()["deleted"] [slots] -> the uint32 bitmap words the walks read (bit s % 32 of word s // 32)"""
    d = np.asarray(deleted, np.uint8) != 0
    pad = (-len(d)) % 32
    b = np.packbits(np.concatenate([d, np.zeros(pad, bool)]), bitorder="little")
    return np.ascontiguousarray(b).view(np.uint32).copy()
