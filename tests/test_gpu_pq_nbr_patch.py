"""The neighbourhood blocks of the product-quantised walk (pq_nbr[slot][p] = pq_codes[adj0[slot][p]]) are kept current by the writers: after Insert,
InsertBatchDevice and Remove the blocks that were current before the call are current when it returns — no search in between, no whole rebuild — and they are
byte for byte what a whole build would gather from the final level-0 rows.  Everything that cannot be patched (a grown capacity, Load / BulkLoad / a new
quantiser, the knob switched off) leaves them stale for the next walk to rebuild, and the answers never differ from the walk that gathers by neighbour slot."""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
K = 10
# (dim, sub-vectors, centroids, M): 16-byte code rows at W = 2 M = 32 | 48-byte rows (3 pieces) | 64-byte rows (the bench's 64 x 32) | W = 8
SHAPES = [(64, 16, 32, 16), (96, 48, 16, 16), (128, 64, 32, 16), (64, 16, 32, 4)]


def expected_blocks(h):
    """what pq_nbr_build_kernel writes for the index as it is now: zeros, and the neighbour's code row wherever the level-0 row lists one"""
    adj0 = h.ExportRaw()["adj0"]
    codes = h.PqCodes()
    row = (codes.shape[1] + 15) & ~15
    padded = np.zeros((codes.shape[0], row), np.uint8); padded[:, :codes.shape[1]] = codes
    expected = np.zeros(adj0.shape + (row,), np.uint8)
    expected[adj0 != NONE] = padded[adj0[adj0 != NONE]]
    return expected, adj0


class Case:
    """an index of n vertices (graph built on the GPU), Reserve'd for everything the test adds, with a quantiser trained on its stored rows attached"""

    def __init__(self, gpu, shape, metric, explicit, n=2000, spare=256, algo=0, seed=7100, reserve=True):
        import torch
        self.gpu, self.n0, self.explicit = gpu, n, explicit
        d, m, c, M = shape
        self.d, self.M = d, M
        tot = n + spare
        self.X = O.fill_normal(seed + d + m + M, (tot, d)); self.lv = O.levels(seed + 1 + d + m + M, tot)
        self.ids = (np.arange(tot, dtype=np.uint64) * np.uint64(7) + np.uint64(3)) if explicit else np.arange(tot, dtype=np.uint64)
        self.h = h = gpu.Hnsw(d, metric, gpu.HnswCfg.default(m=M, ef=32, ef_construction=40, algo=algo, keep_pruned=0 if algo == 2 else 1))
        if reserve:
            h.Reserve(tot)
        self.xd = torch.from_numpy(self.X).to("cuda:0"); torch.cuda.synchronize()
        h.InsertBatchDevice(self.xd.data_ptr(), n, self.lv[:n], batch=64, first_id=0, ids=self.ids[:n] if explicit else None)
        self.pqm = gpu.PQ_COSINE if metric == gpu.COSINE else gpu.PQ_EUCLIDEAN
        self.pq = gpu.PQSpace(d, self.pqm, m, c); self.pq.Fit(h.FetchRows()[:n], iterations=3)
        h.PqAttach(self.pq)
        self.next = n                                          # the next unused row of X / ids
        self.Q = O.fill_normal(seed + 9, (16, d))
        self.W = h.cfg.m_max0
        self.rows_seen = h.PqNbrStats()["patched_rows"]; self.calls_seen = h.PqNbrStats()["patches"]

    def insert(self, level=None):
        i = self.next; self.next += 1
        self.h.Insert(int(self.ids[i]), self.X[i], int(self.lv[i] if level is None else level))

    def insert_batch(self, b, batch):
        i = self.next; self.next += b
        self.h.InsertBatchDevice(self.xd.data_ptr() + i * self.d * 4, b, self.lv[i:i + b], batch=batch, first_id=int(self.ids[i]),
                                 ids=self.ids[i:i + b] if self.explicit else None)

    def verify(self, tag, before, calls, bound, builds=1):
        """state / builds, the blocks byte for byte, and how many blocks the `calls` mutating calls since `before` (an adj0 snapshot) rewrote: at least the level-0
        rows that differ (new rows included), at most `bound` (the request bound the write kernels size their queues by).  Returns the adj0 snapshot of now."""
        st = self.h.PqNbrStats()
        assert st["state"] == 1 and st["builds"] == builds, (tag, st)
        want, adj0 = expected_blocks(self.h)
        got = self.h.PqFetchNbr()
        assert got.shape == want.shape and np.array_equal(got, want), (tag, np.argwhere((got != want).any(axis=(1, 2)))[:8].ravel())
        changed = int((adj0[:len(before)] != before).any(axis=1).sum()) + (len(adj0) - len(before))
        grew = st["patched_rows"] - self.rows_seen
        print(f"[{tag}] level-0 rows changed {changed}, blocks patched {grew}, bound {bound}")
        assert changed <= grew <= bound, (tag, changed, grew, bound)
        assert st["patches"] - self.calls_seen == calls, (tag, st, calls)
        self.rows_seen, self.calls_seen = st["patched_rows"], st["patches"]
        return adj0


def run_sequence(c, n_single=40, n_remove=40, n_batch=150, check=True):
    """attach -> first walk (the one whole build) -> single Inserts -> Removes -> InsertBatchDevice at batch 8; no search after the first one"""
    h, gpu = c.h, c.gpu
    st = h.PqNbrStats()
    assert st["state"] == 0 and st["builds"] == 0, st                       # attached, never built
    with pytest.raises(gpu.ColttError) as e:
        h.PqFetchNbr(0, 1)
    assert e.value.code == -4
    h.PqSearch(c.Q, K, ef=300)
    snap = c.verify("first walk", h.ExportRaw()["adj0"], 0, 0) if check else None
    # single Inserts: levels > 0 among them, and one above the entry level (the entry point moves)
    g = h.ExportRaw()
    levels = [None] * n_single
    levels[1], levels[3], levels[4] = 1, 2, g["entry_level"] + 1
    for i in range(n_single):
        c.insert(levels[i])
        if check and i < 5:
            snap = c.verify(f"insert {i}", snap, 1, 1 + c.M)
    g2 = h.ExportRaw()
    assert g2["entry"] == c.n0 + 4 and g2["entry_level"] == g["entry_level"] + 1
    if check:
        snap = c.verify("single inserts", snap, n_single - 5, (n_single - 5) * (1 + c.M))
    # Removes: the current entry point, a vertex of the previous step, and old ones
    victims = [g2["entry"], c.n0 + 7] + list(range(5, 5 + 3 * (n_remove - 2), 3))
    for j, s in enumerate(victims):
        h.Remove(int(c.ids[s]))
        if check and j < 2:
            snap = c.verify(f"remove {j}", snap, 1, c.W)
    assert h.ExportRaw()["entry"] != g2["entry"]
    if check:
        snap = c.verify("removes", snap, n_remove - 2, (n_remove - 2) * c.W)
    assert h.ExportRaw()["n"] % 32 != 0                                      # the batch below starts inside a word of the tombstone bitmap
    c.insert_batch(n_batch, 8)
    if check:
        c.verify("batch insert", snap, 1, n_batch * (1 + c.M))
    assert h.Len() == c.n0 + n_single - n_remove + n_batch


@pytest.mark.parametrize("explicit", [False, True], ids=["dense", "explicit-ids"])
@pytest.mark.parametrize("metric", ["l2", "cos"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d-m%d-c%d-M%d" % s)
def test_blocks_follow_every_write_without_a_rebuild(gpu, shape, metric, explicit):
    """Fails without the feature: a write then leaves the blocks stale (state 2) and the next walk builds them whole again (builds grows)."""
    run_sequence(Case(gpu, shape, gpu.COSINE if metric == "cos" else gpu.EUCLIDEAN, explicit))


def _walks(gpu, h, Q, ef, rr, monkeypatch, flt=None):
    """the same search over the blocks and gathering by neighbour slot (COLTT_PQ_NBR=0), in this process on this index"""
    got = {}
    for nbr in ("1", "0"):
        monkeypatch.setenv("COLTT_PQ_NBR", nbr)
        try:
            if flt is None:
                got[nbr] = h.PqSearch(Q, K, ef=ef, rerank=rr, with_stats=True)
            else:
                got[nbr] = h.PqSearchFiltered(Q, K, flt, ef=ef, rerank=rr, mode=gpu.FILTER_WALK, with_stats=True)
        finally:
            monkeypatch.delenv("COLTT_PQ_NBR")
    return got


def assert_same_as_gathered(gpu, h, Q, monkeypatch, tag, efs=((300, 0), (200, 0))):
    for ef, rr in efs:
        got = _walks(gpu, h, Q, ef, rr, monkeypatch)
        a, b = got["1"], got["0"]
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]) and a[3] == b[3], (tag, ef, rr)


def test_answers_are_unchanged_after_patched_writes(gpu, monkeypatch):
    """After the whole sequence the walk over the PATCHED blocks (never rebuilt) equals the oracle's definition — ids, exact score bits, all four counters — and
    the walk that gathers code rows by neighbour slot; the filtered walk (its FILTER instances read the blocks too) equals its gathered twin."""
    d = 64
    c = Case(gpu, SHAPES[0], gpu.EUCLIDEAN, False)
    run_sequence(c, check=False)
    h = c.h
    assert h.PqNbrStats()["state"] == 1 and h.PqNbrStats()["builds"] == 1
    codes = h.PqCodes(); g = h.ExportRaw(); rows = h.FetchRows(); ex = h.Export(); cb = c.pq.Codebooks()
    assert ex["deleted"].any()
    dl = np.packbits(ex["deleted"].astype(np.uint8), bitorder="little")
    dl = np.concatenate([dl, np.zeros((-len(dl)) % 4, np.uint8)]).view(np.uint32)
    for ef, rr in ((300, 0), (300, 40), (200, 0)):
        sl, sc, cn, ost, _ = O.csr_search_pq(rows, O.Q_NONE, g["adj0"], g["upper_off"], g["adjU"], d, O.L2, g["entry"], g["entry_level"], codes, cb, c.pqm, c.Q, K, ef,
                                             rerank=rr, del_bits=dl)
        got = _walks(gpu, h, c.Q, ef, rr, monkeypatch)
        for nbr in ("1", "0"):
            gi, gs, gc, st = got[nbr]
            assert np.array_equal(gc, cn.astype(np.uint32)), (ef, rr, nbr)
            for qi in range(len(c.Q)):
                assert np.array_equal(gi[qi, :gc[qi]], ex["ids"][sl[qi, :cn[qi]]]), (ef, rr, nbr, qi)
                assert np.array_equal(bits(gs[qi, :gc[qi]]), bits(sc[qi, :cn[qi]])), (ef, rr, nbr, qi)
            assert st == ost, (ef, rr, nbr, st, ost)
    live = ex["ids"][ex["deleted"] == 0]
    with h.Filter(live[::3]) as flt:
        for ef, rr in ((300, 0), (300, 12)):
            got = _walks(gpu, h, c.Q, ef, rr, monkeypatch, flt)
            a, b = got["1"], got["0"]
            assert a[3]["path"] == gpu.FILTER_WALK and a[3] == b[3], (ef, rr, a[3], b[3])
            assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]), (ef, rr)
    st = h.PqNbrStats()
    assert st["state"] == 1 and st["builds"] == 1, st                       # none of the searches above had anything to rebuild
    assert np.array_equal(h.PqFetchNbr(), expected_blocks(h)[0])


@pytest.mark.parametrize("metric", ["l2", "cos"])
def test_blocks_follow_the_diverse_link_kernel(gpu, metric):
    """cfg.algo == 2: the rows are rewritten by hnsw_link_diverse_kernel (one wave per touched row) — the same conditions, a shorter sequence"""
    c = Case(gpu, SHAPES[0], gpu.COSINE if metric == "cos" else gpu.EUCLIDEAN, False, n=1500, algo=2)
    run_sequence(c, n_single=12, n_remove=10, n_batch=60)


def test_growth_past_the_reserved_capacity_falls_back_to_the_rebuild(gpu, monkeypatch):
    """(a) an Insert that grows the slot capacity leaves the blocks stale (the array is too small); the next walk rebuilds, later Inserts patch again"""
    c = Case(gpu, SHAPES[0], gpu.EUCLIDEAN, False, n=1000, spare=80, reserve=False)      # capacity 1 024 after the build
    h = c.h
    h.PqSearch(c.Q, K, ef=300)
    snap = c.verify("first walk", h.ExportRaw()["adj0"], 0, 0)
    for _ in range(20): c.insert()                                                       # slots 1 000 .. 1 019: within capacity
    snap = c.verify("within capacity", snap, 20, 20 * (1 + c.M))
    for _ in range(10): c.insert()                                                       # slot 1 024 grows the arrays
    st = h.PqNbrStats()
    assert st["state"] in (1, 2) and st["builds"] == 1, st
    if st["state"] == 2:
        with pytest.raises(gpu.ColttError) as e:
            h.PqFetchNbr()
        assert e.value.code == -4
    assert_same_as_gathered(gpu, h, c.Q, monkeypatch, "after growth")
    st = h.PqNbrStats()
    assert st["state"] == 1 and st["builds"] == 2, st
    assert np.array_equal(h.PqFetchNbr(), expected_blocks(h)[0])
    c.rows_seen, c.calls_seen = st["patched_rows"], st["patches"]
    snap = h.ExportRaw()["adj0"]
    for _ in range(5): c.insert()
    c.verify("after the rebuild", snap, 5, 5 * (1 + c.M), builds=2)
    assert_same_as_gathered(gpu, h, c.Q, monkeypatch, "after the rebuild")


def test_load_bulk_load_and_a_new_quantiser_leave_the_blocks_stale(gpu, monkeypatch):
    """(b) everything renumbered or re-coded: stale, rebuilt whole by the next walk"""
    c = Case(gpu, SHAPES[0], gpu.EUCLIDEAN, False, n=800, spare=16)
    h = c.h
    h.PqSearch(c.Q, K, ef=300)
    builds = 1
    pq2 = gpu.PQSpace(c.d, gpu.PQ_EUCLIDEAN, 32, 16); pq2.Fit(h.FetchRows(), iterations=2)   # 32-byte code rows instead of 16
    ex = h.Export(); raw = h.FetchRows().copy()                                          # (a Euclidean f32 index stores the raw vectors)
    for tag, act in (("Load", lambda: h.Load(h.Commit())), ("BulkLoad", lambda: h.BulkLoad(ex, raw)), ("PqAttach", lambda: h.PqAttach(pq2))):
        assert h.PqNbrStats()["state"] == 1, tag
        act()
        st = h.PqNbrStats()
        assert st["state"] == 2 and st["builds"] == builds and st["patches"] == 0, (tag, st)
        with pytest.raises(gpu.ColttError):
            h.PqFetchNbr()
        assert_same_as_gathered(gpu, h, c.Q, monkeypatch, tag)
        builds += 1
        st = h.PqNbrStats()
        assert st["state"] == 1 and st["builds"] == builds, (tag, st)
        assert np.array_equal(h.PqFetchNbr(), expected_blocks(h)[0]), tag
    assert h.PqFetchNbr().shape[2] == 32


def test_knob_off_is_the_lazy_rebuild(gpu, monkeypatch):
    """(c) COLTT_PQ_NBR_PATCH=0: every write leaves the blocks stale, nothing is patched, the next walk builds them whole — the behaviour before this feature"""
    c = Case(gpu, SHAPES[0], gpu.EUCLIDEAN, False, n=800, spare=16)
    h = c.h
    h.PqSearch(c.Q, K, ef=300)
    monkeypatch.setenv("COLTT_PQ_NBR_PATCH", "0")
    try:
        builds = 1
        for tag, act in (("Insert", c.insert), ("Remove", lambda: h.Remove(11)), ("InsertBatchDevice", lambda: c.insert_batch(9, 4))):
            act()
            st = h.PqNbrStats()
            assert st["state"] == 2 and st["patches"] == 0 and st["patched_rows"] == 0 and st["builds"] == builds, (tag, st)
            with pytest.raises(gpu.ColttError) as e:
                h.PqFetchNbr()
            assert e.value.code == -4
            h.PqSearch(c.Q, K, ef=300)
            builds += 1
            st = h.PqNbrStats()
            assert st["state"] == 1 and st["builds"] == builds, (tag, st)
            assert np.array_equal(h.PqFetchNbr(), expected_blocks(h)[0]), tag
    finally:
        monkeypatch.delenv("COLTT_PQ_NBR_PATCH")
    snap = h.ExportRaw()["adj0"]
    c.insert()                                                                           # the knob is back on: the same index patches
    c.verify("knob back on", snap, 1, 1 + c.M, builds=builds)
    assert_same_as_gathered(gpu, h, c.Q, monkeypatch, "knob back on")


def test_nothing_is_tracked_while_no_blocks_are_kept(gpu, monkeypatch):
    """(d) a quantiser is attached but no walk has built the blocks, or COLTT_PQ_NBR=0: writes patch nothing; (e) PqFetchNbr refuses unless the blocks are current"""
    c = Case(gpu, SHAPES[0], gpu.EUCLIDEAN, False, n=800, spare=16)
    h = c.h
    for act in (c.insert, lambda: h.Remove(3), lambda: c.insert_batch(5, 2)):            # never built
        act()
        assert h.PqNbrStats() == {"builds": 0, "patches": 0, "patched_rows": 0, "state": 0}
    with pytest.raises(gpu.ColttError) as e:
        h.PqFetchNbr()
    assert e.value.code == -4
    h.PqSearch(c.Q, K, ef=48)                                                            # the LDS-hash walk does not read the blocks
    assert h.PqNbrStats()["state"] == 0
    assert_same_as_gathered(gpu, h, c.Q, monkeypatch, "first build")
    assert h.PqNbrStats() == {"builds": 1, "patches": 0, "patched_rows": 0, "state": 1}
    monkeypatch.setenv("COLTT_PQ_NBR", "0")                                              # switched off: state none, a write tracks nothing
    try:
        assert h.PqNbrStats()["state"] == 0
        with pytest.raises(gpu.ColttError) as e:
            h.PqFetchNbr()
        assert e.value.code == -4
        c.insert(); h.Remove(17)
        assert h.PqNbrStats() == {"builds": 1, "patches": 0, "patched_rows": 0, "state": 0}
    finally:
        monkeypatch.delenv("COLTT_PQ_NBR")
    assert h.PqNbrStats()["state"] == 2                                                  # back on: what the writes left is stale, never "current"
    assert_same_as_gathered(gpu, h, c.Q, monkeypatch, "switched back on")
    assert h.PqNbrStats()["builds"] == 2 and np.array_equal(h.PqFetchNbr(), expected_blocks(h)[0])
    no_pq = gpu.Hnsw(16, gpu.EUCLIDEAN)                                                  # no quantiser at all
    no_pq.Insert(0, np.ones(16, np.float32), 0); no_pq.Insert(1, np.zeros(16, np.float32), 0); no_pq.Remove(0)
    assert no_pq.PqNbrStats() == {"builds": 0, "patches": 0, "patched_rows": 0, "state": 0}
    with pytest.raises(gpu.ColttError):
        no_pq.PqFetchNbr(0, 1)


def test_readers_beside_a_writer(gpu):
    """two threads walk (shared lock) while the main thread Inserts and Removes (exclusive lock, patching before it lets go): every call succeeds, the blocks
    are never rebuilt and end up exactly the gathered ones"""
    c = Case(gpu, SHAPES[0], gpu.EUCLIDEAN, False, n=1500, spare=64)
    h = c.h
    h.PqSearch(c.Q, K, ef=300)
    stop = threading.Event(); errors = []; rounds = [0, 0]

    def reader(t):
        try:
            while not stop.is_set():
                _, _, cnt = h.PqSearch(c.Q, K, ef=300)
                assert (cnt == K).all()
                rounds[t] += 1
        except Exception as ex:   # noqa: BLE001 — reported by the main thread
            errors.append(ex)

    threads = [threading.Thread(target=reader, args=(t,), daemon=True) for t in range(2)]
    for t in threads: t.start()
    try:
        for i in range(60):
            c.insert()
            if i % 3 == 0:
                h.Remove(int(c.ids[100 + i]))
    finally:
        stop.set()
        for t in threads: t.join(timeout=60)
    assert not any(t.is_alive() for t in threads) and not errors, errors
    assert min(rounds) > 0, rounds
    st = h.PqNbrStats()
    assert st["state"] == 1 and st["builds"] == 1 and st["patches"] == 80, st
    assert np.array_equal(h.PqFetchNbr(), expected_blocks(h)[0])
