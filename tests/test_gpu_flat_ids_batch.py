"""coltt_flat_search_ids_batch (FlatSpace.FilterableVertexSearchBatch) on the GPU: a batch of filtered queries with a candidate list
each, in one call.  Row i must EQUAL — counts, ids, score bits, no tolerance —
  (a) the existing one-query call FilterableVertexSearch(list_i, Q[i:i+1], k, select) on the same store, and
  (b) the independent CPU oracle O.Flat(...).search(Q[i], k, nearest=..., mode=2, cand=list_i)
(edge/none_vectorstore.go:182-253; the reference serves one filtered query per RPC, each with its own id list)."""
import ctypes as C
import threading

import numpy as np
import pytest

from coltt_amd import _lib as LL
from oracle import oracle as O
from util import bits

pytestmark = pytest.mark.gpu


def scrambled_ids(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 33)   # slot order != id order (test_gpu_round3.py)


class Pair:
    """a GPU store and the oracle's with the same content, and a cache of the two one-query references"""

    def __init__(self, gpu, d, metric, quant, ids, X):
        self.gpu = gpu
        self.gf = gpu.FlatSpace(d, metric, quant); self.gf.ChangedVertex(ids, X)
        self.of = O.Flat(d, metric, quant); self.of.upsert(ids, X)
        self.ref = {}

    def remove(self, ids):
        self.gf.RemoveVertex(ids); self.of.remove(ids); self.ref.clear()

    def reference(self, key, cand, q, k, sel):
        """(count, ids, score bits) of the one-query GPU call, checked against the oracle once"""
        key = (key, k, sel)
        if key not in self.ref:
            gi, gs, gc = self.gf.FilterableVertexSearch(cand, q[None, :], k, sel)
            c = int(gc[0])
            # the oracle takes a roaring ToArray(): a set — it scores a repeated id twice, the store once (pkg/inverted/search.go:113-119)
            wi, ws = self.of.search(q, k, nearest=sel == self.gpu.SELECT_NEAREST, mode=2, cand=np.unique(cand))
            if not np.isnan(ws).any():     # NaN scores (cosine against a zero vector) are outside the oracle's parity contract
                assert c == len(wi) and np.array_equal(gi[0, :c], wi) and np.array_equal(bits(gs[0, :c]), bits(ws)), ("single call != oracle", key)
            self.ref[key] = (c, gi[0, :c].copy(), bits(gs[0, :c]).copy())
        return self.ref[key]

    def check_batch(self, lists, Q, k, sel, list_of=None, keys=None, tag=""):
        bi, bs, bc = self.gf.FilterableVertexSearchBatch(lists, Q, k, sel, list_of)
        lo = np.arange(len(Q)) if list_of is None else np.asarray(list_of)
        for i in range(len(Q)):
            l = int(lo[i])
            c, wi, wb = self.reference((keys[l] if keys else l, i), lists[l], Q[i], k, sel)
            assert int(bc[i]) == c, (tag, i, int(bc[i]), c)
            assert np.array_equal(bi[i, :c], wi), (tag, i, bi[i, :c], wi)
            assert np.array_equal(bits(bs[i, :c]), wb), (tag, i)
        return bi, bs, bc


def set_chunk(monkeypatch, v):
    """COLTT_FLAT_IDS_CHUNK through the policy snapshot: the binding sees the environment change and calls coltt_policy_reload"""
    if v is None:
        monkeypatch.delenv("COLTT_FLAT_IDS_CHUNK", raising=False)
    else:
        monkeypatch.setenv("COLTT_FLAT_IDS_CHUNK", str(v))


SHAPES = [(O.COSINE, O.Q_NONE, 4000, 128), (O.L2, O.Q_NONE, 3000, 77), (O.COSINE, O.Q_F16, 2000, 768), (O.L2, O.Q_BF16, 2000, 200),
          (O.COSINE, O.Q_F8, 3000, 64), (O.COSINE, O.Q_NONE, 1500, 1536)]


@pytest.mark.parametrize("metric,quant,n,d", SHAPES)
def test_codecs_and_metrics(gpu, monkeypatch, metric, quant, n, d):
    """Case 1: every codec and both metrics, dims that are no multiple of 8 / 4, ties decided by id (planted duplicate rows, ids not in
    slot order), one list per query and shared lists, list lengths {0, 1, 31, 32, 33, 100, n // 3, n}, 32-row tiles and automatic ones."""
    X = O.fill_normal(9000 + d + quant, (n, d)); X[500:600] = X[3]; X[n - 40:] = X[3]
    ids = scrambled_ids(n)
    NQ = 70
    Q = np.concatenate([X[3:4], O.fill_normal(9100 + d, (NQ - 1, d))])
    S = Pair(gpu, d, metric, quant, ids, X)
    rng = np.random.default_rng(n + d)
    sizes = [0, 1, 31, 32, 33, 100, n // 3, n]
    # 70 lists: the first three are the ones the shared-list batches use (every id, a third, 33), the rest draw their length
    lens = [n, n // 3, 33] + [sizes[int(rng.integers(len(sizes)))] for _ in range(NQ - 3)]
    pool = [ids.copy() if m == n else np.sort(rng.choice(ids, m, replace=False)) for m in lens]
    list_ofs = {(nq, nl): rng.integers(0, nl, nq).astype(np.uint32) for nq in (1, 9, 70) for nl in (1, 3)}
    st0 = S.gf.IdsBatchStats()
    calls = pairs = 0
    for nq in (1, 9, 70):
        for k in (1, 10, 64):
            for sel in (gpu.SELECT_REFERENCE, gpu.SELECT_NEAREST):
                shapes = [(pool[:nq], None)] + [(pool[:nl], list_ofs[(nq, nl)]) for nl in (1, 3)]
                for lists, lo in shapes:
                    tag = (nq, k, sel, len(lists))
                    set_chunk(monkeypatch, 32)
                    a = S.check_batch(lists, Q[:nq], k, sel, lo, tag=tag + ("chunk 32",))
                    set_chunk(monkeypatch, None)
                    b = S.check_batch(lists, Q[:nq], k, sel, lo, tag=tag + ("auto",))
                    for i in range(nq):
                        c = int(a[2][i])
                        assert c == int(b[2][i]) and np.array_equal(a[0][i, :c], b[0][i, :c]) and np.array_equal(bits(a[1][i, :c]), bits(b[1][i, :c])), tag
                    calls += 2
                    pairs += 2 * sum(len(lists[i if lo is None else int(lo[i])]) for i in range(nq))   # the lists are clean: live and distinct
    st = S.gf.IdsBatchStats()
    assert st["one_pass_calls"] - st0["one_pass_calls"] == calls and st["fallback_calls"] == st0["fallback_calls"], (st, calls)
    assert st["pairs"] - st0["pairs"] == pairs, (st, pairs)


def test_dirty_lists(gpu, monkeypatch):
    """Case 2: unknown ids, repeated ids, unsorted lists; ids removed before the call — RemoveVertex moves the last row into the hole,
    and that row must still be found under its own id."""
    n, d = 1200, 64
    X = O.fill_normal(9300, (n, d)); X[100:130] = X[5]
    ids = scrambled_ids(n)
    S = Pair(gpu, d, O.COSINE, O.Q_NONE, ids, X)
    Q = np.concatenate([X[5:6], O.fill_normal(9301, (8, d))])
    rng = np.random.default_rng(7)
    unknown = np.uint64(10**13) + np.arange(9, dtype=np.uint64)
    moved = ids[n - 6:]                    # the rows that will be moved into the holes
    gone = ids[[3, 50, 101, 700, 701, 1100]]
    lists = []
    for m in (40, 33, 400, 1, 64, 900, 0, 257, 100):
        base = rng.choice(ids, m, replace=False) if m else np.zeros(0, np.uint64)
        l = np.concatenate([base, base[: m // 3], unknown[: 1 + m % 5], moved[: m % 7], gone[: m % 4]])
        lists.append(rng.permutation(l))
    lists[3] = np.concatenate([moved[:1], moved[:1], unknown])            # one live id, twice
    for chunk in (32, None):
        set_chunk(monkeypatch, chunk)
        for k, sel in ((10, gpu.SELECT_NEAREST), (64, gpu.SELECT_REFERENCE)):
            S.check_batch(lists, Q, k, sel, tag=("dirty", chunk, k, sel))
    st0 = S.gf.IdsBatchStats()
    S.remove(gone)
    S.remove(np.uint64(10**13) + np.arange(3, dtype=np.uint64))           # unknown ids: a no-op
    assert S.gf.LoadSize() == n - len(gone)
    live = set(ids.tolist()) - set(gone.tolist())
    for chunk in (32, None):
        set_chunk(monkeypatch, chunk)
        for k, sel in ((10, gpu.SELECT_NEAREST), (64, gpu.SELECT_REFERENCE)):
            bi, bs, bc = S.check_batch(lists, Q, k, sel, tag=("after remove", chunk, k, sel))
            assert not (set(bi[i, j] for i in range(len(Q)) for j in range(bc[i])) & set(gone.tolist()))
    assert int(bc[3]) == 1 and bi[3, 0] == moved[0]                       # found under its own id, in its new slot
    want = 4 * sum(len(set(l.tolist()) & live) for l in lists)
    assert S.gf.IdsBatchStats()["pairs"] - st0["pairs"] == want           # pairs = live distinct candidates


def test_small_lists_and_mass_ties(gpu, monkeypatch):
    """Case 3: a list shorter than k, a store smaller than k, a cosine zero query, a list made only of duplicates of one row."""
    n, d = 700, 48
    X = O.fill_normal(9400, (n, d)); X[200:500] = X[9]
    ids = scrambled_ids(n)
    S = Pair(gpu, d, O.COSINE, O.Q_F16, ids, X)
    Q = np.concatenate([X[9:10], np.zeros((1, d), np.float32), O.fill_normal(9401, (3, d))])
    dup = ids[200:500]
    lists = [dup, ids[:5], dup[:40], ids, ids[100:330]]
    for chunk in (32, None):
        set_chunk(monkeypatch, chunk)
        for k in (10, 64):
            for sel in (gpu.SELECT_REFERENCE, gpu.SELECT_NEAREST):
                bi, bs, bc = S.check_batch(lists, Q, k, sel, tag=("ties", chunk, k, sel))
                assert bc.tolist() == [k, 5, min(k, 40), k, k]
                want = np.sort(dup)[:k] if sel == gpu.SELECT_NEAREST else np.sort(dup)[-k:]
                assert np.array_equal(bi[0, :k], want)                    # 300 equal scores: the ids decide, in both directions
                lo = np.array([0, 0, 3, 3, 0], np.uint32)                 # the zero query and the duplicates' own row over shared lists
                S.check_batch(lists, Q, k, sel, lo, tag=("ties shared", chunk, k, sel))
    tiny = Pair(gpu, d, O.L2, O.Q_NONE, ids[:7], X[:7])                   # a store smaller than k
    for k in (10, 64):
        bi, bs, bc = tiny.check_batch([ids[:7], ids[3:5], ids[100:200]], Q[:3], k, gpu.SELECT_NEAREST, tag=("tiny", k))
        assert bc.tolist() == [7, 2, 0]
    empty = gpu.FlatSpace(d, O.COSINE, O.Q_NONE)                          # an empty store: all counts 0
    bi, bs, bc = empty.FilterableVertexSearchBatch([ids[:9], ids[:0]], Q[:2], 10, gpu.SELECT_NEAREST)
    assert bc.tolist() == [0, 0]
    bi, bs, bc = S.gf.FilterableVertexSearchBatch([], Q[:0], 10, gpu.SELECT_NEAREST)   # nq == 0 is not an error
    assert len(bc) == 0


@pytest.mark.parametrize("k", [65, 300])
def test_large_k_goes_list_by_list(gpu, k):
    """Case 4: k > 64 is served through the shared-list path inside the same call — same equalities, counted as a fallback call."""
    n, d = 1500, 96
    X = O.fill_normal(9500, (n, d)); X[300:420] = X[4]
    ids = scrambled_ids(n)
    S = Pair(gpu, d, O.L2, O.Q_F16, ids, X)
    Q = np.concatenate([X[4:5], O.fill_normal(9501, (8, d))])
    rng = np.random.default_rng(k)
    lists = [ids, np.sort(rng.choice(ids, 500, replace=False)), ids[:33], ids[:0]]
    st0 = S.gf.IdsBatchStats()
    calls = 0
    for sel in (gpu.SELECT_REFERENCE, gpu.SELECT_NEAREST):
        S.check_batch(lists, Q, k, sel, rng.integers(0, 4, len(Q)).astype(np.uint32), tag=("large k", k, sel))
        S.check_batch(lists, Q[:4], k, sel, tag=("large k, own lists", k, sel))
        calls += 2
    st = S.gf.IdsBatchStats()
    assert st["fallback_calls"] - st0["fallback_calls"] == calls and st["one_pass_calls"] == st0["one_pass_calls"] and st["pairs"] == st0["pairs"]


def test_four_threads(gpu):
    """Case 5: four threads run the same batch 20 times each, concurrently; every answer equals the serial one."""
    n, d, nq, k = 3000, 128, 24, 10
    X = O.fill_normal(9600, (n, d)); X[40:90] = X[2]
    ids = scrambled_ids(n)
    S = Pair(gpu, d, O.COSINE, O.Q_NONE, ids, X)
    Q = np.concatenate([X[2:3], O.fill_normal(9601, (nq - 1, d))])
    rng = np.random.default_rng(5)
    lists = [np.sort(rng.choice(ids, int(m), replace=False)) for m in rng.integers(0, n, 10)]
    lo = rng.integers(0, len(lists), nq).astype(np.uint32)
    want = S.check_batch(lists, Q, k, gpu.SELECT_NEAREST, lo, tag="serial")
    bad = []

    def work():
        try:
            for _ in range(20):
                g = S.gf.FilterableVertexSearchBatch(lists, Q, k, gpu.SELECT_NEAREST, lo)
                if not (np.array_equal(g[2], want[2]) and np.array_equal(g[0], want[0]) and np.array_equal(bits(g[1]), bits(want[1]))):
                    bad.append("differs")
        except Exception as e:   # noqa: BLE001
            bad.append(repr(e))
    ts = [threading.Thread(target=work) for _ in range(4)]
    [t.start() for t in ts]; [t.join() for t in ts]
    assert not bad, bad[:3]


def test_errors_leave_the_outputs_untouched(gpu):
    """Case 6: argument errors on a live handle are found before anything runs."""
    L = gpu.lib()
    n, d, nq, k = 300, 32, 3, 5
    X = O.fill_normal(9700, (n, d)); ids = scrambled_ids(n)
    gf = gpu.FlatSpace(d, O.COSINE, O.Q_NONE); gf.ChangedVertex(ids, X)
    Q = O.fill_normal(9701, (nq, d))
    cand = np.ascontiguousarray(ids[:90])
    good_off = np.array([0, 30, 60, 90], np.uint64)

    def call(off, n_lists, list_of, select=gpu.SELECT_NEAREST, kk=k, q=Q, cand_=cand, null_out=False):
        oi = np.full((nq, k), 0xA5A5A5A5A5A5A5A5, np.uint64); sc = np.full((nq, k), -7.25, np.float32); oc = np.full(nq, 0xA5A5A5A5, np.uint32)
        rc = L.coltt_flat_search_ids_batch(gf.h, LL.vp(q), C.c_size_t(nq), C.c_uint32(kk), select, LL.vp(cand_), LL.vp(off), C.c_size_t(n_lists), LL.vp(list_of),
                                           LL.vp(None if null_out else oi), LL.vp(sc), LL.vp(oc))
        untouched = (oi == 0xA5A5A5A5A5A5A5A5).all() and (sc == -7.25).all() and (oc == 0xA5A5A5A5).all()
        return rc, L.coltt_last_error(), untouched
    rc, msg, same = call(good_off, 3, None)
    assert rc == 0 and not same
    st0 = gf.IdsBatchStats()
    rc, msg, same = call(np.array([0, 60, 30, 90], np.uint64), 3, None)
    assert rc == -1 and same and b"list_offsets" in msg
    rc, msg, same = call(good_off, 3, np.array([0, 2, 3], np.uint32))
    assert rc == -1 and same and b"list_of[2]" in msg                     # the message names the position
    rc, msg, same = call(good_off[:3], 2, None)
    assert rc == -1 and same and b"n_lists" in msg
    rc, msg, same = call(None, 3, None)
    assert rc == -1 and same
    rc, msg, same = call(good_off, 3, None, cand_=None)
    assert rc == -1 and same
    rc, msg, same = call(good_off, 3, None, q=None)
    assert rc == -1 and same
    rc, msg, same = call(good_off, 3, None, null_out=True)
    assert rc == -1 and same
    rc, msg, same = call(good_off, 3, None, select=5)
    assert rc == -1 and same
    for kk in (0, 2049):
        rc, msg, same = call(good_off, 3, None, kk=kk)
        assert rc == -4 and same
    assert gf.IdsBatchStats() == st0                                      # nothing ran


def test_dense_id_store(gpu):
    """A store filled through the append-only device path keeps no id table (id = first id + slot): the same equalities, ids below and
    above the stored range skipped."""
    import torch
    n, d, base = 2500, 40, 1000
    X = O.fill_normal(9800, (n, d)); X[70:120] = X[1]
    ids = np.arange(base, base + n, dtype=np.uint64)
    S = Pair(gpu, d, O.L2, O.Q_F8, ids[:1], X[:1])                        # the oracle's content; the GPU store is replaced below
    xd = torch.from_numpy(X).to("cuda:0"); torch.cuda.synchronize()
    S.gf = gpu.FlatSpace(d, O.L2, O.Q_F8); S.gf.ChangedVertexDevice(xd.data_ptr(), n, first_id=base)
    S.of.upsert(ids, X)
    Q = np.concatenate([X[1:2], O.fill_normal(9801, (11, d))])
    rng = np.random.default_rng(3)
    outside = np.concatenate([np.arange(base - 5, base, dtype=np.uint64), np.arange(base + n, base + n + 5, dtype=np.uint64)])
    lists = [rng.permutation(np.concatenate([rng.choice(ids, m, replace=False), outside])) for m in (n, 800, 33, 1)] + [outside]
    lo = rng.integers(0, len(lists), len(Q)).astype(np.uint32); lo[:5] = np.arange(5)
    for k, sel in ((10, gpu.SELECT_NEAREST), (64, gpu.SELECT_REFERENCE), (100, gpu.SELECT_NEAREST)):
        bi, bs, bc = S.check_batch(lists, Q, k, sel, lo, tag=("dense", k, sel))
        assert int(bc[4]) == 0 and int(bc[3]) == 1


def test_a_batch_large_enough_for_the_translation_threads(gpu):
    """More than 128 Ki candidate ids in one call: the lists are translated by several host threads, each list in place — unsorted lists
    with repeats and unknown ids between ascending ones, and a list nobody names in the middle."""
    n, d, nq, k = 3000, 32, 48, 10
    X = O.fill_normal(9900, (n, d)); X[10:60] = X[2]
    ids = scrambled_ids(n)
    S = Pair(gpu, d, O.COSINE, O.Q_BF16, ids, X)
    Q = np.concatenate([X[2:3], O.fill_normal(9901, (nq - 1, d))])
    rng = np.random.default_rng(11)
    unknown = np.uint64(10**13) + np.arange(40, dtype=np.uint64)
    lists = []
    for j in range(nq + 1):
        if j % 3 == 0:
            lists.append(np.sort(ids))                                                        # ascending and distinct: taken as it is
        else:
            lists.append(rng.permutation(np.concatenate([ids, ids[:600], unknown])))         # 3640 ids for 3000 rows
    lo = np.array([j if j < 20 else j + 1 for j in range(nq)], np.uint32)                    # list 20 is named by nobody
    assert sum(len(lists[j]) for j in lo) > 2 * 65536
    st0 = S.gf.IdsBatchStats()
    S.check_batch(lists, Q, k, gpu.SELECT_NEAREST, lo, tag="threads")
    assert S.gf.IdsBatchStats()["pairs"] - st0["pairs"] == nq * n
