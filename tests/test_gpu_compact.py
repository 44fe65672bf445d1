"""Hnsw.Compact (coltt_hnsw_compact; include/coltt_gpu.h, "HNSW compaction"): the tombstoned slots are dropped in place on the device and nothing a
caller can observe changes except the slot numbers.  Every index is built by the oracle and BulkLoaded, the victims are removed on both sides (as
test_gpu_hnsw.test_hnsw_remove_parity does); after Compact the export is the numpy remap of the export before, the stored bytes are the bytes
they were, the committed stream is the stream committed before, and every search gives the ids, score bits, counts and traversal counters it gave
before — which are the ORACLE's on its uncompacted, tombstoned index.  Each case runs with a 1-byte staging budget (64-row chunks: many chunk
boundaries) and with the default one."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
K = 10
NQ = 32
RUN = 150            # one contiguous dead run, longer than the 64-row minimum chunk
# name: (n, dim, metric, quantisation, explicit ids, quantiser (sub-vectors, centroids) or None, seed)
CASES = {
    "a-701x48-f32-l2-ids": (701, 48, "l2", "f32", True, None, 310),
    "b-601x256-f32-cos": (601, 256, "cos", "f32", True, None, 320),
    "c-401x256-f16-cos": (401, 256, "cos", "f16", True, None, 330),
    "d-701x48-f32-l2-dense": (701, 48, "l2", "f32", False, None, 310),
    "e-601x256-f32-cos-pq": (601, 256, "cos", "f32", True, (16, 32), 320),
}
STAGES = {"stage-1B": 1, "stage-default": 0}
EFS = (20, 128, 300)


def _del_bits(dead):
    db = np.zeros((len(dead) + 31) // 32, np.uint32)
    for s in np.flatnonzero(dead):
        db[s >> 5] |= np.uint32(1 << (s & 31))
    return db


_SHARED = {}


def _shared(name):
    """per case, built once and never changed: the data, the oracle's index with the victims removed, the removal order"""
    if name in _SHARED:
        return _SHARED[name]
    n, d, metric, quant, explicit, pqc, seed = CASES[name]
    om = O.COSINE if metric == "cos" else O.L2
    X = O.fill_normal(seed, (n, d)); lv = O.levels(seed + 1, n)
    ids = np.arange(n, dtype=np.uint64) + np.uint64(500 if explicit else 0)
    oh = O.Hnsw(d, om); oh.insert_many(ids, X, lv)
    g0 = oh.export(with_vectors=False)
    rng = np.random.default_rng(seed + 2)
    run0 = int(rng.integers(40, n - RUN - 40))
    victims = [int(v) for v in rng.choice(n, n // 4, replace=False)]
    for v in [g0["entry"], 0, n - 1] + list(range(run0, run0 + RUN)):
        if v not in victims:
            victims.append(int(v))
    dead = np.zeros(n, bool); dead[victims] = True
    # the test's own preconditions: an upper row disappears, and a live vertex's upper rows move down because of it
    dead_up = np.flatnonzero(dead & (lv >= 1))
    assert len(dead_up) > 0, "no victim of level >= 1: pick another seed"
    assert (~dead[dead_up[0]:] & (lv[dead_up[0]:] >= 1)).any(), "no live vertex of level >= 1 behind a victim of level >= 1: pick another seed"
    assert dead[run0 - 1:run0 + RUN + 1].sum() >= RUN and (~dead).sum() > 64
    for v in victims:
        assert oh.remove(ids[v]) == 0
    s = {"n": n, "d": d, "om": om, "oq": O.Q_NONE if quant == "f32" else O.Q_F16, "X": X, "lv": lv, "ids": ids, "g0": g0, "oh": oh, "victims": victims,
         "dead": dead, "Q": O.fill_normal(seed + 3, (NQ, d)), "pqc": pqc, "explicit": explicit, "oracle": {}}
    _SHARED[name] = s
    return s


def _gpu_index(gpu, s):
    """the GPU's twin of the oracle's index: same graph, same removals in the same order (+ the quantiser of case e)"""
    gh = gpu.Hnsw(s["d"], gpu.COSINE if s["om"] == O.COSINE else gpu.EUCLIDEAN, quantization=gpu.Q_NONE if s["oq"] == O.Q_NONE else gpu.Q_F16)
    g = dict(s["g0"])
    if not s["explicit"]:
        g["ids"] = None                                      # dense-id mode: slot + 0
    gh.BulkLoad(g, s["X"])
    pq = None
    if s["pqc"]:
        pq = gpu.PQSpace(s["d"], gpu.PQ_COSINE, *s["pqc"]); pq.Fit(gh.FetchRows(), iterations=3)
        gh.PqAttach(pq)
    for v in s["victims"]:
        gh.Remove(int(s["ids"][v]))
    return gh, pq


def _searches(gh, s):
    """every search kernel the issue names, with its counters (n_visit_resets left out: it depends on how slots hash)"""
    out = {}
    keep = lambda r: (r[0], bits(r[1]), r[2], {k: r[3][k] for k in ("n_dist", "n_exp", "n_hops")})
    for ef in EFS:                                           # one-wave walk at 20 and 128, the large-ef walk at 300
        out[("search", ef)] = keep(gh.Search(s["Q"], K, ef=ef, with_stats=True))
    out[("one", 64)] = keep(gh.Search(s["Q"][:1], K, ef=64, with_stats=True))   # nq == 1: the latency kernel
    if s["pqc"]:
        r = gh.PqSearch(s["Q"], K, ef=128, rerank=64, with_stats=True)
        out[("pq", 128)] = (r[0], bits(r[1]), r[2], {k: r[3][k] for k in ("n_dist", "n_exp", "n_hops", "n_exact")})
    return out


def _same(a, b, tag):
    assert a.keys() == b.keys()
    for key in a:
        (ai, as_, ac, ast), (bi, bs, bc, bst) = a[key], b[key]
        assert np.array_equal(ac, bc), (tag, key, "counts")
        for q in range(len(ac)):
            c = int(ac[q])
            assert np.array_equal(ai[q, :c], bi[q, :c]), (tag, key, q, "ids")
            assert np.array_equal(as_[q, :c], bs[q, :c]), (tag, key, q, "score bits")
        assert ast == bst, (tag, key, ast, bst)


def _oracle_answers(s, gh_before, before):
    """the oracle's answers on the UNCOMPACTED, tombstoned index, in the shape of _searches.  f32 rows: the oracle's own index object (built and
    removed from independently of the GPU).  2-byte rows and the walk over the quantiser's codes: the oracle's search over the arrays the GPU
    held before the call, tombstone bitmap included."""
    if s["oracle"]:
        return s["oracle"]
    out = {}
    Q = s["Q"]
    if s["oq"] == O.Q_NONE:
        for key, qs in [(("search", ef), Q) for ef in EFS] + [(("one", 64), Q[:1])]:
            ids = np.zeros((len(qs), K), np.uint64); sc = np.zeros((len(qs), K), np.float32); cnt = np.zeros(len(qs), np.uint32)
            tot = {"n_dist": 0, "n_exp": 0, "n_hops": 0}
            for q in range(len(qs)):
                wi, ws, st = s["oh"].search(qs[q], K, mode=1, ef=key[1], with_stats=True)
                ids[q, :len(wi)] = wi; sc[q, :len(wi)] = ws; cnt[q] = len(wi)
                for k in tot:
                    tot[k] += st[k]
            out[key] = (ids, bits(sc), cnt, tot)
    raw, rows, ex = before["raw"], before["rows"], before["export"]
    db = _del_bits(ex["deleted"].astype(bool))
    def by_slot(sl, sc, cn):
        ids = np.zeros(sl.shape, np.uint64)
        for q in range(len(cn)):
            ids[q, :cn[q]] = ex["ids"][sl[q, :cn[q]]]
        return ids, bits(sc), cn.astype(np.uint32)
    if s["oq"] != O.Q_NONE:
        for key, qs in [(("search", ef), Q) for ef in EFS] + [(("one", 64), Q[:1])]:
            sl, sc, cn, st, _ = O.csr_search(rows, s["oq"], raw["adj0"], raw["upper_off"], raw["adjU"], s["d"], s["om"], raw["entry"], raw["entry_level"],
                                             qs, K, key[1], del_bits=db, threads=2)
            out[key] = by_slot(sl, sc, cn) + (st,)
    if s["pqc"]:
        sl, sc, cn, st, _ = O.csr_search_pq(rows, s["oq"], raw["adj0"], raw["upper_off"], raw["adjU"], s["d"], s["om"], raw["entry"], raw["entry_level"],
                                            before["codes"], before["cb"], O.PQ_COSINE, Q, K, 128, rerank=64, del_bits=db, threads=2)
        out[("pq", 128)] = by_slot(sl, sc, cn) + (st,)
    s["oracle"] = out
    return out


def _remap(ex):
    """the definition, in numpy: the export an order-preserving compaction of export `ex` must give, and the edges it drops"""
    live = ex["deleted"] == 0
    new = (np.cumsum(live) - live).astype(np.int64)
    lv = ex["levels"]
    row_owner = np.repeat(np.arange(len(lv)), lv + 1)                      # the slot of every adjacency row, in row order
    deg = np.diff(ex["row_offsets"])
    edge_row = np.repeat(np.arange(len(deg)), deg)
    keep_edge = live[row_owner[edge_row]] & live[ex["nbr"]]
    dropped = int((live[row_owner[edge_row]] & ~live[ex["nbr"]]).sum())
    keep_row = live[row_owner]
    new_deg = np.bincount(edge_row[keep_edge], minlength=len(deg))[keep_row]
    return {"ids": ex["ids"][live], "levels": lv[live], "deleted": np.zeros(int(live.sum()), np.uint8),
            "row_offsets": np.concatenate([[0], np.cumsum(new_deg)]).astype(np.int64), "nbr": new[ex["nbr"][keep_edge]].astype(np.int32),
            "nbr_dist": ex["nbr_dist"][keep_edge], "entry": int(new[ex["entry"]])}, dropped, new, live


def _export_equal(a, b, tag):
    for k in ("ids", "levels", "deleted", "row_offsets", "nbr"):
        assert np.array_equal(a[k], b[k]), (tag, k)
    assert np.array_equal(bits(a["nbr_dist"]), bits(b["nbr_dist"])), (tag, "edge distances")
    assert a["entry"] == b["entry"], tag


def _expected_blocks(h):
    """test_gpu_pq_nbr_patch.expected_blocks: the code row of every listed level-0 neighbour, zeros elsewhere"""
    adj0 = h.ExportRaw()["adj0"]; codes = h.PqCodes()
    row = (codes.shape[1] + 15) & ~15
    padded = np.zeros((codes.shape[0], row), np.uint8); padded[:, :codes.shape[1]] = codes
    want = np.zeros(adj0.shape + (row,), np.uint8)
    want[adj0 != NONE] = padded[adj0[adj0 != NONE]]
    return want


@pytest.mark.parametrize("stage", list(STAGES), ids=list(STAGES))
@pytest.mark.parametrize("name", list(CASES), ids=list(CASES))
def test_compact_changes_nothing_but_the_slot_numbers(gpu, name, stage):
    import torch
    s = _shared(name)
    gh, pq = _gpu_index(gpu, s)
    n, d = s["n"], s["d"]
    # ---- before
    before = {"export": gh.Export(), "raw": gh.ExportRaw(), "rows": gh.FetchRows(), "len": gh.Len()}
    _export_equal({k: v for k, v in before["export"].items()}, dict(s["oh"].export(with_vectors=False), ids=before["export"]["ids"]), "removal parity")
    assert np.array_equal(before["export"]["deleted"].astype(bool), s["dead"])
    if s["explicit"]:
        assert np.array_equal(before["export"]["ids"], s["ids"])
    if s["pqc"]:
        before["codes"] = gh.PqCodes(); before["cb"] = pq.Codebooks()
    shadow8 = 8 in gh.RowFilterStats()["shadow_bits"]
    if name.startswith("b") or name.startswith("e"):
        assert shadow8, "a line-transposed f32 cosine index of dim 256 keeps the 8-bit shadow"
    if shadow8:
        before["shadow"] = gh.FetchShadow8()
    commit_before = gh.Commit() if name[0] in "abc" else None
    got_before = _searches(gh, s)
    _same(got_before, _oracle_answers(s, gh, before), "before vs the oracle")
    allow_ids = s["ids"][::3]
    flt_old = gh.Filter(allow_ids)
    filt_before = {m: gh.SearchFiltered(s["Q"], K, flt_old, ef=64, mode=m) for m in (gpu.FILTER_WALK, gpu.FILTER_EXACT)}
    want, dropped, new, live = _remap(before["export"])
    # ---- the call
    st, nmap = gh.Compact(stage_bytes=STAGES[stage], with_map=True)
    print(f"[{name} {stage}] {st}")
    # 1. the export is the numpy remap of the export before; the stats and the map say what happened
    after = gh.Export()
    _export_equal(after, want, "export after")
    assert gh.Len() == before["len"] == st["slots_after"] == int(live.sum())
    assert st["slots_before"] == n and st["edges_dropped"] == dropped
    assert st["upper_rows_before"] == int(before["export"]["levels"].sum()) and st["upper_rows_after"] == int(want["levels"].sum())
    assert st["rows_moved"] == int((live & (new != np.arange(n))).sum()) and st["bytes_moved"] > 0
    assert np.array_equal(nmap, np.where(live, new, NONE).astype(np.uint32))
    raw = gh.ExportRaw()
    lvl = want["levels"].astype(np.int64)
    assert np.array_equal(raw["upper_off"], np.where(lvl > 0, np.cumsum(lvl) - lvl, NONE).astype(np.uint32))
    # 2. per-slot data: the bytes they were
    assert np.array_equal(gh.FetchRows().view(np.uint8), before["rows"][live].view(np.uint8))
    if shadow8:
        codes, meta, adj_meta = gh.FetchShadow8()
        assert np.array_equal(codes, before["shadow"][0][live]) and np.array_equal(bits(meta), bits(before["shadow"][1][live]))
        a0 = raw["adj0"]                                     # the pairs riding with the level-0 rows: the neighbour's own pair, zeros where empty
        want_adj = np.zeros(a0.shape + (2,), np.float32); want_adj[a0 != NONE] = meta[a0[a0 != NONE]]
        assert np.array_equal(bits(adj_meta), bits(want_adj))
    # 3. the committed stream is byte for byte the one committed before
    if commit_before is not None:
        assert gh.Commit() == commit_before
    # 4. every search: as before, i.e. as the oracle on its tombstoned index
    got_after = _searches(gh, s)
    _same(got_after, got_before, "after vs before")
    _same(got_after, s["oracle"], "after vs the oracle")
    if s["pqc"]:
        assert np.array_equal(gh.PqCodes(), before["codes"][live])
        gh.PqSearch(s["Q"], K, ef=300)                       # a walk that reads the neighbourhood blocks rebuilds them
        assert gh.PqNbrStats()["state"] == 1
        assert np.array_equal(gh.PqFetchNbr(), _expected_blocks(gh))
    # 5. filters: the old one is stale, one re-created from the same ids answers as before
    with pytest.raises(gpu.ColttError) as e:
        gh.SearchFiltered(s["Q"], K, flt_old, ef=64, mode=gpu.FILTER_WALK)
    assert e.value.code == -1
    with gh.Filter(allow_ids) as flt_new:
        assert flt_new.allowed == flt_old.allowed
        for m, (bi, bs, bc) in filt_before.items():
            ai, as_, ac = gh.SearchFiltered(s["Q"], K, flt_new, ef=64, mode=m)
            assert np.array_equal(ac, bc) and all(np.array_equal(ai[q, :ac[q]], bi[q, :ac[q]]) and np.array_equal(bits(as_[q, :ac[q]]), bits(bs[q, :ac[q]]))
                                                 for q in range(NQ)), ("filtered", m)
    flt_old.close()
    # 6. mutations afterwards: the freed tail is filled, ids keep resolving
    Y = O.fill_normal(901, (50, d)); ly = O.levels(902, 50)
    yd = torch.from_numpy(Y).cuda(); torch.cuda.synchronize()
    nid = np.arange(50, dtype=np.uint64) + np.uint64(10000)
    gone = [int(i) for i in after["ids"][5:45:2]]
    if s["oq"] == O.Q_NONE:
        g = dict(after); g["vectors"] = gh.FetchRows()
        twin = O.Hnsw(d, s["om"]); twin.load(g)
        for i in range(50):
            assert twin.insert(nid[i], Y[i], ly[i]) == 0
        for i in gone:
            assert twin.remove(i) == 0
        insert = lambda h: h.InsertBatchDevice(yd.data_ptr(), 50, ly, batch=1, ids=None if name.startswith("d") else nid, first_id=10000)
        twin_export = lambda: twin.export(with_vectors=False)
    else:
        # 2-byte rows: the oracle has no cosine index over codes, so the twin is a fresh GPU index BulkLoaded with the compacted graph
        twin = gpu.Hnsw(d, gpu.COSINE, quantization=gpu.Q_F16); twin.BulkLoad(after, s["X"][live])
        assert np.array_equal(twin.FetchRows(), gh.FetchRows())
        insert = lambda h: h.InsertBatchDevice(yd.data_ptr(), 50, ly, batch=1, ids=nid)
        insert(twin)
        for i in gone:
            twin.Remove(i)
        twin_export = twin.Export
    insert(gh)                                               # case d: ids == NULL, first_id = 10000 on what is now an explicit-id index
    for i in gone:
        gh.Remove(i)
    final = gh.Export()
    _export_equal(final, dict(twin_export(), ids=final["ids"]), "mutations after")
    assert np.array_equal(final["ids"], np.concatenate([after["ids"], nid]))
    assert gh.Len() == before["len"] + 50 - len(gone)
    row, level = gh.Get(10007)
    assert level == ly[7] and np.array_equal(row, gh.FetchRows(len(after["ids"]) + 7, 1)[0])


def _small(gpu, n=300, d=32, seed=77, remove=0):
    X = O.fill_normal(seed, (n, d)); lv = O.levels(seed + 1, n); ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(11)
    oh = O.Hnsw(d, O.L2); oh.insert_many(ids, X, lv)
    gh = gpu.Hnsw(d, gpu.EUCLIDEAN); gh.BulkLoad(oh.export(with_vectors=False), X)
    for i in np.random.default_rng(seed).choice(n, remove, replace=False):
        gh.Remove(int(ids[i]))
    return gh, X, ids, lv


def test_compact_without_tombstones_is_a_noop(gpu):
    gh, X, ids, lv = _small(gpu)
    Q = O.fill_normal(5, (8, 32))
    flt = gh.Filter(ids[::2])
    want = gh.SearchFiltered(Q, K, flt, ef=40, mode=gpu.FILTER_WALK)
    ex = gh.Export()
    st, nmap = gh.Compact(with_map=True)
    assert st["slots_before"] == st["slots_after"] == 300 and st["rows_moved"] == st["bytes_moved"] == st["edges_dropped"] == 0 and st["ms"] == 0.0
    assert np.array_equal(nmap, np.arange(300, dtype=np.uint32))
    got = gh.SearchFiltered(Q, K, flt, ef=40, mode=gpu.FILTER_WALK)       # the filter built before is still valid
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    _export_equal(gh.Export(), ex, "no-op")
    # twice in a row: the second call is that no-op
    for v in (0, 17, 299):
        gh.Remove(int(ids[v]))
    first = gh.Compact()
    assert first["slots_after"] == 297 and first["rows_moved"] == 297 and first["ms"] > 0.0
    ex2 = gh.Export()
    flt2 = gh.Filter(ids[::2])
    second = gh.Compact(stage_bytes=1)
    assert second["slots_before"] == second["slots_after"] == 297 and second["rows_moved"] == second["bytes_moved"] == 0
    _export_equal(gh.Export(), ex2, "second call")
    gh.SearchFiltered(Q, K, flt2, ef=40, mode=gpu.FILTER_WALK)            # not stale: the second call renumbered nothing


def test_compact_all_dead_gives_the_empty_index(gpu):
    gh, X, ids, lv = _small(gpu, n=100)
    for i in ids:
        gh.Remove(int(i))
    assert gh.Len() == 0
    st, nmap = gh.Compact(with_map=True)
    assert st["slots_before"] == 100 and st["slots_after"] == 0 and st["upper_rows_after"] == 0 and (nmap == NONE).all()
    ex = gh.Export()
    assert gh.Len() == 0 and len(ex["ids"]) == 0 and len(ex["nbr"]) == 0
    assert (gh.Search(X[:3], 5)[2] == 0).all()
    # Inserts afterwards: the same graph a fresh index builds, and no tombstone of the old life shows through after a Remove
    fresh = gpu.Hnsw(32, gpu.EUCLIDEAN)
    for h in (gh, fresh):
        for i in range(40):
            h.Insert(int(ids[i]), X[i], int(lv[i]))
        h.Remove(int(ids[3]))
    _export_equal(gh.Export(), fresh.Export(), "after all-dead")
    a, b = gh.Search(X[:8], 5, ef=30), fresh.Search(X[:8], 5, ef=30)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_compact_refuses_a_short_map_before_anything_runs(gpu):
    from coltt_amd._lib import vp
    gh, X, ids, lv = _small(gpu, remove=40)
    ex = gh.Export()
    m = np.zeros(299, np.uint32)
    rc = gpu.lib().coltt_hnsw_compact(gh.h, C.c_uint64(0), vp(m), C.c_uint64(299), None)
    assert rc == -1 and b"map" in gpu.lib().coltt_last_error()
    _export_equal(gh.Export(), ex, "refused")
    assert gh.Len() == 260 and gh.Export()["deleted"].sum() == 40
    assert gpu.lib().coltt_hnsw_compact(gh.h, C.c_uint64(0), None, C.c_uint64(0), None) == 0    # no map, no stats: fine
    assert len(gh.Export()["ids"]) == 260


def test_readers_see_the_same_answers_while_the_index_is_compacted(gpu):
    """four threads search without pause while the main thread compacts once: searches hold the lock shared, the call takes it exclusive, and the
    answers are invariant — every answer any reader gets equals the expected one."""
    s = _shared("a-701x48-f32-l2-ids")
    gh, _ = _gpu_index(gpu, s)
    Q = s["Q"]
    want = gh.Search(Q, K, ef=64)
    stop = threading.Event(); bad = []; rounds = [0] * 4

    def reader(t):
        try:
            while not stop.is_set():
                lo = (t * 8) % NQ
                gi, gs, gc = gh.Search(Q[lo:lo + 8], K, ef=64)
                if not (np.array_equal(gc, want[2][lo:lo + 8]) and np.array_equal(gi, want[0][lo:lo + 8]) and np.array_equal(bits(gs), bits(want[1][lo:lo + 8]))):
                    bad.append((t, rounds[t]))
                rounds[t] += 1
        except Exception as e:   # noqa: BLE001
            bad.append((t, repr(e)))

    th = [threading.Thread(target=reader, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    try:
        while min(rounds) < 20:
            stop.wait(0.001)
        st = gh.Compact(stage_bytes=1)
        seen = list(rounds)
        while min(r - r0 for r, r0 in zip(rounds, seen)) < 20 and not bad:
            stop.wait(0.001)
    finally:
        stop.set()
        for t in th:
            t.join()
    assert st["slots_after"] == gh.Len() and not bad, bad[:4]
