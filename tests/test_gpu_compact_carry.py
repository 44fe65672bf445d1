"""Hnsw.CompactCarry (coltt_hnsw_compact_carry; include/coltt_gpu.h, "Carrying resident filters and attribute columns through a compaction"): the
compaction of test_gpu_compact.py, after which the LISTED filters and columns are valid under the same handles and answer as before.
1. the kernels alone (carry_bits_device) against the host definition and numpy; 2. index level, on the shapes and victims of test_gpu_compact.py;
3. the edges (no tombstones, rejected calls, duplicates, all dead); 4. readers and filter_info during the call."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits
from carry_ref import N_BIG, TILE_SLOTS, carry_numpy, dead_patterns, pack, unpack
from test_gpu_compact import _shared

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
K = 10
EXTRA = 40           # vertices inserted after the early objects were made: their coverage lies below n
INVALID, NOT_FOUND = -1, -3


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
def _source_bitmaps(n, nb, dead, rng):
    """nb bitmaps over n slots: all ones (stray bits past n included), exactly the dead slots, then random densities"""
    words = (n + 31) // 32
    b = np.zeros((nb, words), np.uint32)
    b[0] = 0xFFFFFFFF
    if nb > 1:
        b[1] = pack(dead)
    for p in range(2, nb):
        b[p] = pack(rng.random(n) < (0.003, 0.3, 0.5, 0.97)[p % 4])
    return b


@pytest.mark.parametrize("nb", [1, 3, 65])
def test_kernels_alone_equal_the_host_definition_and_numpy(gpu, nb):
    n = N_BIG
    rng = np.random.default_rng(700 + nb)
    seen_wide = seen_straddle = False
    for pname, dead in dead_patterns(n).items():
        dw = pack(dead)
        b = _source_bitmaps(n, nb, dead, rng)
        live = int((~dead).sum())
        oon = np.flatnonzero(~dead)
        # ---- the test's own preconditions
        bounds = np.arange(TILE_SLOTS, live, TILE_SLOTS)          # the output tile boundaries: new slots B - 1 | B
        if pname == "none":
            assert len(bounds) == 3 and live % 32 == 5            # three full tiles and a ragged word
        if pname == "run-40000":
            lo, hi = np.flatnonzero(dead)[[0, -1]]
            assert hi - lo + 1 == 40000 > TILE_SLOTS and lo // TILE_SLOTS != hi // TILE_SLOTS       # longer than a tile, across a tile boundary
            src = oon[min(TILE_SLOTS, live) - 1] - oon[0] + 1     # what output tile 0 reads
            assert src > 2 * TILE_SLOTS, src
            seen_wide = True
        if len(bounds) and pname != "all":
            surv = unpack(b[0], n)[~dead]                         # bitmap 0 allows every slot: its survivors sit on both sides of every boundary
            assert surv[bounds - 1].all() and surv[bounds].all()
            if ((oon[bounds - 1] >> 5) == (oon[bounds] >> 5)).all():
                seen_straddle = True                              # at every boundary one source word's two pieces land in two tiles
        # ---- device == host == numpy
        out, allowed, lists = gpu.carry_bits_device(b, dw, n, with_lists=True)
        assert out.shape == (nb, (live + 31) // 32)
        for p in range(nb):
            want = carry_numpy(b[p], dead, n)
            host = gpu.carry_bits_host(b[p], dw, n)
            assert host[1:] == want[1:] and np.array_equal(host[0], want[0]), (pname, p, "host")
            assert int(allowed[p]) == want[1], (pname, p, int(allowed[p]), want[1])
            assert np.array_equal(out[p], want[0]), (pname, p, "words", np.flatnonzero(out[p] != want[0])[:8])
            assert np.array_equal(lists[p], np.flatnonzero(unpack(want[0], live)).astype(np.uint32)), (pname, p, "list")
        if nb > 1 and live:
            assert allowed[1] == 0 and allowed[0] == live         # bits on dead slots and past n do not survive
    assert seen_wide and seen_straddle


def test_kernels_alone_short_bitmaps_and_no_tombstones(gpu):
    n = N_BIG
    rng = np.random.default_rng(5)
    dead = dead_patterns(n)["random-0.5"]
    for words in (0, 1, 1023, 1024, 1025, (n + 31) // 32 - 1):   # coverage below n: the words the bitmap lacks read as 0
        b = np.stack([pack(rng.random(n) < 0.5)[:words], np.full(words, 0xFFFFFFFF, np.uint32)])
        for dw, dd in ((pack(dead), dead), (None, np.zeros(n, bool))):
            out, allowed, lists = gpu.carry_bits_device(b, dw, n, with_lists=True)
            for p in range(2):
                want = carry_numpy(b[p], dd, n)
                assert int(allowed[p]) == want[1] and np.array_equal(out[p], want[0]), (words, dw is None, p)
                assert np.array_equal(lists[p], np.flatnonzero(unpack(want[0], want[2])).astype(np.uint32))
    out, allowed = gpu.carry_bits_device(np.zeros((3, 4), np.uint32), pack(np.ones(100, bool)), 100)   # nothing survives: nothing is launched
    assert out.shape == (3, 0) and (allowed == 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. index level
CARRY_CASES = ["a-701x48-f32-l2-ids", "d-701x48-f32-l2-dense", "c-401x256-f16-cos", "e-601x256-f32-cos-pq"]
STAGES = {"stage-1B": 1, "stage-default": 0}


def _build(gpu, s):
    """the oracle's graph BulkLoaded (+ the quantiser of case e), no victim removed yet"""
    gh = gpu.Hnsw(s["d"], gpu.COSINE if s["om"] == O.COSINE else gpu.EUCLIDEAN, quantization=gpu.Q_NONE if s["oq"] == O.Q_NONE else gpu.Q_F16)
    g = dict(s["g0"])
    if not s["explicit"]:
        g["ids"] = None
    gh.BulkLoad(g, s["X"])
    pq = None
    if s["pqc"]:
        pq = gpu.PQSpace(s["d"], gpu.PQ_COSINE, *s["pqc"]); pq.Fit(gh.FetchRows(), iterations=3)
        gh.PqAttach(pq)
    return gh, pq


def _insert(gh, Y, first_id, dense=False):
    """len(Y) level-0 vertices behind the last slot (level 0: the upper layers, hence the entrypoint elections of the removes, stay the oracle's);
    dense: ids == NULL, the ids continue the slots"""
    import torch
    yd = torch.from_numpy(np.ascontiguousarray(Y, np.float32)).cuda(); torch.cuda.synchronize()
    ids = np.arange(len(Y), dtype=np.uint64) + np.uint64(first_id)
    gh.InsertBatchDevice(yd.data_ptr(), len(Y), np.zeros(len(Y), np.int32), batch=1, ids=None if dense else ids, first_id=int(first_id))
    return ids


def _slots(gh):
    """the slot count, tombstones included"""
    return gh.ExportRaw()["n"]


def _answers(gpu, gh, s, flt, pq):
    """every filtered entry point over one filter: ids, score bits, counts, path, the traversal counters (not ef_walk and n_exact_rows: they follow
    the allowed count, which for a filter made before the removes counted the victims)"""
    Q = s["Q"]
    out = {}
    keep = lambda r: (r[0], bits(r[1]), r[2], {k: r[3][k] for k in ("n_dist", "n_exp", "n_hops", "path")})
    out["walk"] = keep(gh.SearchFiltered(Q, K, flt, ef=40, mode=gpu.FILTER_WALK, with_stats=True))
    out["exact"] = keep(gh.SearchFiltered(Q, K, flt, mode=gpu.FILTER_EXACT, with_stats=True))
    out["auto"] = keep(gh.SearchFiltered(Q, K, flt, ef=40, mode=gpu.FILTER_AUTO, with_stats=True))
    r = gh.SearchFilteredBatch(Q[:8], K, [flt] * 8, ef=40, mode=gpu.FILTER_AUTO, with_stats=True)
    out["batch"] = (r[0], bits(r[1]), r[2], dict({k: r[4][k] for k in ("n_dist", "n_exp", "n_hops", "path")}, paths=r[3].tolist()))
    if pq is not None:
        out["pq"] = keep(gh.PqSearchFiltered(Q, K, flt, ef=64, rerank=32, mode=gpu.FILTER_WALK, with_stats=True))
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


def _equal_as_sets(gpu, gh, f, g):
    """two filters of one index allow the same vertices: F G ANDNOT and G F ANDNOT both allow nothing"""
    a, b = gh.FilterEvalBatch([[0, 1, gpu.FOP_ANDNOT], [1, 0, gpu.FOP_ANDNOT]], [f, g])
    return a.allowed == 0 and b.allowed == 0 and f.info()["allowed"] == g.info()["allowed"]


def _stale(gpu, fn):
    with pytest.raises(gpu.ColttError) as e:
        fn()
    return e.value.code == INVALID


@pytest.mark.parametrize("stage", list(STAGES), ids=list(STAGES))
@pytest.mark.parametrize("name", CARRY_CASES, ids=CARRY_CASES)
def test_listed_objects_answer_as_before_under_the_same_handles(gpu, name, stage):
    s = _shared(name)
    n, d = s["n"], s["d"]
    gh, pq = _build(gpu, s)
    rng = np.random.default_rng(s["n"] + 9)
    ids0 = s["ids"]
    # ---- objects made BEFORE the removes; the early ones when the index had EXTRA fewer slots
    f_early = gh.Filter(ids0[rng.random(n) < 0.5])
    c2 = gh.AttrColumn(gpu.ATTR_F64)
    sub = np.flatnonzero(rng.random(n) < 0.6)
    v2 = rng.normal(size=len(sub))
    assert c2.set(ids0[sub], v2) == len(sub)
    xid = _insert(gh, O.fill_normal(4242, (EXTRA, d)), 20000 if s["explicit"] else n, dense=not s["explicit"])
    ids = np.concatenate([ids0, xid]); nt = n + EXTRA
    assert _slots(gh) == nt and f_early.info()["slots"] == n == c2.info()["slots"]
    dead = np.concatenate([s["dead"], np.zeros(EXTRA, bool)])
    in_f1 = rng.random(nt) < 0.3
    assert (in_f1 & dead).any()                                                   # F1 allows victims
    f1 = gh.Filter(ids[in_f1])
    c1 = gh.AttrColumn(gpu.ATTR_I64)
    v1 = rng.integers(-1000, 1000, nt)
    assert c1.set(ids, v1) == nt
    c_never = gh.AttrColumn(gpu.ATTR_I64)
    c_unlisted = gh.AttrColumn(gpu.ATTR_I64); c_unlisted.set(ids[:10], np.arange(10))
    for v in s["victims"]:
        gh.Remove(int(ids[v]))
    live_ids = ids[~dead]
    # ---- objects made AFTER the removes
    f2 = gh.Filter(live_ids[::3])
    sib_a, sib_b = gh.FilterEvalBatch([[0, gpu.FOP_NOT], [0, 1, gpu.FOP_AND]], [f1, f2])   # two outputs of one call share a slab
    f_empty = gh.Filter(np.zeros(0, np.uint64))
    carried_f = [f1, f_early, f2, sib_a, f_empty]
    carried_c = [c1, c2, c_never]
    # ---- recorded before the call
    t = 0
    pred = lambda: gh.FilterEvalAttr([1, 0, gpu.FOP_AND], [f1], [(c1, gpu.CMP_LT, t)])    # C1 < t AND F1
    before = {i: _answers(gpu, gh, s, f, pq) for i, f in enumerate(carried_f)}
    # (filter_ids lists what the filter allows, tombstoned since or not: of a filter made before the removes, the live part is what is carried)
    fids = [f.ids() for f in carried_f]
    fids = [x[~np.isin(x, ids[dead])] for x in fids]
    assert len(fids[0]) < f1.info()["allowed"] and len(fids[1]) < f_early.info()["allowed"]
    got1, set1 = c1.get(ids); got2, set2 = c2.get(ids)
    assert set1[~dead].all() and not set1[dead].any()
    with pred() as p0, gh.FilterEval([0, gpu.FOP_NOT], [f1]) as not0:
        pred_ids, not_ids = p0.ids(), not0.ids()
    infos = [f.info() for f in carried_f]
    # ---- the call: duplicates in both lists
    st, cs, allowed, nset, nmap = gh.CompactCarry(filters=carried_f + [f1], columns=carried_c + [c2], stage_bytes=STAGES[stage], with_map=True)
    print(f"[{name} {stage}] {st} {cs}")
    live = ~dead
    new = (np.cumsum(live) - live)
    assert np.array_equal(nmap, np.where(live, new, NONE).astype(np.uint32)) and st["slots_after"] == int(live.sum()) == gh.Len()
    assert cs["filters"] == len(carried_f) and cs["columns"] == len(carried_c) and cs["ms"] > 0.0
    assert cs["bitmap_words"] == (len(carried_f) + len(carried_c)) * ((int(live.sum()) + 31) // 32)
    # ---- the same handles: every recorded answer
    for i, f in enumerate(carried_f):
        _same(_answers(gpu, gh, s, f, pq), before[i], f"filter {i}")
        assert np.array_equal(f.ids(), fids[i]), i
        inf = f.info()
        assert inf["allowed"] == allowed[i] == len(fids[i]) == f.allowed
        assert inf["slots"] == int(live[:infos[i]["slots"]].sum())                # new(F.slots)
        with gh.Filter(fids[i]) as g:                                             # re-created from those ids on the compacted index
            assert g.allowed == inf["allowed"] and _equal_as_sets(gpu, gh, f, g), i
    assert allowed[len(carried_f)] == allowed[0]                                  # the duplicate reports the same object
    assert cs["list_entries"] == sum(len(x) for x in fids)
    assert f_empty.info()["allowed"] == 0 and f_early.info()["slots"] == int(live[:n].sum()) < gh.Len()
    # columns: attr_get by id, n_set, the coverage
    a1, s1 = c1.get(ids); a2, s2 = c2.get(ids)
    assert np.array_equal(a1[live], got1[live]) and np.array_equal(s1[live], set1[live]) and not s1[dead].any() and not a1[dead].any()
    assert np.array_equal(a2[live].view(np.uint64), got2[live].view(np.uint64)) and np.array_equal(s2[live], set2[live]) and not s2[dead].any()
    assert np.array_equal(a1[live], v1[live])
    i1, i2, i3 = c1.info(), c2.info(), c_never.info()
    assert i1["set"] == int(set1[live].sum()) == nset[0] and i1["slots"] == int(live.sum()) and i1["type"] == gpu.ATTR_I64
    assert i2["set"] == int(set2[live].sum()) == nset[1] == nset[3] and i2["slots"] == int(live[:n].sum()) and i2["type"] == gpu.ATTR_F64
    assert i3["set"] == 0 == nset[2] and i3["slots"] == 0 and not c_never.get(ids)[1].any()
    with pred() as p1, gh.FilterEval([0, gpu.FOP_NOT], [f1]) as not1:
        assert np.array_equal(p1.ids(), pred_ids) and np.array_equal(not1.ids(), not_ids)
    with gh.FilterEvalAttr([0], [], [(c2, gpu.CMP_GT, 0.0)]) as p2:               # a predicate over the column whose coverage lay below n
        want = ids[:n][sub][(v2 > 0.0) & live[:n][sub]]
        assert np.array_equal(np.sort(p2.ids()), np.sort(want))
    # what was not listed is stale
    assert _stale(gpu, lambda: sib_b.ids()) and _stale(gpu, lambda: c_unlisted.get(ids[:3]))
    assert _stale(gpu, lambda: gh.SearchFiltered(s["Q"], K, sib_b, ef=40))
    # ---- life goes on: the freed tail is filled, C1 grows over it, NOT F1 sees the new vertices and F1 does not
    yid = _insert(gh, O.fill_normal(4343, (50, d)), 30000)
    assert c1.set(yid, np.arange(50) + 5000) == 50 and c1.info()["slots"] == int(live.sum()) + 50
    with gh.FilterEval([0, gpu.FOP_NOT], [f1]) as not2:
        assert set(yid.tolist()) <= set(not2.ids().tolist())
    assert not set(yid.tolist()) & set(f1.ids().tolist())
    ex1 = gh.Export()
    entry_id = ex1["ids"][gh.ExportRaw()["entry"]]                                # (stays: no election among the dead)
    drop1 = fids[0][fids[0] != entry_id][:7]
    # coverages that now lie BELOW the slot count, inside the first live slots: F1 and its sibling cover the slots of before the inserts, C2 the
    # ones that were below n.  Two victims in the ragged last word of each coverage: new(coverage) must count them out
    cov_f, cov_c = f1.info()["slots"], c2.info()["slots"]
    assert cov_f == int(live.sum()) and cov_c == int(live[:n].sum()) < cov_f < _slots(gh) and cov_f % 32 >= 2 and cov_c % 32 >= 2
    ragged = np.array([ex1["ids"][c - k] for c in (cov_f, cov_c) for k in (1, 2)], np.uint64)
    gone = np.unique(np.concatenate([yid[::2], drop1, ragged[ragged != entry_id]]))
    for i in gone:
        gh.Remove(int(i))
    dead2 = gh.Export()["deleted"].astype(bool)
    for c in (cov_f, cov_c):
        assert dead2[c & ~31:c].any()                                             # the precondition: a tombstone below the coverage in its own word
    keep1 = fids[0][~np.isin(fids[0], gone)]
    b1 = _answers(gpu, gh, s, f1, pq)
    all_ids = np.concatenate([ids[live], yid])
    w1, ws1 = c1.get(all_ids); w2, ws2 = c2.get(all_ids)
    st2, cs2, al2, ns2 = gh.CompactCarry(filters=[f1, sib_a], columns=[c1, c2], stage_bytes=STAGES[stage])   # a carry of carried objects
    assert st2["slots_after"] == int(live.sum()) + 50 - len(gone) == gh.Len() and al2[0] == len(keep1)
    assert np.array_equal(f1.ids(), keep1)
    # new(coverage) = the live slots that were below it
    assert f1.info()["slots"] == sib_a.info()["slots"] == int((~dead2[:cov_f]).sum()) < cov_f
    assert c2.info()["slots"] == int((~dead2[:cov_c]).sum()) < cov_c
    assert c1.info()["slots"] == int((~dead2).sum())
    _same(_answers(gpu, gh, s, f1, pq), b1, "second carry")
    x1, xs1 = c1.get(all_ids); x2, xs2 = c2.get(all_ids)
    alive = ~np.isin(all_ids, gone)
    assert np.array_equal(x1[alive], w1[alive]) and np.array_equal(xs1[alive], ws1[alive]) and not xs1[~alive].any() and ns2[0] == int(xs1.sum())
    assert np.array_equal(x2[alive].view(np.uint64), w2[alive].view(np.uint64)) and np.array_equal(xs2[alive], ws2[alive]) and not xs2[~alive].any()
    assert ns2[1] == int(xs2.sum()) == c2.info()["set"]
    assert _stale(gpu, lambda: f2.ids())                                          # carried the first time, not listed the second
    for o in carried_f + carried_c + [sib_b, c_unlisted]:
        o.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. edges
def _small(gpu, n=300, d=32, seed=77, remove=0):
    X = O.fill_normal(seed, (n, d)); lv = O.levels(seed + 1, n); ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(11)
    oh = O.Hnsw(d, O.L2); oh.insert_many(ids, X, lv)
    gh = gpu.Hnsw(d, gpu.EUCLIDEAN); gh.BulkLoad(oh.export(with_vectors=False), X)
    ent = oh.export(with_vectors=False)["entry"]
    pool = np.setdiff1d(np.arange(n), [ent])                                     # (the entrypoint stays: no election among the dead)
    for i in np.random.default_rng(seed).choice(pool, remove, replace=False):
        gh.Remove(int(ids[i]))
    return gh, X, ids, lv


def test_without_tombstones_nothing_is_launched_and_the_objects_stay_valid(gpu):
    gh, X, ids, lv = _small(gpu)
    Q = O.fill_normal(5, (8, 32))
    f = gh.Filter(ids[::2]); c = gh.AttrColumn(gpu.ATTR_I64); c.set(ids, np.arange(300))
    want = gh.SearchFiltered(Q, K, f, ef=40, mode=gpu.FILTER_WALK)
    st, cs, al, ns, nmap = gh.CompactCarry([f], [c], with_map=True)
    assert st["slots_before"] == st["slots_after"] == 300 and st["bytes_moved"] == 0 and st["ms"] == 0.0
    assert cs["ms"] == 0.0 and cs["bitmap_words"] == cs["list_entries"] == cs["column_values"] == 0
    assert np.array_equal(nmap, np.arange(300, dtype=np.uint32)) and al[0] == 150 and ns[0] == 300
    got = gh.SearchFiltered(Q, K, f, ef=40, mode=gpu.FILTER_WALK)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(c.get(ids)[0], np.arange(300))


def test_rejected_calls_change_nothing(gpu):
    from coltt_amd._lib import vp
    L = gpu.lib()
    gh, X, ids, lv = _small(gpu, remove=40)
    other, _, oids, _ = _small(gpu, n=100, seed=78)
    f = gh.Filter(ids[::2]); c = gh.AttrColumn(gpu.ATTR_I64); c.set(ids, np.arange(300))
    f_foreign = other.Filter(oids[::2]); c_foreign = other.AttrColumn(gpu.ATTR_I64)
    gh2, _, ids2, _ = _small(gpu, n=100, seed=79, remove=5)
    f_stale = gh2.Filter(ids2[::2]); c_stale = gh2.AttrColumn(gpu.ATTR_I64); gh2.Compact()
    f_stale_h, c_stale_h = f_stale.h.value, c_stale.h.value
    f_ids = f.ids()

    def call(fl, cl, nf=None, nc=None):
        fa = np.array(fl or [], np.uint64); ca = np.array(cl or [], np.uint64)
        return L.coltt_hnsw_compact_carry(gh.h, C.c_uint64(0), vp(fa) if fl is not None else None, C.c_size_t(len(fa) if nf is None else nf), None,
                                          vp(ca) if cl is not None else None, C.c_size_t(len(ca) if nc is None else nc), None, None, C.c_uint64(0), None, None)

    def unchanged():
        return gh.Len() == 260 and _slots(gh) == 300 and np.array_equal(f.ids(), f_ids) and c.get(ids[:1])[1].size == 1

    fh, ch = f.h.value, c.h.value
    cases = [
        (lambda: call([fh, 987654321], [ch]), NOT_FOUND, b"filters[1]"),
        (lambda: call([fh], [ch, 987654321]), NOT_FOUND, b"columns[1]"),
        (lambda: call([fh, f_foreign.h.value], [ch]), INVALID, b"filters[1]"),
        (lambda: call([fh], [c_foreign.h.value]), INVALID, b"columns[0]"),
        (lambda: call([ch], []), NOT_FOUND, b"filters[0]"),                       # a column where a filter belongs
        (lambda: call(None, [ch], nf=2), INVALID, b"filters"),
        (lambda: call([fh], None, nc=1), INVALID, b"columns"),
    ]
    for fn, code, word in cases:
        assert fn() == code and word in L.coltt_last_error(), (code, L.coltt_last_error())
        assert unchanged()
    # stale objects of their own index
    for fl, cl, word in (([f_stale_h], [], b"filters[0]"), ([], [c_stale_h], b"columns[0]")):
        fa = np.array(fl, np.uint64); ca = np.array(cl, np.uint64)
        rc = L.coltt_hnsw_compact_carry(gh2.h, C.c_uint64(0), vp(fa) if fl else None, C.c_size_t(len(fl)), None, vp(ca) if cl else None, C.c_size_t(len(cl)),
                                        None, None, C.c_uint64(0), None, None)
        assert rc == INVALID and word in L.coltt_last_error() and b"stale" in L.coltt_last_error()
        assert gh2.Len() == 95
    # a short map, as coltt_hnsw_compact refuses it: the objects stay valid
    m = np.zeros(299, np.uint32); fa = np.array([fh], np.uint64)
    rc = L.coltt_hnsw_compact_carry(gh.h, C.c_uint64(0), vp(fa), C.c_size_t(1), None, None, C.c_size_t(0), None, vp(m), C.c_uint64(299), None, None)
    assert rc == INVALID and b"map" in L.coltt_last_error() and unchanged()
    # and the accepted call still works afterwards
    st, cs, al, ns = gh.CompactCarry([f, f, f], [c, c])
    assert st["slots_after"] == 260 and cs["filters"] == 1 and cs["columns"] == 1 and list(al) == [len(f_ids)] * 3 and list(ns) == [260, 260]
    assert np.array_equal(f.ids(), f_ids) and cs["list_entries"] == len(f_ids) and cs["column_values"] > 0


def test_all_dead_gives_the_empty_index_and_valid_empty_objects(gpu):
    gh, X, ids, lv = _small(gpu, n=100)
    f = gh.Filter(ids[::2]); c = gh.AttrColumn(gpu.ATTR_I64); c.set(ids, np.arange(100))
    for i in ids:
        gh.Remove(int(i))
    st, cs, al, ns, nmap = gh.CompactCarry([f], [c], with_map=True)
    assert st["slots_after"] == 0 and (nmap == NONE).all() and al[0] == 0 and ns[0] == 0
    assert f.info()["allowed"] == 0 and f.info()["slots"] == 0 and c.info()["slots"] == 0 and c.info()["set"] == 0
    assert len(f.ids()) == 0
    assert (gh.SearchFiltered(X[:3], 5, f, ef=20)[2] == 0).all()
    for i in range(40):
        gh.Insert(int(ids[i]), X[i], int(lv[i]))
    assert gh.Len() == 40 and (gh.Search(X[:3], 5, ef=20)[2] == 5).all()
    assert (gh.SearchFiltered(X[:3], 5, f, ef=20)[2] == 0).all()                  # the carried filter covers none of them
    assert not c.get(ids[:40])[1].any()
    assert c.set(ids[:40], np.arange(40)) == 40 and np.array_equal(c.get(ids[:40])[0], np.arange(40))
    with gh.FilterEval([0, gpu.FOP_NOT], [f]) as nf:
        assert nf.allowed == 40


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. concurrency
def test_readers_and_filter_info_during_the_call(gpu):
    """readers search with F1 and evaluate a predicate over C1 while the main thread calls CompactCarry once: every answer equals the recorded one
    (ids are invariant); a thread looping on filter_info sees the pair (allowed, slots) of before or of after, never a mix."""
    s = _shared("a-701x48-f32-l2-ids")
    gh, _ = _build(gpu, s)
    ids, n = s["ids"], s["n"]
    f1 = gh.Filter(ids[::2]); c1 = gh.AttrColumn(gpu.ATTR_I64); c1.set(ids, np.arange(n))
    for v in s["victims"]:
        gh.Remove(int(ids[v]))
    Q = s["Q"]
    want = gh.SearchFiltered(Q[:8], K, f1, ef=40, mode=gpu.FILTER_WALK)
    with gh.FilterEvalAttr([0], [], [(c1, gpu.CMP_LT, n // 2)]) as p:
        want_pred = p.ids()
    pair_before = (f1.info()["allowed"], f1.info()["slots"])
    live = ~s["dead"]
    pair_after = (int(live[::2].sum()), int(live.sum()))
    assert pair_before[0] != pair_after[0] and pair_before[1] != pair_after[1]
    stop = threading.Event(); bad = []; rounds = [0] * 4; pairs = set(); raced = []

    def reader(t):
        try:
            while not stop.is_set():
                if t == 3:
                    i = f1.info(); pairs.add((i["allowed"], i["slots"]))
                elif t == 2:
                    with gh.FilterEvalAttr([0], [], [(c1, gpu.CMP_LT, n // 2)]) as q:
                        if q.allowed != len(want_pred):
                            bad.append((t, rounds[t], "allowed"))
                        try:
                            if not np.array_equal(q.ids(), want_pred):
                                bad.append((t, rounds[t], "ids"))
                        except gpu.ColttError as e:
                            # q is this thread's own, unlisted filter: the one call may fall between its evaluation and its read-back
                            if e.code != INVALID or b"stale" not in gpu.lib().coltt_last_error():
                                raise
                            raced.append(rounds[t])
                else:
                    gi, gs, gc = gh.SearchFiltered(Q[:8], K, f1, ef=40, mode=gpu.FILTER_WALK)
                    if not (np.array_equal(gc, want[2]) and np.array_equal(gi, want[0]) and np.array_equal(bits(gs), bits(want[1]))):
                        bad.append((t, rounds[t]))
                rounds[t] += 1
        except Exception as e:   # noqa: BLE001
            bad.append((t, repr(e)))

    th = [threading.Thread(target=reader, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    try:
        while min(rounds) < 5 and not bad:
            stop.wait(0.001)
        st = gh.CompactCarry([f1], [c1], stage_bytes=1)[0]
        seen = list(rounds)
        while min(r - r0 for r, r0 in zip(rounds, seen)) < 5 and not bad:
            stop.wait(0.001)
    finally:
        stop.set()
        for t in th:
            t.join()
    assert st["slots_after"] == gh.Len() and not bad, bad[:4]
    assert pairs == {pair_before, pair_after}, pairs
    assert len(raced) <= 1, raced
