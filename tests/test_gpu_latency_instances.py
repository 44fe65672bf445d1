"""Every instance of the 256-thread latency kernel a search can launch (hnsw_search_lat_kernel<METRIC, QUANT, TP, SEQ>, coltt_amd/csrc/hnsw_lat.hpp;
launch_search_lat in hnsw.hip) against the oracle's canonical Hnsw.Search over the very arrays copied out of HBM: ids, ranks, f32 score bits of every query
of every call, and the traversal counters.  No tolerance.

The table is tests/latency_cases.py (test_latency_cases_host.py holds it against the plan function without a device).  Each case's index is built in
batches, loses ~12 % of its rows to Remove — the entrypoint among them, so one is re-elected — and gains 40 single Inserts: the walks run over rows that
still list tombstones.  Before every search the plan must be the launch under test (family, walk, row layout, helpers, and the TP that follows from the
index's facts); after it the launch counters must be the latency kernel's: a case that quietly ran another kernel fails."""
import time

import numpy as np
import pytest

import latency_cases as LC
from oracle import oracle as O
from util import assert_same_results, bits

pytestmark = pytest.mark.gpu

_INDEXES = {}


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in LC.KNOBS:
        monkeypatch.delenv(k, raising=False)


def _gpu_build(gpu, X, lv, metric, quant, cfg, batch):
    import torch
    n, d = X.shape
    gh = gpu.Hnsw(d, metric, cfg, quantization=quant)
    xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
    i = 0
    while i < n:
        b = int(min(n - i, max(1, min(batch, i // 16))))
        gh.InsertBatchDevice(xd.data_ptr() + i * d * 4, b, lv[i:i + b], batch=b, first_id=i)
        i += b
    return gh


def _index(gpu, c, monkeypatch):
    """the case's index after build, Removes and single Inserts; its arrays as the oracle reads them; its queries; the oracle's answers as they are asked for"""
    key = LC.index_key(c)
    if key in _INDEXES:
        return _INDEXES[key]
    t0 = time.time()
    n1, n2 = LC.sizes(c)
    d = c.dim
    seed = 41000 + 16 * [LC.index_key(x) for x in LC.CASES + [LC.CASE_801]].index(key)   # the same data whichever tests run, in whatever order
    X = O.fill_normal(seed, (n1 + n2, d))
    if c.group == "D":   # NaN distances (a zero vector has no direction) and exact ties (every distance to rows 0-999 appears twice)
        X[7] = 0.0; X[100] = 0.0
        X[1000:2000] = X[0:1000]
    lv = O.levels(seed + 1, n1 + n2, c.m)
    if c.rows8 is not None:
        monkeypatch.setenv("COLTT_ROWS8", c.rows8)
    gh = _gpu_build(gpu, X[:n1], lv[:n1], c.metric, c.quant, gpu.HnswCfg.default(m=c.m, ef_construction=40 if d > 800 else 48), batch=256)
    monkeypatch.delenv("COLTT_ROWS8", raising=False)
    assert gh.cfg.m_max0 == 2 * c.m
    # ~12 % Removes, the entrypoint among them (ids are slots: first_id = the slot)
    entry0 = int(gh.ExportRaw()["entry"])
    rng = np.random.default_rng(seed + 2)
    keep = {7, 100} if c.group == "D" else set()
    victims = [int(v) for v in rng.choice(n1, int(0.12 * n1), replace=False) if int(v) not in keep and int(v) != entry0]
    victims.insert(len(victims) // 2, entry0)
    for v in victims:
        gh.Remove(v)
    for j in range(n2):
        gh.Insert(n1 + j, X[n1 + j], int(lv[n1 + j]))
    # ---- the oracle's side: the arrays as they lie in HBM
    g = gh.ExportRaw(); rows = gh.FetchRows(); ex = gh.Export()
    n = int(g["n"])
    assert n == n1 + n2 and np.array_equal(ex["ids"], np.arange(n, dtype=np.uint64))
    dead = ex["deleted"].astype(bool)
    assert dead.sum() == len(victims) and dead[victims].all()
    adj0 = g["adj0"]
    named = adj0[~dead]                                    # rows of live vertices
    listed = int(dead[named[named != gpu.hnsw.L.NBR_NONE]].sum())
    assert listed >= 50, f"{c.name}: only {listed} level-0 adjacency entries name a tombstone"
    assert dead[entry0] and int(g["entry"]) != entry0 and not dead[int(g["entry"])], "the first entrypoint must be tombstoned and another one elected"
    del_bits = np.zeros((n + 31) // 32, np.uint32)
    for s in np.nonzero(dead)[0]:
        del_bits[s >> 5] |= np.uint32(1 << (int(s) & 31))
    Q = O.fill_normal(seed + 3, (LC.SECOND_QUERY_NQ, d))
    ix = {"gh": gh, "g": g, "rows": rows, "del_bits": del_bits, "Q": Q, "listed": listed, "removed": len(victims), "oracle": {}, "n": n,
          "build_s": time.time() - t0}
    _INDEXES[key] = ix
    return ix


def _oracle(ix, c, nq, k, ef):
    """(slots, scores, counts, counters) of the first nq queries — computed once per (index, call), shared by the cases and tests over that index"""
    ef = max(ef, k)                           # Hnsw.Search walks with max(ef, k) (hnsw.go:258); csr_search takes the walk's ef
    key = (nq, k, ef)
    if key not in ix["oracle"]:
        g = ix["g"]
        sl, sc, cn, ost, _ = O.csr_search(ix["rows"], c.quant, g["adj0"], g["upper_off"], g["adjU"], c.dim, c.metric, g["entry"], g["entry_level"],
                                          ix["Q"][:nq], k, ef, del_bits=ix["del_bits"], threads=4)
        for a in (sl, sc, cn):
            a.setflags(write=False)
        ix["oracle"][key] = (sl, sc, cn, ost)
    return ix["oracle"][key]


def _expect_latency_plan(gpu, ix, c, nq, k, ef, helpers=0):
    """the launch Search(Q[:nq], k, ef) is about to make is the instance under test"""
    gh = ix["gh"]
    p = gh.SearchPlan(nq, k, ef)
    tag = f"{c.name} nq{nq} k{k} ef{ef}"
    assert p["family"] == gpu.hnsw.PLAN_LATENCY, (tag, p)
    assert (p["lat_seq"], p["r8"], p["rows8_launch"], p["lat_helpers"]) == (LC.lat_seq(c), LC.r8(c), LC.r8(c), helpers), (tag, p)
    f = gh.PlanFacts()
    assert (f.dim, f.quant, f.metric, f.m_max0, f.stride, f.slots, f.r8) == (c.dim, c.quant, c.metric, 2 * c.m, LC.stride(c), ix["n"], LC.r8(c)), tag
    assert LC.tp_of(f.r8, f.stride, p["lat_seq"]) == LC.tp(c), (tag, f.r8, f.stride)
    return p


def _search_equals_oracle(gpu, ix, c, nq, k, ef, latency=True, helpers=0):
    """one call: plan, search, launch counters, every query's ids / ranks / score bits, the summed traversal counters.  Returns what the GPU answered."""
    gh = ix["gh"]
    tag = f"{c.name} nq{nq} k{k} ef{ef} helpers{helpers}"
    if latency:
        _expect_latency_plan(gpu, ix, c, nq, k, ef, helpers)
    else:
        assert gh.SearchPlan(nq, k, ef)["family"] != gpu.hnsw.PLAN_LATENCY, tag
    r8_before = gh.Rows8()[0]
    gi, gs, gc, st = gh.Search(ix["Q"][:nq], k, ef=ef, with_stats=True)
    if latency:
        v = gh.VisitedStats()
        assert (v["kind"], v["waves_per_cu"], v["grid"]) == (32, 1, min(nq, 256)), (tag, v)
        assert gh.Rows8()[0] - r8_before == LC.r8(c), tag
    sl, sc, cn, ost = _oracle(ix, c, nq, k, ef)
    assert st["n_visit_resets"] == 0, (tag, st)
    for qi in range(nq):
        assert_same_results(gi[qi, :gc[qi]], gs[qi, :gc[qi]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], f"{tag} q{qi}")
    assert {k_: st[k_] for k_ in ost} == ost, (tag, st, ost)
    return gi, gs, gc, st


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c.name)
def test_instance_equals_oracle(gpu, monkeypatch, c):
    """nq 1, 7, 40 at ef 1, 2, 3 (the speculatively popped candidate is truncated away), 20, 64, 128, k > ef, and ef 200 where the plan still says latency"""
    ix = _index(gpu, c, monkeypatch)
    _set(monkeypatch, LC.search_knobs(c))
    t0 = time.time()
    calls = 0
    for nq in LC.NQS:
        for k, ef in LC.SEARCHES:
            if (k, ef) == (10, 200) and not c.ef200:
                _search_equals_oracle(gpu, ix, c, nq, k, ef, latency=False)   # the plan leaves the kernel there: still the oracle's answers
                continue
            _search_equals_oracle(gpu, ix, c, nq, k, ef)
            calls += 1
    if c.group == "D":
        k = LC.TIES_K
        for nq in (7, 40):
            _search_equals_oracle(gpu, ix, c, nq, k, k)
            calls += 1
        sl, sc, cn, _ = _oracle(ix, c, 40, k, k)
        pairs = [int((bits(sc[qi, :cn[qi]])[1:] == bits(sc[qi, :cn[qi]])[:-1]).sum()) for qi in range(40)]
        assert max(pairs) >= 20, f"the oracle's top-{k} hold at most {max(pairs)} adjacent pairs of equal score bits: the case decides no tie"
        print(f"[latency-instances] {c.name}: adjacent equal-score pairs in the top-{k}, most per query {max(pairs)}, queries with >= 20: {sum(p >= 20 for p in pairs)}")
    print(f"[latency-instances] {c.name}: instance {LC.instance(c)} latency calls {calls} rows {ix['n']} removed {ix['removed']} "
          f"tombstoned entries listed {ix['listed']} build {ix['build_s']:.2f}s searches {time.time() - t0:.2f}s")


@pytest.mark.parametrize("name", LC.EDGE_CASES)
def test_capacity_edge(gpu, monkeypatch, name):
    """the largest ef the hash-capacity rule lets into the kernel, found from the plan itself, and one more, which another family serves"""
    c = LC.BY_NAME[name]
    ix = _index(gpu, c, monkeypatch)
    _set(monkeypatch, LC.search_knobs(c))
    gh = ix["gh"]
    gh.Search(ix["Q"][:1], 10, ef=200)           # makes the HBM visited workspace: from here on the facts hold still
    assert gh.PlanFacts().vis_ready
    e = LC.largest_latency_ef(gh.SearchPlan)
    assert e is not None and e > 128, (name, e)
    p = gh.SearchPlan(1, 10, e)
    assert (p["hcap"] // 4) * 3 >= e * 34 + 64 > (p["hcap"] // 4) * 3 - 34, (name, e, p)   # it is the capacity rule that ends there, not the LDS limit
    for nq in (1, 7):
        _search_equals_oracle(gpu, ix, c, nq, 10, e)
        _search_equals_oracle(gpu, ix, c, nq, 10, e + 1, latency=False)
    print(f"[latency-instances] {name}: capacity-edge ef {e} (hash table of {p['hcap']} entries)")


@pytest.mark.parametrize("name", LC.SECOND_QUERY_CASES)
def test_a_workgroups_second_query(gpu, monkeypatch, name):
    """300 queries on a grid of 256: at least 44 workgroups claim a second query and re-initialise the visited table, the result set, the delta, the counters
    and the exchange words for it"""
    c = LC.BY_NAME[name]
    ix = _index(gpu, c, monkeypatch)
    _set(monkeypatch, LC.search_knobs(c))
    nq = LC.SECOND_QUERY_NQ
    assert ix["gh"].SearchPlan(nq, 10, 64)["family"] != gpu.hnsw.PLAN_LATENCY
    monkeypatch.setenv("COLTT_LAT_MAX_NQ", "512")
    assert ix["gh"].SearchPlan(nq, 10, 64)["grid"] == 256
    for k, ef in ((10, 64), (1, 2)):
        _search_equals_oracle(gpu, ix, c, nq, k, ef)
    print(f"[latency-instances] {name}: {nq} queries on 256 workgroups, >= {nq - 256} second queries")


@pytest.mark.parametrize("name", LC.HELPER_CASES)
def test_helper_workgroups_change_nothing(gpu, monkeypatch, name):
    """COLTT_LAT_HELPERS 1 .. 3: lat_helper_loop, the hints posted from wave 0's mid hook and the mailbox launch — answers, score bits and counters are the
    oracle's and those of the same call without helpers.  nq 9 > LAT_MASTERS launches no helper; the plan field is set all the same."""
    c = LC.BY_NAME[name]
    ix = _index(gpu, c, monkeypatch)
    _set(monkeypatch, LC.search_knobs(c))
    plain = {(nq, ef): _search_equals_oracle(gpu, ix, c, nq, 10, ef) for nq in LC.HELPER_NQS for ef in LC.HELPER_EFS}
    for helpers in (1, 2, 3):
        monkeypatch.setenv("COLTT_LAT_HELPERS", str(helpers))
        for (nq, ef), (pi, ps, pc, pst) in plain.items():
            gi, gs, gc, st = _search_equals_oracle(gpu, ix, c, nq, 10, ef, helpers=helpers)
            assert np.array_equal(gi, pi) and np.array_equal(bits(gs), bits(ps)) and np.array_equal(gc, pc) and st == pst, (name, helpers, nq, ef)


def test_the_sequential_walk_takes_no_helpers(gpu, monkeypatch):
    c = LC.BY_NAME[LC.HELPER_SEQ_CASE]
    ix = _index(gpu, c, monkeypatch)
    _set(monkeypatch, LC.search_knobs(c))
    monkeypatch.setenv("COLTT_LAT_HELPERS", "3")
    for nq in (1, 8):
        _search_equals_oracle(gpu, ix, c, nq, 10, 64, helpers=0)   # _expect_latency_plan: lat_seq 1, lat_helpers 0


def test_801_elements_leave_the_kernel(gpu, monkeypatch):
    """beside c-f32-799-cos (stride 3 200 = LAT_MAX_STRIDE): 801-d f32 rows (3 216 bytes) must not plan the latency kernel; their answers are the oracle's too"""
    c = LC.CASE_801
    ix = _index(gpu, c, monkeypatch)
    assert ix["gh"].PlanFacts().stride == 3216
    for nq in LC.NQS:
        for k, ef in LC.SEARCHES:
            _search_equals_oracle(gpu, ix, c, nq, k, ef, latency=False)
