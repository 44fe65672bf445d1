"""Filtered search over the product-quantised walk with a filter per query (coltt_hnsw_pq_search_filtered_batch; include/coltt_gpu.h): row i
of a batch call equals coltt_hnsw_pq_search_filtered on query i alone — ids, exact score bits, count, path — and the batch's counters are
the sums of the single calls'.  Over every kernel form of the (LS, NP, NBR) dispatch and rows of 64, the WALK / EXACT / AUTO modes, both
visited sets, batches that need both walk launches and the exact scan at once, differing per-query geometries inside one launch, forced
variants, the CPU restatement (tests/filtered_pq_ref.py), edge cases, all-or-nothing validation, concurrency with inserts, a C++ consumer
of the batcher, and the neighbouring entry points before and after."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import filtered_ref as F
import filtered_pq_ref as P

pytestmark = pytest.mark.gpu

K = P.K
ALL = [(c, P.N, P.GRAPH) for c in P.CASES] + [(P.WIDE, P.N_WIDE, P.GRAPH_WIDE)]
COUNTERS = ("n_dist", "n_exp", "n_hops", "n_visit_resets", "n_exact_rows")
FRACS = (1.0, 0.5, 0.1, 0.01)


def _consts(gpu, case):
    metric, quant = case[0], case[1]
    return (gpu.COSINE if metric == "cos" else gpu.EUCLIDEAN, gpu.Q_NONE if quant == "f32" else gpu.Q_F16,
            O.COSINE if metric == "cos" else O.L2, O.Q_NONE if quant == "f32" else O.Q_F16)


def _make(gpu, case, n, graph, X=None, lv=None, ids=None, batch=64):
    """an index whose graph is built on the GPU, with a quantiser trained on its stored rows attached; returns (index, codebooks)"""
    import torch
    M, Qn, om, oq = _consts(gpu, case)
    d, m, c, pqm = case[2], case[3], case[4], case[5]
    if X is None:
        X, lv, _ = P.case_data(case, n)
    h = gpu.Hnsw(d, M, gpu.HnswCfg.default(**graph), quantization=Qn)
    xd = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0"); torch.cuda.synchronize()
    h.InsertBatchDevice(xd.data_ptr(), n, lv, batch=batch, ids=ids)
    seen = F.decode(oq, h.FetchRows())
    pq = gpu.PQSpace(d, pqm, m, c)
    pq.Fit(seen[: max(c, min(n, 2000))], iterations=4)
    h.PqAttach(pq)
    return h, pq.Codebooks()


_CACHE = {}


def _index(gpu, case, n, graph):
    """one index per case, shared by the tests that do not change it"""
    if case not in _CACHE:
        h, cb = _make(gpu, case, n, graph)
        _CACHE[case] = (h, cb, P.case_data(case, n)[2])
    return _CACHE[case]


def _queries(case, nq, seed=0):
    return O.fill_normal(P.case_seed(case[2], case[3]) + 70 + seed, (nq, case[2]))


def _singles(h, Q, k, flts, ef, rerank, mode):
    """the reference answer: one single-filter call per query"""
    nq = len(Q)
    ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32); paths = np.zeros(nq, np.int32)
    tot = {c: 0 for c in COUNTERS}
    ef_walk = 0
    for i in range(nq):
        gi, gs, gc, st = h.PqSearchFiltered(Q[i:i + 1], k, flts[i], ef=ef, rerank=rerank, mode=mode, with_stats=True)
        ids[i], sc[i], cnt[i], paths[i] = gi[0], gs[0], gc[0], st["path"]
        for c in COUNTERS:
            tot[c] += st[c]
        ef_walk = max(ef_walk, st["ef_walk"])
    return ids, sc, cnt, paths, tot, ef_walk


def _assert_equal_rows(got, want, msg):
    gi, gs, gc, gp = got[:4]
    wi, ws, wc, wp = want[:4]
    assert np.array_equal(gc, wc), (msg, gc, wc)
    assert np.array_equal(gp, wp), (msg, gp, wp)
    for i in range(len(gc)):
        c = int(gc[i])
        assert np.array_equal(gi[i, :c], wi[i, :c]), (msg, i, gi[i, :c], wi[i, :c])
        assert np.array_equal(bits(gs[i, :c]), bits(ws[i, :c])), (msg, i)


def _check_batch(gpu, h, Q, k, flts, ef, rerank, mode, msg=""):
    bi, bs, bc, bp, st = h.PqSearchFilteredBatch(Q, k, flts, ef=ef, rerank=rerank, mode=mode, with_stats=True)
    want = _singles(h, Q, k, flts, ef, rerank, mode)
    _assert_equal_rows((bi, bs, bc, bp), want, msg)
    assert {c: st[c] for c in COUNTERS} == want[4], (msg, st, want[4])
    assert st["n_visit_resets"] == 0, (msg, st)
    assert st["ef_walk"] == want[5], (msg, st, want[5])
    kinds = set(int(p) for p in want[3])
    assert st["path"] == (kinds.pop() if len(kinds) == 1 else gpu.FILTER_AUTO), (msg, st, want[3])
    return bi, bs, bc, bp, st


@pytest.mark.parametrize("case,n,graph", ALL)
def test_batch_equals_single_calls(gpu, monkeypatch, case, n, graph):
    h, cb, _ = _index(gpu, case, n, graph)
    flts = [h.Filter(np.nonzero(P.allow_mask(case, n, frac) if frac < 1.0 else np.ones(n, bool))[0]) for frac in FRACS]
    try:
        Q = _queries(case, 11)
        per_row = [flts[(i * 3) % 4] for i in range(len(Q))]
        # ef 48: LDS hash | ef 300: byte map with the neighbourhood blocks, and the same walk gathering code rows by neighbour slot
        for ef, nbr in ((48, None), (300, None), (300, "0")):
            if nbr is not None:
                monkeypatch.setenv("COLTT_PQ_NBR", nbr)
            try:
                for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
                    for rerank in P.WALK_RERANKS:
                        _check_batch(gpu, h, Q, K, per_row, ef, rerank, mode, (mode, ef, nbr, rerank))
            finally:
                if nbr is not None:
                    monkeypatch.delenv("COLTT_PQ_NBR")
    finally:
        for f in flts:
            f.close()


def test_batch_equals_the_restatement(gpu):
    """row by row against tests/filtered_pq_ref.py: the test does not only compare the library with itself"""
    case, n, graph = ALL[1]
    h, cb, _ = _index(gpu, case, n, graph)
    _, _, om, oq = _consts(gpu, case)
    g = h.ExportRaw(); rows = F.decode(oq, h.FetchRows()); codes = h.PqCodes(); ids = h.Export()["ids"]
    allows = [P.allow_mask(case, n, frac) for frac in (0.5, 0.1)]
    flts = [h.Filter(np.nonzero(a)[0]) for a in allows]
    try:
        Q = _queries(case, 6, 1)
        pick = [i % 2 for i in range(len(Q))]
        for ef, rerank in ((48, 0), (300, 12)):
            gi, gs, gc, gp, st = h.PqSearchFilteredBatch(Q, K, [flts[p] for p in pick], ef=ef, rerank=rerank, mode=gpu.FILTER_WALK, with_stats=True)
            tot = {"n_dist": 0, "n_exp": 0, "n_hops": 0}; nr = 0
            for qi in range(len(Q)):
                s, v, r, t = P.search(rows, g, om, oq, cb, case[5], codes, Q[qi], K, ef, rerank, allows[pick[qi]])
                c = int(gc[qi])
                assert gp[qi] == gpu.FILTER_WALK and c == len(s) == min(K, r), (ef, rerank, qi, c, len(s), r)
                assert np.array_equal(gi[qi, :c], ids[s]), (ef, rerank, qi)
                assert np.array_equal(bits(gs[qi, :c]), bits(v)), (ef, rerank, qi)
                nr += r
                for kk in tot:
                    tot[kk] += t[kk]
            assert {kk: st[kk] for kk in tot} == tot and st["n_exact_rows"] == nr, (ef, rerank, st, tot, nr)
    finally:
        for f in flts:
            f.close()


MIXED = ("l2", "f32", 64, 16, 32, O.PQ_EUCLIDEAN)


def _big(gpu, n, ef, seed):
    key = ("big", n, ef)
    if key not in _CACHE:
        X = O.fill_normal(seed, (n, 64)); lv = O.levels(seed + 1, n)
        h, cb = _make(gpu, MIXED, n, dict(m=8, ef=ef, ef_construction=40), X=X, lv=lv, batch=512)
        _CACHE[key] = (h, cb)
    return _CACHE[key][0]


def test_one_batch_takes_both_walks_and_the_exact_scan(gpu, monkeypatch):
    """20 000 vertices, cfg ef 64; filters at 100 %, 40 %, 10 % interleaved: AUTO walks at 64 (LDS hash) and 160 (byte map) and sends the
    10 % rows to the exact scan — all in one call"""
    n = 20_000
    want_paths = [F.auto_path(a, n, 64) for a in (n, n * 4 // 10, n // 10)]
    assert want_paths[0] == (F.WALK, 64) and want_paths[1] == (F.WALK, 160) and want_paths[2][0] == F.EXACT, want_paths
    h = _big(gpu, n, 64, 901)
    rng = np.random.default_rng(903)
    flts = [h.Filter(rng.permutation(n)[:m]) for m in (n, n * 4 // 10, n // 10)]
    try:
        Q = O.fill_normal(904, (30, 64))
        per_row = [flts[i % 3] for i in range(len(Q))]
        for rerank in (0, 12):
            bi, bs, bc, bp, st = _check_batch(gpu, h, Q, K, per_row, 0, rerank, gpu.FILTER_AUTO, ("mixed", rerank))
            assert st["path"] == gpu.FILTER_AUTO and st["ef_walk"] == 160
            assert [int(p) for p in bp[:3]] == [F.WALK, F.WALK, F.EXACT]
            assert (bc == K).all()
        # an LDS-hash walk near the capacity of its hash (ef 170: 8 192 words): a query that fills it runs again over the byte map, in the
        # batch as in the single call; the rows are equal whether or not any does
        monkeypatch.setenv("COLTT_VISG", "0")
        try:
            _check_batch(gpu, h, Q, K, per_row, 170, 0, gpu.FILTER_WALK, "ef 170 over the LDS hash")
        finally:
            monkeypatch.delenv("COLTT_VISG")
    finally:
        for f in flts:
            f.close()


def test_differing_geometries_in_one_launch(gpu, monkeypatch):
    """cfg ef 32, ef_override 0, AUTO: filters at 100 %, 50 % and 25 % of 17 000 vertices walk at 32, 64 and 128 — three result-set sizes,
    capacities of R and LDS layouts inside ONE launch; over the LDS hash (the default at these breadths) and, with the byte map forced,
    inside the byte-map launch (with the neighbourhood blocks and gathering)"""
    n = 17_000
    want = [F.auto_path(a, n, 32) for a in (n, n // 2, n // 4)]
    assert want == [(F.WALK, 32), (F.WALK, 64), (F.WALK, 128)], want
    h = _big(gpu, n, 32, 911)
    rng = np.random.default_rng(913)
    flts = [h.Filter(rng.permutation(n)[:m]) for m in (n, n // 2, n // 4)]
    try:
        Q = O.fill_normal(914, (13, 64))
        per_row = [flts[(i * 2) % 3] for i in range(len(Q))]
        for visg, nbr in ((None, None), ("1", None), ("1", "0")):
            for name, val in (("COLTT_VISG", visg), ("COLTT_PQ_NBR", nbr)):
                if val is not None:
                    monkeypatch.setenv(name, val)
            try:
                for rerank in (0, 40):           # 40: R's capacity is min(40, ef_walk) = 32, 40, 40
                    bi, bs, bc, bp, st = _check_batch(gpu, h, Q, K, per_row, 0, rerank, gpu.FILTER_AUTO, (visg, nbr, rerank))
                    assert (bp == F.WALK).all() and st["ef_walk"] == 128 and st["path"] == gpu.FILTER_WALK
            finally:
                for name, val in (("COLTT_VISG", visg), ("COLTT_PQ_NBR", nbr)):
                    if val is not None:
                        monkeypatch.delenv(name)
        # both launches at once with differing breadths in each: ef_override 100 -> 100 (LDS hash), 200 and 400 (byte map)
        want = [F.auto_path(a, n, 100) for a in (n, n // 2, n // 4)]
        assert want[0] == (F.WALK, 100) and want[1] == (F.WALK, 200), want
        _check_batch(gpu, h, Q, K, per_row, 100, 12, gpu.FILTER_AUTO, "ef 100")
    finally:
        for f in flts:
            f.close()


@pytest.mark.parametrize("visg,ef", [("0", 300), ("1", 48)])
def test_forced_variants(gpu, monkeypatch, visg, ef):
    case, n, graph = ALL[1]
    h, cb, _ = _index(gpu, case, n, graph)
    flts = [h.Filter(np.nonzero(P.allow_mask(case, n, frac))[0]) for frac in (0.5, 0.1)]
    monkeypatch.setenv("COLTT_VISG", visg)
    try:
        Q = _queries(case, 7, 2)
        _check_batch(gpu, h, Q, K, [flts[i % 2] for i in range(len(Q))], ef, 12, gpu.FILTER_WALK, (visg, ef))
    finally:
        monkeypatch.delenv("COLTT_VISG")
        for f in flts:
            f.close()


def test_edge_cases(gpu):
    import torch
    case, n, graph = P.CASES[0], P.N, P.GRAPH
    d = case[2]
    X, lv, _ = P.case_data(case, n)
    idv = np.arange(n, dtype=np.uint64) * 7 + 1000          # caller ids (the shared indexes have dense ones)
    h, cb = _make(gpu, case, n, graph, X=X, lv=lv, ids=idv)
    Q = _queries(case, 8, 3)
    a_slots = np.arange(0, n, 3)
    fa = h.Filter(idv[a_slots])
    fb = h.Filter(idv[np.arange(1, n, 50)])
    few = h.Filter(idv[[4, 8, 15]])                          # k larger than |R|
    empty = h.Filter([10 ** 12])                             # an empty filter among served rows
    assert empty.allowed == 0 and few.allowed == 3
    per_row = [fa, empty, fb, fa, few, empty, fb, fa]        # repeated handles
    for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
        for ef in (48, 300):
            bi, bs, bc, bp, st = _check_batch(gpu, h, Q, K, per_row, ef, 0, mode, (mode, ef))
            assert bc[1] == 0 and bc[5] == 0 and bc[4] <= 3
            assert (bc[[0, 2, 3, 6, 7]] > 0).all()             # the served rows are intact (their equality with the single calls: above)
            assert bc[4] == 3 or mode == gpu.FILTER_WALK     # (a walk holds only the allowed vertices it meets)
    # nq = 0 and nq = 1
    bi, bs, bc, bp, st = h.PqSearchFilteredBatch(np.zeros((0, d), np.float32), K, [], with_stats=True)
    assert bc.shape == (0,) and st["path"] == 0 and st["n_dist"] == 0
    for ef in (48, 300):
        _check_batch(gpu, h, Q[:1], K, [fb], ef, 12, gpu.FILTER_WALK, ("nq=1", ef))
    # tombstones after the filter was built: never returned; vertices inserted after it: not allowed
    gone = a_slots[:40]
    for s in gone:
        h.Remove(int(idv[s]))
    X2 = np.concatenate([Q, O.fill_normal(7999, (64 - len(Q), d))]); lv2 = O.levels(8000, 64)   # copies of the queries: they would be the nearest
    x2 = torch.from_numpy(np.ascontiguousarray(X2)).to("cuda:0"); torch.cuda.synchronize()
    h.InsertBatchDevice(x2.data_ptr(), 64, lv2, batch=16, ids=np.arange(64, dtype=np.uint64) + 10 ** 9)
    ok = set(int(x) for x in idv[a_slots[40:]])
    for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
        for ef in (48, 300):
            bi, bs, bc, bp = _check_batch(gpu, h, Q, K, [fa] * 8, ef, 0, mode, ("removed + inserted", mode, ef))[:4]
            for qi in range(8):
                assert bc[qi] > 0 and set(int(x) for x in bi[qi, :bc[qi]]) <= ok, (mode, ef, qi)
    # an empty index that carries a quantiser: every count 0
    e_idx = gpu.Hnsw(d, gpu.EUCLIDEAN)
    pq = gpu.PQSpace(d, case[5], case[3], case[4]); pq.SetCodebooks(cb)
    e_idx.PqAttach(pq)
    with e_idx.Filter([1, 2]) as f0:
        for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
            _, _, bc, _ = e_idx.PqSearchFilteredBatch(Q[:3], K, [f0] * 3, mode=mode)
            assert (bc == 0).all()
    for f in (fa, fb, few, empty):
        f.close()


SENT_ID, SENT_SC, SENT_CNT, SENT_PATH = 0xABCDABCDABCDABCD, -7.25, 0xABCDABCD, -77


def _raw_batch(gpu, h, handles, Q, k=K, ef=0, rerank=0, mode=0, null_filters=False):
    """the call at the C ABI over output buffers pre-filled with a sentinel; returns (rc, last_error, whether every buffer is untouched)"""
    L = gpu.lib()
    nq = len(Q)
    fh = np.array(handles, np.uint64)
    q = np.ascontiguousarray(Q, np.float32)
    kk = max(k, 1)
    ids = np.full((nq, kk), SENT_ID, np.uint64); sc = np.full((nq, kk), SENT_SC, np.float32); cnt = np.full(nq, SENT_CNT, np.uint32)
    paths = np.full(nq, SENT_PATH, np.int32)
    rc = L.coltt_hnsw_pq_search_filtered_batch(h.h, None if null_filters else fh.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                               C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_uint32(rerank), C.c_int(mode),
                                               ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p),
                                               paths.ctypes.data_as(C.c_void_p), None)
    untouched = bool((ids == SENT_ID).all() and (sc == np.float32(SENT_SC)).all() and (cnt == SENT_CNT).all() and (paths == SENT_PATH).all())
    return rc, L.coltt_last_error().decode(), untouched


def test_validation_is_all_or_nothing(gpu):
    import torch
    case, n, graph = P.CASES[0], 600, P.GRAPH
    d = case[2]
    X, lv, _ = P.case_data(case, n)
    h, cb = _make(gpu, case, n, graph, X=X, lv=lv)
    other, _ = _make(gpu, case, 300, graph, X=X[:300], lv=lv[:300])
    bare = gpu.Hnsw(d, gpu.EUCLIDEAN, gpu.HnswCfg.default(**graph))
    xd = torch.from_numpy(X).to("cuda:0"); torch.cuda.synchronize()
    bare.InsertBatchDevice(xd.data_ptr(), n, lv, batch=64)
    Q = _queries(case, 5, 4)
    good = h.Filter(np.arange(0, n, 2))
    g = good.h.value
    dead = h.Filter([1, 2, 3]); dead_h = dead.h.value; dead.close()
    foreign = other.Filter([1, 2, 3])
    cases = [("null", None, -1, "NULL filters"),
             ("unknown", 0xDEADBEEF, -3, "position 3"),
             ("destroyed", dead_h, -3, "position 3"),
             ("foreign", foreign.h.value, -1, "position 3")]
    for name, bad, code, text in cases:
        if name == "null":
            rc, msg, clean = _raw_batch(gpu, h, [g] * 5, Q, null_filters=True)
        else:
            rc, msg, clean = _raw_batch(gpu, h, [g, g, g, bad, g], Q)
        assert rc == code and text in msg and clean, (name, rc, msg, clean)
    # no codes attached: checked first, for every mode and before the filters are looked at
    with bare.Filter(np.arange(100)) as bf:
        for mode in (gpu.FILTER_AUTO, gpu.FILTER_WALK, gpu.FILTER_EXACT):
            for handles in ([bf.h.value] * 5, [g, g, g, 0xDEADBEEF, g]):
                rc, msg, clean = _raw_batch(gpu, bare, handles, Q, mode=mode)
                assert rc == -1 and "no product-quantiser codes" in msg and clean, (mode, rc, msg, clean)
    rc, msg, clean = _raw_batch(gpu, h, [g] * 5, Q, mode=7)
    assert rc == -1 and "mode" in msg and clean, (rc, msg)
    rc, msg, clean = _raw_batch(gpu, h, [g] * 5, Q, k=0)
    assert rc == -1 and "k must be" in msg and clean, (rc, msg)
    rc, msg, clean = _raw_batch(gpu, h, [g] * 5, Q, ef=5000)
    assert rc == -4 and clean, (rc, msg)
    # the index still answers, and the same as the single calls
    _check_batch(gpu, h, Q, K, [good] * 5, 48, 0, gpu.FILTER_AUTO, "after errors")
    # stale: built before a Load
    h.Load(other.Commit())
    with h.Filter([1, 2, 3, 4]) as fresh:
        rc, msg, clean = _raw_batch(gpu, h, [fresh.h.value, fresh.h.value, fresh.h.value, g], Q[:4])
        assert rc == -1 and "position 3" in msg and "stale" in msg and clean, (rc, msg)
    good.close(); foreign.close()


def test_concurrent_batches_with_inserts(gpu):
    case, n, graph = P.CASES[0], P.N, P.GRAPH
    d = case[2]
    h, cb = _make(gpu, case, n, graph)
    fa = h.Filter(np.arange(1, n, 3)); fb = h.Filter(np.arange(2, n, 40))
    ok = [set(range(1, n, 3)), set(range(2, n, 40))]
    Q = _queries(case, 16, 5)
    errors = []

    def caller(ef):
        try:
            for _ in range(12):
                gi, gs, gc, gp = h.PqSearchFilteredBatch(Q, K, [fa, fb] * 8, ef=ef, rerank=0, mode=gpu.FILTER_WALK)
                for qi in range(len(Q)):
                    if gc[qi] > K or not set(int(x) for x in gi[qi, :gc[qi]]) <= ok[qi % 2]:
                        errors.append((ef, qi, int(gc[qi])))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    def inserter():
        try:
            Y = O.fill_normal(84, (64, d))
            for j in range(64):
                h.Insert(n + j, Y[j], 0)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=caller, args=(ef,)) for ef in (64, 300)] + [threading.Thread(target=inserter)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    fa.close(); fb.close()
    assert not errors, errors[:5]


def test_cpp_filtered_batcher_over_the_pq_backend(gpu, tmp_path):
    """include/coltt_batcher.hpp: FilteredBatcher over PqFilteredBackend (tests/cpp/pq_filter_batch_test.cpp), 16 callers with their own filters"""
    import shutil
    import subprocess
    import torch
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the C++ consumer"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.lib_path())
    exe = tmp_path / "pq_filter_batch_test"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "pq_filter_batch_test.cpp"), "-o", str(exe), "-L", libdir, "-lcoltt_gpu", f"-Wl,-rpath,{libdir}"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "pq filter batch ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_neighbours_are_unchanged_by_a_batch_call(gpu):
    """PqSearch, PqSearchFiltered and SearchFilteredBatch: the same answers and counters before and after PqSearchFilteredBatch calls over both
    visited sets and the exact scan — the new path leaves no state behind (work counters, visited epochs, region leases)"""
    case, n, graph = ALL[1]
    h, cb, _ = _index(gpu, case, n, graph)
    Q = _queries(case, 9, 6)
    flts = [h.Filter(np.nonzero(P.allow_mask(case, n, frac))[0]) for frac in (0.5, 0.1, 0.01)]
    per_row = [flts[i % 3] for i in range(len(Q))]

    def neighbours():
        out = []
        for ef, rr in ((48, 0), (300, 12)):
            out.append(h.PqSearch(Q, K, ef=ef, rerank=rr, with_stats=True))
            out.append(h.PqSearchFiltered(Q, K, flts[0], ef=ef, rerank=rr, mode=gpu.FILTER_WALK, with_stats=True))
            out.append(h.SearchFilteredBatch(Q, K, per_row, ef=ef, mode=gpu.FILTER_WALK, with_stats=True))
        out.append(h.SearchFilteredBatch(Q, K, per_row, mode=gpu.FILTER_AUTO, with_stats=True))
        return out

    try:
        before = neighbours()
        for ef in (48, 300):
            for mode in (gpu.FILTER_WALK, gpu.FILTER_AUTO):
                h.PqSearchFilteredBatch(Q, K, per_row, ef=ef, rerank=12, mode=mode)
        after = neighbours()
        for a, b in zip(before, after):
            cnt = a[2]
            assert np.array_equal(cnt, b[2]) and a[-1] == b[-1], (a[-1], b[-1])
            for qi in range(len(Q)):
                c = int(cnt[qi])
                assert np.array_equal(a[0][qi, :c], b[0][qi, :c]) and np.array_equal(bits(a[1][qi, :c]), bits(b[1][qi, :c]))
            if len(a) == 5:
                assert np.array_equal(a[3], b[3])
    finally:
        for f in flts:
            f.close()
