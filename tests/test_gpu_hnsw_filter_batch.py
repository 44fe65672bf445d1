"""Filtered HNSW search with a filter per query (coltt_hnsw_search_filtered_batch; include/coltt_gpu.h, "A FILTER PER QUERY"): row i of a
batch call equals the single-filter call on query i alone — ids, score bits, count, path — and the batch's counters are the sums of the
single calls'.  Over every codec and both metrics, the WALK / EXACT / AUTO modes, a batch that needs both walk launches and the exact scan at
once, the CPU restatement (tests/filtered_ref.py), edge cases, all-or-nothing validation, concurrency and a C++ consumer of the batcher."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import filtered_ref as F

pytestmark = pytest.mark.gpu

K = 10
SHAPES = [(O.Q_NONE, 5000, 128), (O.Q_F16, 1800, 768), (O.Q_BF16, 1800, 768), (O.Q_F8, 3000, 64)]
COUNTERS = ("n_dist", "n_exp", "n_hops", "n_visit_resets", "n_exact_rows")


def _build(gpu, X, lv, metric, quant, ids=None, batch=128, cfg=None):
    import torch
    n, d = X.shape
    gh = gpu.Hnsw(d, metric, cfg, quantization=quant)
    xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
    i = 0
    while i < n:
        b = int(min(n - i, max(1, min(batch, i // 16))))
        gh.InsertBatchDevice(xd.data_ptr() + i * d * 4, b, lv[i:i + b], batch=b, first_id=i, ids=None if ids is None else ids[i:i + b])
        i += b
    return gh


_CACHE = {}


def _index(gpu, quant, n, d, metric, ids=False):
    key = (quant, n, d, metric, ids)
    if key not in _CACHE:
        seed = 300 + quant * 10 + metric
        X = O.fill_normal(seed, (n, d)); lv = O.levels(seed + 1, n)
        idv = (np.arange(n, dtype=np.uint64) * 7 + 1000) if ids else None
        _CACHE[key] = (_build(gpu, X, lv, metric, quant, ids=idv), X, idv)
    return _CACHE[key]


def _slot_ids(ids, slots):
    return slots.astype(np.uint64) if ids is None else ids[slots]


def _singles(gh, Q, k, flts, ef, mode):
    """the reference answer: one single-filter call per query"""
    nq = len(Q)
    ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32); paths = np.zeros(nq, np.int32)
    tot = {c: 0 for c in COUNTERS}
    ef_walk = 0
    for i in range(nq):
        gi, gs, gc, st = gh.SearchFiltered(Q[i:i + 1], k, flts[i], ef=ef, mode=mode, with_stats=True)
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


def _check_batch(gpu, gh, Q, k, flts, ef, mode, msg=""):
    bi, bs, bc, bp, st = gh.SearchFilteredBatch(Q, k, flts, ef=ef, mode=mode, with_stats=True)
    want = _singles(gh, Q, k, flts, ef, mode)
    _assert_equal_rows((bi, bs, bc, bp), want, msg)
    assert {c: st[c] for c in COUNTERS} == want[4], (msg, st, want[4])
    assert st["ef_walk"] == want[5], (msg, st, want[5])
    kinds = set(int(p) for p in want[3])
    assert st["path"] == (kinds.pop() if len(kinds) == 1 else gpu.FILTER_AUTO), (msg, st, want[3])
    return bi, bs, bc, bp, st


@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
@pytest.mark.parametrize("quant,n,d", SHAPES)
def test_batch_equals_single_calls(gpu, metric, quant, n, d):
    gh, X, ids = _index(gpu, quant, n, d, metric, ids=(quant == O.Q_F16))
    rng = np.random.default_rng(quant * 5 + metric)
    flts = [gh.Filter(_slot_ids(ids, np.nonzero(rng.random(n) < frac)[0])) for frac in (1.0, 0.5, 0.1, 0.01)]
    try:
        Q = O.fill_normal(40 + quant, (11, d))
        per_row = [flts[(i * 3) % len(flts)] for i in range(len(Q))]
        for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
            for ef in (64, 256):            # WALK: the LDS hash | the HBM byte map
                _check_batch(gpu, gh, Q, K, per_row, ef, mode, (mode, ef))
    finally:
        for f in flts:
            f.close()


def test_one_batch_takes_both_walks_and_the_exact_scan(gpu):
    """20 000 vertices, cfg ef 64; filters at 100 %, 40 %, 10 % interleaved: AUTO walks at 64 (LDS hash) and 160 (HBM byte map) and
    sends the 10 % rows to the exact scan — all in one call"""
    n, d = 20_000, 32
    X = O.fill_normal(501, (n, d)); lv = O.levels(502, n)
    gh = _build(gpu, X, lv, O.L2, O.Q_NONE, batch=512, cfg=gpu.HnswCfg.default(ef=64))
    rng = np.random.default_rng(503)
    flts = [gh.Filter(rng.permutation(n)[:m]) for m in (n, n * 4 // 10, n // 10)]
    try:
        Q = O.fill_normal(504, (30, d))
        per_row = [flts[i % 3] for i in range(len(Q))]
        want_paths = [F.auto_path(f.allowed, n, 64) for f in flts]
        assert want_paths[0] == (F.WALK, 64) and want_paths[1] == (F.WALK, 160) and want_paths[2][0] == F.EXACT, want_paths
        bi, bs, bc, bp, st = _check_batch(gpu, gh, Q, K, per_row, 0, gpu.FILTER_AUTO, "mixed")
        assert st["path"] == gpu.FILTER_AUTO and st["ef_walk"] == 160
        assert [int(p) for p in bp[:3]] == [F.WALK, F.WALK, F.EXACT]
        assert (bc == K).all()
    finally:
        for f in flts:
            f.close()


def test_batch_equals_the_restatement(gpu):
    gh, X, ids = _index(gpu, O.Q_NONE, 5000, 128, O.L2)
    g = gh.ExportRaw()
    rows = F.decode(O.Q_NONE, gh.FetchRows())
    rng = np.random.default_rng(17)
    allows = [rng.random(5000) < frac for frac in (0.3, 0.05)]
    flts = [gh.Filter(np.nonzero(a)[0]) for a in allows]
    try:
        Q = O.fill_normal(18, (6, 128))
        pick = [i % 2 for i in range(len(Q))]
        for mode, ef in ((gpu.FILTER_WALK, 64), (gpu.FILTER_WALK, 256), (gpu.FILTER_EXACT, 0)):
            gi, gs, gc, gp = gh.SearchFilteredBatch(Q, K, [flts[p] for p in pick], ef=ef, mode=mode)
            for qi in range(len(Q)):
                q = F.prep_query(O.L2, O.Q_NONE, Q[qi])
                if mode == gpu.FILTER_WALK:
                    s, v, _ = F.walk(rows, g["adj0"], g["upper_off"], g["adjU"], O.L2, g["entry"], g["entry_level"], q, K, ef, allows[pick[qi]])
                else:
                    s, v = F.exact(rows, O.L2, q, K, allows[pick[qi]])
                c = int(gc[qi])
                assert gp[qi] == mode and c == len(s), (mode, ef, qi)
                assert np.array_equal(gi[qi, :c], s.astype(np.uint64)), (mode, ef, qi)
                assert np.array_equal(bits(gs[qi, :c]), bits(v)), (mode, ef, qi)
    finally:
        for f in flts:
            f.close()


def test_same_filter_in_every_row_equals_one_call(gpu):
    gh, X, ids = _index(gpu, O.Q_F16, 1800, 768, O.COSINE, ids=True)
    rng = np.random.default_rng(23)
    with gh.Filter(_slot_ids(ids, np.nonzero(rng.random(1800) < 0.2)[0])) as flt:
        Q = O.fill_normal(24, (40, 768))
        for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
            si, ss, sc, sst = gh.SearchFiltered(Q, K, flt, mode=mode, with_stats=True)
            bi, bs, bc, bp, bst = gh.SearchFilteredBatch(Q, K, [flt] * len(Q), mode=mode, with_stats=True)
            _assert_equal_rows((bi, bs, bc, bp), (si, ss, sc, np.full(len(Q), sst["path"], np.int32)), mode)
            assert bst == sst, (mode, bst, sst)


def test_edge_cases(gpu):
    n, d = 3000, 64
    X = O.fill_normal(601, (n, d)); lv = O.levels(602, n)
    gh = _build(gpu, X, lv, O.L2, O.Q_NONE)
    Q = X[:8] + 0.01
    a_ids = np.arange(0, n, 3, dtype=np.uint64)
    fa = gh.Filter(a_ids)
    fb = gh.Filter(np.arange(1, n, 50, dtype=np.uint64))
    few = gh.Filter([4, 8, 15])                        # k larger than allowed
    empty = gh.Filter([10 ** 12])                      # empty amid non-empty ones
    assert empty.allowed == 0 and few.allowed == 3
    per_row = [fa, empty, fb, fa, few, empty, fb, fa]  # repeated handles
    for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
        bi, bs, bc, bp, st = _check_batch(gpu, gh, Q, K, per_row, 64, mode, mode)
        assert bc[1] == 0 and bc[5] == 0
        assert bc[4] == 3 or mode == gpu.FILTER_WALK   # (a walk holds only the allowed vertices it meets)
    # removes after the filter was built: tombstones never returned; inserts after it: not allowed
    gone = [int(i) for i in a_ids[:40]]
    for i in gone:
        gh.Remove(i)
    for j in range(8):
        gh.Insert(n + j, Q[j], 0)
    ok = set(int(x) for x in a_ids[40:])
    for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
        bi, bs, bc, bp = _check_batch(gpu, gh, Q, K, [fa] * 8, 64, mode, ("removed", mode))[:4]
        for qi in range(8):
            assert bc[qi] == K and set(int(x) for x in bi[qi, :bc[qi]]) <= ok, (mode, qi)
    # nq = 0 and nq = 1
    bi, bs, bc, bp, st = gh.SearchFilteredBatch(np.zeros((0, d), np.float32), K, [], with_stats=True)
    assert bc.shape == (0,) and st["path"] == 0 and st["n_dist"] == 0
    _check_batch(gpu, gh, Q[:1], K, [fb], 64, gpu.FILTER_AUTO, "nq=1")
    # an empty index: every count 0
    e_idx = gpu.Hnsw(d, gpu.EUCLIDEAN)
    with e_idx.Filter([1, 2]) as f0:
        _, _, bc, _ = e_idx.SearchFilteredBatch(Q[:3], K, [f0] * 3)
        assert (bc == 0).all()
    for f in (fa, fb, few, empty):
        f.close()


def _raw_batch(gpu, gh, handles, Q, k=K, ef=0, mode=0, null_filters=False):
    L = gpu.lib()
    nq = len(Q)
    fh = np.array(handles, np.uint64)
    q = np.ascontiguousarray(Q, np.float32)
    ids = np.zeros((max(nq, 1), k), np.uint64); sc = np.zeros((max(nq, 1), k), np.float32); cnt = np.zeros(max(nq, 1), np.uint32)
    rc = L.coltt_hnsw_search_filtered_batch(gh.h, None if null_filters else fh.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                            C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_int(mode), ids.ctypes.data_as(C.c_void_p),
                                            sc.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), None, None)
    return rc, L.coltt_last_error().decode()


def test_validation_is_all_or_nothing(gpu):
    n, d = 2000, 32
    X = O.fill_normal(701, (n, d)); lv = O.levels(702, n)
    gh = _build(gpu, X, lv, O.L2, O.Q_NONE)
    other = _build(gpu, X[:300], lv[:300], O.L2, O.Q_NONE)
    Q = X[:5] + 0.01
    good = gh.Filter(np.arange(0, n, 2))
    g = good.h.value
    dead = gh.Filter([1, 2, 3]); dead_h = dead.h.value; dead.close()
    foreign = other.Filter([1, 2, 3])
    cases = [("null", None, -1, "NULL filters"),
             ("unknown", 0xDEADBEEF, -3, "position 2"),
             ("destroyed", dead_h, -3, "position 2"),
             ("foreign", foreign.h.value, -1, "position 2")]
    for name, bad, code, text in cases:
        if name == "null":
            rc, msg = _raw_batch(gpu, gh, [g] * 5, Q, null_filters=True)
        else:
            rc, msg = _raw_batch(gpu, gh, [g, g, bad, g, g], Q)
        assert rc == code and text in msg, (name, rc, msg)
    rc, msg = _raw_batch(gpu, gh, [g] * 5, Q, mode=7)
    assert rc == -1 and "mode" in msg, (rc, msg)
    rc, msg = _raw_batch(gpu, gh, [g] * 5, Q, ef=5000)
    assert rc == -4, (rc, msg)
    # the index still answers, and the same as before
    _check_batch(gpu, gh, Q, K, [good] * 5, 64, gpu.FILTER_AUTO, "after errors")
    # stale: built before a Load
    gh.Load(other.Commit())
    with gh.Filter([1, 2, 3, 4]) as fresh:
        rc, msg = _raw_batch(gpu, gh, [fresh.h.value, fresh.h.value, g, fresh.h.value], Q[:4])
        assert rc == -1 and "position 2" in msg and "stale" in msg, (rc, msg)
        _, _, bc, _ = gh.SearchFilteredBatch(Q[:4], K, [fresh] * 4, mode=gpu.FILTER_EXACT)
        assert (bc == 4).all()
    good.close(); foreign.close()


def test_concurrent_batches_with_filter_churn(gpu):
    gh, X, ids = _index(gpu, O.Q_NONE, 5000, 128, O.L2)
    Q = O.fill_normal(801, (16, 128))
    rng = np.random.default_rng(802)
    per_thread = []
    for t in range(8):
        fl = [gh.Filter(np.nonzero(rng.random(5000) < frac)[0]) for frac in (0.5, 0.05, 0.01)]
        rows = [fl[(i + t) % 3] for i in range(len(Q))]
        per_thread.append((fl, rows, _singles(gh, Q, K, rows, 0, gpu.FILTER_AUTO)))
    errors = []
    stop = threading.Event()

    def caller(t):
        fl, rows, want = per_thread[t]
        try:
            for _ in range(6):
                got = gh.SearchFilteredBatch(Q, K, rows)
                _assert_equal_rows(got, want, t)
        except Exception as e:   # noqa: BLE001
            errors.append((t, repr(e)[:300]))

    def churn():
        try:
            while not stop.is_set():
                f = gh.Filter(np.arange(0, 5000, 7))
                f.close()
        except Exception as e:   # noqa: BLE001
            errors.append(("churn", repr(e)))

    ts = [threading.Thread(target=caller, args=(t,)) for t in range(8)]
    tc = threading.Thread(target=churn)
    for t in ts + [tc]:
        t.start()
    for t in ts:
        t.join()
    stop.set(); tc.join()
    for fl, _, _ in per_thread:
        for f in fl:
            f.close()
    assert not errors, errors[:3]


def test_concurrent_batches_with_inserts(gpu):
    n, d = 4000, 64
    X = O.fill_normal(811, (n, d)); lv = O.levels(812, n)
    gh = _build(gpu, X, lv, O.L2, O.Q_NONE)
    fa = gh.Filter(np.arange(1, n, 5)); fb = gh.Filter(np.arange(2, n, 40))
    ok = [set(range(1, n, 5)), set(range(2, n, 40))]
    Q = O.fill_normal(813, (16, d))
    errors = []

    def caller():
        try:
            for _ in range(15):
                gi, gs, gc, gp = gh.SearchFilteredBatch(Q, K, [fa, fb] * 8, ef=64)
                for qi in range(len(Q)):
                    if gc[qi] != K or not set(int(x) for x in gi[qi, :gc[qi]]) <= ok[qi % 2]:
                        errors.append(qi)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    def inserter():
        try:
            Y = O.fill_normal(814, (150, d))
            for j in range(150):
                gh.Insert(n + j, Y[j], 0)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=caller) for _ in range(3)] + [threading.Thread(target=inserter)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    fa.close(); fb.close()
    assert not errors, errors[:5]


def test_cpp_filtered_batcher_over_the_index(gpu, tmp_path):
    """include/coltt_batcher.hpp: FilteredBatcher over coltt::Hnsw (tests/cpp/filter_batch_test.cpp), 64 callers with their own filters"""
    import os
    import shutil
    import subprocess
    import torch
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the C++ consumer"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.lib_path())
    exe = tmp_path / "filter_batch_test"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "filter_batch_test.cpp"), "-o", str(exe), "-L", libdir, "-lcoltt_gpu", f"-Wl,-rpath,{libdir}"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "filter batch ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
