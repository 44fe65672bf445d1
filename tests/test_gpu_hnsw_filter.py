"""Filtered HNSW search on the GPU (coltt_hnsw_filter_create / coltt_hnsw_search_filtered; include/coltt_gpu.h, "Filtered HNSW search" —
an extension the reference does not have) against its CPU restatement (tests/filtered_ref.py) over GPU-built graphs: WALK (ids, score bits,
counts, counters) over the LDS-hash and the HBM-map walks, EXACT against a brute force, the AUTO rule, the filter's lifecycle, answer
quality against a post-filter, concurrency with inserts."""
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import filtered_ref as F

pytestmark = pytest.mark.gpu

K = 10
# (quant, n, d): the shapes of the issue — 128-d f32 rows (pair-owned core), 768-d 2-byte rows (line-transposed), 64-d f8
SHAPES = [(O.Q_NONE, 5000, 128), (O.Q_F16, 1800, 768), (O.Q_BF16, 1800, 768), (O.Q_F8, 3000, 64)]


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
        seed = 100 + quant * 10 + metric
        X = O.fill_normal(seed, (n, d)); lv = O.levels(seed + 1, n)
        idv = (np.arange(n, dtype=np.uint64) * 7 + 1000) if ids else None
        gh = _build(gpu, X, lv, metric, quant, ids=idv)
        _CACHE[key] = (gh, X, idv)
    return _CACHE[key]


def _view(gh, metric, quant):
    g = gh.ExportRaw()
    rows = F.decode(quant, gh.FetchRows())
    return g, rows


def _slot_ids(ids, slots):
    return slots.astype(np.uint64) if ids is None else ids[slots]


@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
@pytest.mark.parametrize("quant,n,d", SHAPES)
def test_walk_equals_the_restatement(gpu, metric, quant, n, d):
    gh, X, ids = _index(gpu, quant, n, d, metric, ids=(quant == O.Q_F16))
    g, rows = _view(gh, metric, quant)
    Q = O.fill_normal(7 + quant, (6, d))
    rng = np.random.default_rng(quant * 3 + metric)
    for frac in (0.5, 0.1, 0.01):
        allow = rng.random(n) < frac
        idl = _slot_ids(ids, np.nonzero(allow)[0])
        with gh.Filter(idl) as flt:
            assert flt.allowed == int(allow.sum())
            for ef in (64, 256):            # LDS hash | HBM byte map
                gi, gs, gc, st = gh.SearchFiltered(Q, K, flt, ef=ef, mode=gpu.FILTER_WALK, with_stats=True)
                assert st["path"] == gpu.FILTER_WALK and st["ef_walk"] == ef and st["n_visit_resets"] == 0
                tot = {"n_dist": 0, "n_exp": 0, "n_hops": 0}
                for qi in range(len(Q)):
                    q = F.prep_query(metric, quant, Q[qi])
                    s, v, t = F.walk(rows, g["adj0"], g["upper_off"], g["adjU"], metric, g["entry"], g["entry_level"], q, K, ef, allow)
                    c = gc[qi]
                    assert c == len(s), (frac, ef, qi)
                    assert np.array_equal(gi[qi, :c], _slot_ids(ids, s)), (frac, ef, qi, gi[qi, :c], s)
                    assert np.array_equal(bits(gs[qi, :c]), bits(v)), (frac, ef, qi)
                    for kk in tot:
                        tot[kk] += t[kk]
                assert {kk: st[kk] for kk in tot} == tot, (frac, ef, st, tot)


@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
@pytest.mark.parametrize("quant,n,d", [s for s in SHAPES if s[0] in (O.Q_NONE, O.Q_F16)])
def test_all_ones_filter_walks_as_search(gpu, metric, quant, n, d):
    """the same walk as Search at that ef (counters equal); R is element-wise <= Search's answer (it also keeps evaluated neighbours the
    stale lowerBound refused: tests/test_filtered_ref.py) and equal to it on most queries.  (f8 rows: distance ties are routine.)"""
    gh, X, ids = _index(gpu, quant, n, d, metric, ids=(quant == O.Q_F16))
    Q = O.fill_normal(21, (16, d))
    with gh.Filter(_slot_ids(ids, np.arange(n))) as flt:
        assert flt.allowed == n
        for ef in (64, 256):
            si, ss, sc, sst = gh.Search(Q, K, ef=ef, with_stats=True)
            fi, fs, fc, fst = gh.SearchFiltered(Q, K, flt, ef=ef, mode=gpu.FILTER_WALK, with_stats=True)
            assert {kk: fst[kk] for kk in ("n_dist", "n_exp", "n_hops")} == {kk: sst[kk] for kk in ("n_dist", "n_exp", "n_hops")}, ef
            same = 0
            for qi in range(len(Q)):
                assert fc[qi] == sc[qi]
                a = [(int(b) << 32) | int(i) for b, i in zip(bits(fs[qi, :fc[qi]]), fi[qi, :fc[qi]])]   # ids ascend with slots here
                w = [(int(b) << 32) | int(i) for b, i in zip(bits(ss[qi, :sc[qi]]), si[qi, :sc[qi]])]
                assert all(x <= y for x, y in zip(a, w)), (ef, qi)
                same += np.array_equal(fi[qi, :fc[qi]], si[qi, :sc[qi]]) and np.array_equal(bits(fs[qi, :fc[qi]]), bits(ss[qi, :sc[qi]]))
            assert same >= (len(Q) * 3) // 4, (ef, same)


@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
@pytest.mark.parametrize("quant,n,d", SHAPES)
def test_exact_equals_brute_force(gpu, metric, quant, n, d):
    gh, X, ids = _index(gpu, quant, n, d, metric, ids=(quant == O.Q_F16))
    _, rows = _view(gh, metric, quant)
    Q = O.fill_normal(33 + quant, (20, d))
    rng = np.random.default_rng(5)
    for frac in (0.3, 0.004):
        allow = rng.random(n) < frac
        A = int(allow.sum())
        with gh.Filter(_slot_ids(ids, np.nonzero(allow)[0])) as flt:
            for k in (K, A + 5):             # including k > A
                gi, gs, gc, st = gh.SearchFiltered(Q, k, flt, mode=gpu.FILTER_EXACT, with_stats=True)
                assert st["path"] == gpu.FILTER_EXACT and st["ef_walk"] == 0 and st["n_exact_rows"] == A * len(Q)
                for qi in range(len(Q)):
                    s, v = F.exact(rows, metric, F.prep_query(metric, quant, Q[qi]), k, allow)
                    assert gc[qi] == len(s) == min(k, A)
                    assert np.array_equal(gi[qi, :gc[qi]], _slot_ids(ids, s)), (frac, k, qi)
                    assert np.array_equal(bits(gs[qi, :gc[qi]]), bits(v)), (frac, k, qi)


def test_auto_follows_the_rule(gpu):
    gh, X, ids = _index(gpu, O.Q_NONE, 5000, 128, O.L2)
    Q = O.fill_normal(3, (4, 128))
    rng = np.random.default_rng(9)
    n_live = gh.Len()
    for frac in (1.0, 0.9, 0.5, 0.1, 0.01):
        allow = rng.random(5000) < frac
        with gh.Filter(np.nonzero(allow)[0]) as flt:
            for ef in (20, 64, 128):
                for k in (10, 100):
                    _, _, _, st = gh.SearchFiltered(Q, k, flt, ef=ef, with_stats=True)
                    assert (st["path"], st["ef_walk"]) == F.auto_path(flt.allowed, n_live, max(ef, k)), (frac, ef, k, st)


def test_filter_lifecycle(gpu):
    n, d = 3000, 64
    X = O.fill_normal(61, (n, d)); lv = O.levels(62, n)
    gh = _build(gpu, X, lv, O.L2, O.Q_NONE)
    Q = X[:8] + 0.01
    # unknown and duplicate ids are reflected in .allowed
    with gh.Filter([5, 5, 5, 7, 10 ** 9, n, n + 5]) as f:
        assert f.allowed == 2
    allow_ids = np.arange(0, n, 3, dtype=np.uint64)
    flt = gh.Filter(allow_ids)
    assert flt.allowed == len(allow_ids)
    # removed after the filter was built: never returned
    gone = [int(i) for i in allow_ids[:40]]
    for i in gone:
        gh.Remove(i)
    # inserted after it (copies of the queries: they would be the nearest): never returned
    for j in range(8):
        gh.Insert(n + j, Q[j], 0)
    for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
        gi, gs, gc = gh.SearchFiltered(Q, K, flt, ef=64, mode=mode)
        for qi in range(len(Q)):
            got = set(int(x) for x in gi[qi, :gc[qi]])
            assert gc[qi] == K and got <= set(int(x) for x in allow_ids[40:]), (mode, qi)
    # a filter built from removed / unknown ids only is empty: counts 0, not an error
    with gh.Filter(gone + [10 ** 12]) as empty:
        assert empty.allowed == 0
        for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
            _, _, gc = gh.SearchFiltered(Q, K, empty, mode=mode)
            assert (gc == 0).all()
    # another index: COLTT_E_INVALID
    other = _build(gpu, X[:500], lv[:500], O.L2, O.Q_NONE)
    with pytest.raises(gpu.ColttError) as e:
        other.SearchFiltered(Q, K, flt)
    assert e.value.code == -1
    # Load renumbers the index: the filter is stale
    blob = other.Commit()
    gh.Load(blob)
    with pytest.raises(gpu.ColttError) as e:
        gh.SearchFiltered(Q, K, flt)
    assert e.value.code == -1
    with gh.Filter([1, 2, 3]) as fresh:      # a filter built after the Load serves
        _, _, gc = gh.SearchFiltered(Q, K, fresh, mode=gpu.FILTER_EXACT)
        assert (gc == 3).all()
    flt.close()
    # an empty index
    e_idx = gpu.Hnsw(d, gpu.EUCLIDEAN)
    with e_idx.Filter([1, 2]) as f0:
        assert f0.allowed == 0
        _, _, gc = e_idx.SearchFiltered(Q, K, f0)
        assert (gc == 0).all()


def _lowrank(seed, n, d, rank=8):
    rng = np.random.default_rng(seed)
    basis = rng.standard_normal((rank, d)).astype(np.float32)
    centers = rng.standard_normal((64, rank)).astype(np.float32) * 3
    lab = rng.integers(0, 64, n)
    Z = centers[lab] + rng.standard_normal((n, rank)).astype(np.float32)
    return (Z @ basis + 0.05 * rng.standard_normal((n, d))).astype(np.float32)


def _recall(got, cnt, want, wcnt):
    r = []
    for i in range(len(want)):
        w = set(int(x) for x in want[i, :wcnt[i]])
        if w:
            r.append(len(w & set(int(x) for x in got[i, :cnt[i]])) / len(w))
    return float(np.mean(r))


def test_quality_against_post_filter(gpu):
    """clustered rows, cfg ef 20: AUTO at 10 % is within 0.02 of the unfiltered recall@10 and beats a corrected 3 k post-filter at 10 % and 1 %"""
    n, d = 80_000, 64
    X = _lowrank(71, n, d); lv = O.levels(72, n)
    gh = _build(gpu, X, lv, O.COSINE, O.Q_NONE, batch=512)
    Q = _lowrank(73, 200, d)
    rng = np.random.default_rng(74)
    with gh.Filter(np.arange(n)) as everyone:
        ti, _, tc = gh.SearchFiltered(Q, K, everyone, mode=gpu.FILTER_EXACT)
    ui, _, uc = gh.Search(Q, K)
    base = _recall(ui, uc, ti, tc)
    pi, _, pc = gh.Search(Q, 3 * K)
    for frac in (0.1, 0.01):
        allow = rng.random(n) < frac
        with gh.Filter(np.nonzero(allow)[0]) as flt:
            ei, _, ec = gh.SearchFiltered(Q, K, flt, mode=gpu.FILTER_EXACT)
            ai, _, ac, st = gh.SearchFiltered(Q, K, flt, with_stats=True)
            assert (st["path"], st["ef_walk"]) == F.auto_path(flt.allowed, n, 20)
            ra = _recall(ai, ac, ei, ec)
            post = np.zeros((len(Q), K), np.uint64); postc = np.zeros(len(Q), np.uint32)
            for qi in range(len(Q)):             # the corrected post-filter: the allowed ones among 3 k unfiltered candidates
                keep = [x for x in pi[qi, :pc[qi]] if allow[int(x)]][:K]
                post[qi, :len(keep)] = keep; postc[qi] = len(keep)
            rp = _recall(post, postc, ei, ec)
            if frac == 0.1:
                assert st["path"] == gpu.FILTER_WALK
                assert ra >= base - 0.02, (ra, base)
            assert ra > rp, (frac, ra, rp)


def test_concurrent_searches_with_inserts(gpu):
    n, d = 4000, 64
    X = O.fill_normal(81, (n, d)); lv = O.levels(82, n)
    gh = _build(gpu, X, lv, O.L2, O.Q_NONE)
    allow_ids = np.arange(1, n, 5, dtype=np.uint64)
    ok_set = set(int(x) for x in allow_ids)
    flt = gh.Filter(allow_ids)
    Q = O.fill_normal(83, (32, d))
    errors = []
    stop = threading.Event()

    def searcher(mode):
        try:
            for _ in range(25):
                gi, gs, gc = gh.SearchFiltered(Q, K, flt, ef=64, mode=mode)
                for qi in range(len(Q)):
                    if gc[qi] != K or not set(int(x) for x in gi[qi, :gc[qi]]) <= ok_set:
                        errors.append((mode, qi))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    def inserter():
        try:
            Y = O.fill_normal(84, (200, d))
            for j in range(200):
                if stop.is_set():
                    break
                gh.Insert(n + j, Y[j], 0)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=searcher, args=(m,)) for m in (gpu.FILTER_WALK, gpu.FILTER_AUTO)]
    ti = threading.Thread(target=inserter)
    for t in ts + [ti]:
        t.start()
    for t in ts:
        t.join()
    stop.set(); ti.join()
    flt.close()
    assert not errors, errors[:5]


def test_cpp_mirror_filter(gpu, tmp_path):
    """include/coltt_gpu.hpp: Hnsw::Filter / Hnsw::SearchFiltered from a compiled C++ consumer (tests/cpp/filter_test.cpp)"""
    import os
    import shutil
    import subprocess
    import torch
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the C++ consumer"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.lib_path())
    exe = tmp_path / "filter_test"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "filter_test.cpp"), "-o", str(exe), "-L", libdir, "-lcoltt_gpu", f"-Wl,-rpath,{libdir}"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "filter ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
