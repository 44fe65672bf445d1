"""The certified level-0 row filter (coltt_amd/csrc/row_filter.hpp, hnsw_walk2.hpp: Group8FilterEval; the binary16 shadow rows_h of rows8.hpp) changes
what a search READS, never what it computes: with COLTT_ROW_FILTER=1 ids, score bits and the traversal counters equal the oracle's canonical
Hnsw.Search over the arrays copied out of HBM AND the same index's answers with COLTT_ROW_FILTER=0.  The fixtures are far below the size at which the
filter switches itself on, so every case forces it; the rejected-counter must move wherever a result set fills — no case passes with the filter
silently off."""
import numpy as np
import pytest

from oracle import oracle as O
from util import assert_same_results, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _throughput_kernels(monkeypatch):
    monkeypatch.setenv("COLTT_MW_MAX_NQ", "0")   # batches of any size on the one-wave-per-query kernels (the latency kernel is not filtered)
    monkeypatch.delenv("COLTT_ROW_FILTER", raising=False)
    monkeypatch.delenv("COLTT_ROW_SHADOW", raising=False)


def _gpu_build(gpu, X, lv, metric, quant, cfg=None, batch=64, ids=None):
    import torch
    n, d = X.shape
    gh = gpu.Hnsw(d, metric, cfg, quantization=quant)
    xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
    i = 0
    while i < n:   # no Reserve: the arrays (the shadow among them) grow by reallocation and copy as the index fills
        b = int(min(n - i, max(1, min(batch, i // 16))))
        gh.InsertBatchDevice(xd.data_ptr() + i * d * 4, b, lv[i:i + b], batch=b, first_id=i, ids=None if ids is None else ids[i:i + b])
        i += b
    return gh


def _both(gh, Q, k, ef, monkeypatch):
    """the same call with the filter forced off, then on: (answers off, answers on, evaluations the filter rejected, f32 rows the filtered launch read)"""
    monkeypatch.setenv("COLTT_ROW_FILTER", "0")
    s0 = gh.RowFilterStats()
    off = gh.Search(Q, k, ef=ef, with_stats=True)
    s1 = gh.RowFilterStats()
    assert (s1["rejected"], s1["f32_rows"], s1["launches"]) == (s0["rejected"], s0["f32_rows"], s0["launches"]), "COLTT_ROW_FILTER=0 took a filtered launch"
    monkeypatch.setenv("COLTT_ROW_FILTER", "1")
    on = gh.Search(Q, k, ef=ef, with_stats=True)
    s2 = gh.RowFilterStats()
    monkeypatch.delenv("COLTT_ROW_FILTER")
    _both.survivors = (s2["shadow_rows"] - s1["shadow_rows"]) - (s2["rejected"] - s1["rejected"])   # full-set neighbours the shadow could not reject: phase B
    assert 0 <= _both.survivors <= s2["f32_rows"] - s1["f32_rows"]
    return off, on, s2["rejected"] - s1["rejected"], s2["f32_rows"] - s1["f32_rows"], s2["launches"] - s1["launches"]


def _check(gh, Q, efs, monkeypatch, k=10, del_bits=None, id_of=None, expect_filter=True, metric=O.COSINE, quant=O.Q_NONE):
    d = gh.dim
    g = gh.ExportRaw(); rows = gh.FetchRows()
    assert gh.RowFilterStats()["shadow"] == expect_filter
    for ef in efs:
        (i0, s0, c0, st0), (i1, s1, c1, st1), rej, f32, launches = _both(gh, Q, k, ef, monkeypatch)
        sl, sc, cn, ost, _ = O.csr_search(rows, quant, g["adj0"], g["upper_off"], g["adjU"], d, metric, g["entry"], g["entry_level"],
                                          Q, k, ef, del_bits=del_bits, threads=4)
        for qi in range(len(Q)):
            want = sl[qi, :cn[qi]].astype(np.uint64) if id_of is None else id_of[sl[qi, :cn[qi]]]
            assert_same_results(i1[qi, :c1[qi]], s1[qi, :c1[qi]], want, sc[qi, :cn[qi]], f"filter on, q{qi} ef{ef}")
        assert np.array_equal(i0, i1) and np.array_equal(bits(s0), bits(s1)) and np.array_equal(c0, c1), f"ef{ef}: filter on != filter off"
        assert st0 == st1, (ef, st0, st1)
        assert {k_: st1[k_] for k_ in ost} == ost, (ef, st1, ost)
        if expect_filter:
            assert launches == 1
            # the set fills (the graph reaches far more than ef vertices): the filter must have rejected something, and every level-0 evaluation
            # it saw is either rejected or an f32 row read
            assert rej > 0, f"ef{ef}: the filter rejected nothing"
            assert 0 < rej + f32 <= st1["n_dist"], (rej, f32, st1)
        else:
            assert (rej, f32, launches) == (0, 0, 0)
    return True


@pytest.mark.parametrize("nt", ["0", "1"], ids=["default-loads", "non-temporal-twins"])
@pytest.mark.parametrize("d,n", [(256, 5000), (768, 3000)])
def test_filtered_walk_equals_oracle_and_unfiltered(gpu, monkeypatch, d, n, nt):
    """dense ids, growth without Reserve; ef 32 / 128 on the LDS-hash kernel, 256 on the HBM-visited one.  COLTT_ROWS_NT=1: the non-temporal twins
    (hnsw_search2_rowfilter_kernel<.., true>), the instances a large index takes"""
    monkeypatch.setenv("COLTT_ROWS_NT", nt)
    X = O.fill_normal(7000 + d, (n, d)); lv = O.levels(7001 + d, n)
    gh = _gpu_build(gpu, X, lv, O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=60), batch=256)
    Q = O.fill_normal(7002 + d, (48, d))
    _check(gh, Q, (32, 128, 256), monkeypatch)
    _check(gh, Q[:6], (128,), monkeypatch, k=100)


@pytest.mark.parametrize("d", [256, 768])
def test_filtered_walk_with_removes_and_explicit_ids(gpu, monkeypatch, d):
    n = 2500
    X = O.fill_normal(7100 + d, (n, d)) * np.linspace(0.5, 4.0, n, dtype=np.float32)[:, None]   # norms differ before Normalize
    lv = O.levels(7101 + d, n); ids = (np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(10**9))
    gh = _gpu_build(gpu, X, lv, O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=40), batch=64, ids=ids)
    Q = O.fill_normal(7102 + d, (32, d)) * np.float32(3.0)   # queries are not normalised
    _check(gh, Q, (32, 128, 256), monkeypatch, id_of=ids)
    rng = np.random.default_rng(d)
    dead = rng.choice(n, 300, replace=False)
    for i in dead:
        gh.Remove(int(ids[i]))
    db = np.zeros((n + 31) // 32, np.uint32)
    for i in dead:
        db[i >> 5] |= np.uint32(1 << (i & 31))
    _check(gh, Q, (32, 128, 256), monkeypatch, del_bits=db, id_of=ids)
    # single Inserts on top of the removed ones: the shadow follows every writer of the rows
    Y = O.fill_normal(7103 + d, (30, d)); ly = O.levels(7104 + d, 30)
    for j in range(30):
        gh.Insert(5 + j, Y[j], int(ly[j]))
    db2 = np.zeros((n + 30 + 31) // 32, np.uint32); db2[:len(db)] = db
    _check(gh, Q, (128,), monkeypatch, del_bits=db2, id_of=np.concatenate([ids, np.uint64(5) + np.arange(30, dtype=np.uint64)]))


def test_filtered_walk_after_commit_load_and_bulk_load(gpu, monkeypatch):
    d, n = 256, 2000
    X = O.fill_normal(7200, (n, d)); lv = O.levels(7201, n)
    g1 = _gpu_build(gpu, X, lv, O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=40), batch=64)
    blob = g1.Commit()
    g2 = gpu.Hnsw(d, O.COSINE)
    assert g2.Load(blob) == n
    Q = O.fill_normal(7202, (32, d))
    _check(g2, Q, (32, 128, 256), monkeypatch, id_of=g2.Export()["ids"])   # slots follow the stream's shard order
    # a second Load into the same (already allocated) index, fewer vertices: every slot's shadow is rewritten with its row
    g3 = _gpu_build(gpu, X[:900] * np.float32(-1.0), lv[:900], O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=40), batch=64)
    assert g2.Load(g3.Commit()) == 900
    _check(g2, Q, (128,), monkeypatch, id_of=g2.Export()["ids"])
    oh = O.Hnsw(d, O.COSINE); ids = np.arange(700, dtype=np.uint64); oh.insert_many(ids, X[:700], lv[:700])
    g4 = gpu.Hnsw(d, O.COSINE); g4.BulkLoad(oh.export(with_vectors=False), X[:700])
    _check(g4, Q, (32, 128), monkeypatch, id_of=g4.Export()["ids"])


def test_ties_and_near_ties_with_lower_bound(gpu, monkeypatch):
    """Many neighbours tie or nearly tie with lowerBound: every base vector is stored six times — exact duplicates, and copies that differ from it in
    ONE low bit of one or two elements (the walk still has to cross from cluster to cluster: a collection of nothing but duplicates fills the set with
    ties and leaves the filter nothing it could reject) — and the queries are those base vectors and small perturbations of them.  The shadow cannot separate such rows from the
    set's worst member (their distances differ by less than the margin, or not at all): they must reach the exact f32 evaluation, and admissions at
    d == lowerBound (never admitted: `d < lowerBound`) and one ulp either side of it must come out as the oracle's."""
    d, nb, copies = 256, 400, 6
    rng = np.random.default_rng(99)
    base = O.fill_normal(7300, (nb, d))
    base /= np.linalg.norm(base, axis=1, keepdims=True).astype(np.float32)
    X = np.repeat(base, copies, axis=0)
    for i in range(len(X)):
        c = i % copies
        if c % 3 == 1:     # one low bit of one element, up
            j = int(rng.integers(0, d)); X[i, j] = np.nextafter(X[i, j], np.float32(4), dtype=np.float32)
        elif c % 3 == 2:   # ... or down, or two elements
            for j in rng.integers(0, d, 2):
                X[i, j] = np.nextafter(X[i, j], np.float32(-4), dtype=np.float32)
    X = X[rng.permutation(len(X))]
    n = len(X); lv = O.levels(7301, n)
    gh = _gpu_build(gpu, X, lv, O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=80), batch=64)
    Q = np.concatenate([base[:16], base[16:32] + O.fill_normal(7302, (16, d)) * np.float32(1e-4), O.fill_normal(7303, (16, d))])
    d_ = gh.dim
    g = gh.ExportRaw(); rows = gh.FetchRows()
    for ef in (32, 64, 128, 256):
        (i0, s0, c0, st0), (i1, s1, c1, st1), rej, f32, launches = _both(gh, Q, 20, ef, monkeypatch)
        sl, sc, cn, ost, _ = O.csr_search(rows, O.Q_NONE, g["adj0"], g["upper_off"], g["adjU"], d_, O.COSINE, g["entry"], g["entry_level"], Q, 20, ef, threads=4)
        for qi in range(len(Q)):
            assert_same_results(i1[qi, :c1[qi]], s1[qi, :c1[qi]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], f"ties q{qi} ef{ef}")
        assert np.array_equal(i0, i1) and np.array_equal(bits(s0), bits(s1)) and np.array_equal(c0, c1) and st0 == st1
        assert {k_: st1[k_] for k_ in ost} == ost
        assert launches == 1 and f32 > 0 and rej > 0 and rej + f32 <= st1["n_dist"]
        assert _both.survivors > 0, "no full-set neighbour reached the exact evaluation: phase B did not run at the boundary"


@pytest.mark.parametrize("metric,quant,d", [(O.L2, O.Q_NONE, 256), (O.COSINE, O.Q_F16, 256), (O.COSINE, O.Q_BF16, 256), (O.COSINE, O.Q_NONE, 128),
                                            (O.COSINE, O.Q_NONE, 320), (O.COSINE, O.Q_NONE, 100)])
def test_indexes_the_filter_does_not_cover_have_no_shadow(gpu, monkeypatch, metric, quant, d):
    """L2 (rows are not normalised), 2-byte rows, rows that are not line-transposed (dim 128 by default, dim 100) and line-transposed rows whose length
    is not a whole number of shadow bursts (dim 320): no shadow, no filtered launch, no rejections — and the answers are the oracle's as before"""
    n = 1500
    X = O.fill_normal(7400 + d, (n, d)); lv = O.levels(7401 + d, n)
    gh = _gpu_build(gpu, X, lv, metric, quant, gpu.HnswCfg.default(ef_construction=40), batch=64)
    Q = O.fill_normal(7402 + d, (16, d))
    _check(gh, Q, (32, 128, 256), monkeypatch, expect_filter=False, metric=metric, quant=quant)


def test_no_shadow_when_the_index_is_created_without_one(gpu, monkeypatch):
    d, n = 256, 1500
    X = O.fill_normal(7500, (n, d)); lv = O.levels(7501, n)
    monkeypatch.setenv("COLTT_ROW_SHADOW", "0")
    gh = _gpu_build(gpu, X, lv, O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=40), batch=64)
    monkeypatch.delenv("COLTT_ROW_SHADOW")
    Q = O.fill_normal(7502, (16, d))
    _check(gh, Q, (32, 128), monkeypatch, expect_filter=False)
    # ... and an index created afterwards has one again; unset COLTT_ROW_FILTER leaves a small index unfiltered (the filter is for row arrays far larger than the caches)
    g2 = _gpu_build(gpu, X, lv, O.COSINE, O.Q_NONE, gpu.HnswCfg.default(ef_construction=40), batch=64)
    assert g2.RowFilterStats()["shadow"]
    g2.Search(Q, 10, ef=128)
    assert g2.RowFilterStats()["launches"] == 0
    monkeypatch.setenv("COLTT_ROWS_NT", "1")   # forcing the non-temporal hint is not the size rule: still unfiltered
    g2.Search(Q, 10, ef=128)
    assert g2.RowFilterStats()["launches"] == 0
    monkeypatch.delenv("COLTT_ROWS_NT")
    _check(g2, Q, (128,), monkeypatch)
