"""The level-0 row filter over the 8-BIT shadow (coltt_amd/csrc/row_filter8.hpp; rows8.hpp: rows_b, group8_stream_b; hnsw_walk2.hpp:
Group8FilterEval<.., 8>) changes what a search READS, never what it computes.  One index keeps BOTH shadows (COLTT_ROW_SHADOW_BITS=both) and answers the
same call with the filter off, over the 8-bit shadow and over the binary16 one: ids, score bits, counts and the traversal counters equal the oracle's
canonical Hnsw.Search over the arrays copied out of HBM and each other.  The 8-bit arrays themselves — codes, (scale, error norm) per slot and per
level-0 edge — equal the numpy restatement of the quantiser after every kind of writer."""
import numpy as np
import pytest

from oracle import oracle as O
from row_filter8_ref import quantise
from util import assert_same_results, bits

pytestmark = pytest.mark.gpu

KNOBS = ("COLTT_ROW_FILTER", "COLTT_ROW_FILTER_BITS", "COLTT_ROW_SHADOW", "COLTT_ROW_SHADOW_BITS")


@pytest.fixture(autouse=True)
def _throughput_kernels(monkeypatch):
    monkeypatch.setenv("COLTT_MW_MAX_NQ", "0")   # batches of any size on the one-wave-per-query kernels (the latency kernel is not filtered)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("COLTT_ROW_SHADOW_BITS", "both")


def _gpu_build(gpu, X, lv, cfg=None, batch=64, ids=None):
    import torch
    n, d = X.shape
    gh = gpu.Hnsw(d, O.COSINE, cfg, quantization=O.Q_NONE)
    xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
    i = 0
    while i < n:   # no Reserve: the arrays (both shadows, the per-edge metadata) grow by reallocation and copy as the index fills
        b = int(min(n - i, max(1, min(batch, i // 16))))
        gh.InsertBatchDevice(xd.data_ptr() + i * d * 4, b, lv[i:i + b], batch=b, first_id=i, ids=None if ids is None else ids[i:i + b])
        i += b
    return gh


def _sides(gh, Q, k, ef, monkeypatch, sides=("off", "8", "16")):
    """the same call per side: {side: (answers, counter deltas)}"""
    out = {}
    for side in sides:
        monkeypatch.setenv("COLTT_ROW_FILTER", "0" if side == "off" else "1")
        if side != "off":
            monkeypatch.setenv("COLTT_ROW_FILTER_BITS", side)
        a = gh.RowFilterStats()
        res = gh.Search(Q, k, ef=ef, with_stats=True)
        b = gh.RowFilterStats()
        out[side] = (res, {kk: b[kk] - a[kk] for kk in ("rejected", "f32_rows", "shadow_rows", "launches")})
        monkeypatch.delenv("COLTT_ROW_FILTER_BITS", raising=False)
    monkeypatch.delenv("COLTT_ROW_FILTER")
    return out


def _check(gh, Q, efs, monkeypatch, k=10, del_bits=None, id_of=None, sides=("off", "8", "16"), want_survivors=False, gaussian=True):
    """gaussian=False switches off the two expectations that were calibrated for Gaussian rows — that every ef rejects something and that the 8-bit
    shadow rejects no more than the binary16 one — and nothing else.  Returns {(ef, side): counter deltas}."""
    d = gh.dim
    seen = {}
    g = gh.ExportRaw(); rows = gh.FetchRows()
    for ef in efs:
        r = _sides(gh, Q, k, ef, monkeypatch, sides)
        sl, sc, cn, ost, _ = O.csr_search(rows, O.Q_NONE, g["adj0"], g["upper_off"], g["adjU"], d, O.COSINE, g["entry"], g["entry_level"],
                                          Q, k, ef, del_bits=del_bits, threads=4)
        (i0, s0, c0, st0), f0 = r["off"]
        assert (f0["rejected"], f0["f32_rows"], f0["shadow_rows"], f0["launches"]) == (0, 0, 0, 0), "COLTT_ROW_FILTER=0 took a filtered launch"
        for side in sides[1:]:
            (i1, s1, c1, st1), f = r[side]
            for qi in range(len(Q)):
                want = sl[qi, :cn[qi]].astype(np.uint64) if id_of is None else id_of[sl[qi, :cn[qi]]]
                assert_same_results(i1[qi, :c1[qi]], s1[qi, :c1[qi]], want, sc[qi, :cn[qi]], f"filter over {side} bits, q{qi} ef{ef}")
            assert np.array_equal(i0, i1) and np.array_equal(bits(s0), bits(s1)) and np.array_equal(c0, c1), f"ef{ef}: filter over {side} bits != filter off"
            assert st0 == st1, (ef, side, st0, st1)
            assert {k_: st1[k_] for k_ in ost} == ost, (ef, side, st1, ost)
            surv = f["shadow_rows"] - f["rejected"]   # full-set neighbours the shadow could not reject: phase B
            print(f"d{d} ef{ef} k{k} side {side}: shadow rows {f['shadow_rows']} rejected {f['rejected']} survivors {surv} f32 rows {f['f32_rows']} n_dist {st1['n_dist']}")
            seen[(ef, side)] = f
            assert f["launches"] == 1
            if gaussian:
                assert f["rejected"] > 0, f"ef{ef}: the filter over {side} bits rejected nothing"
            assert 0 <= surv <= f["f32_rows"]
            assert 0 < f["rejected"] + f["f32_rows"] <= st1["n_dist"]
            if want_survivors:
                assert surv > 0, "no full-set neighbour reached the exact evaluation: phase B did not run at the boundary"
        if "8" in sides and "16" in sides:
            f8, f16 = r["8"][1], r["16"][1]
            # the same walk meets the same full-set neighbours whichever shadow it reads
            assert f8["shadow_rows"] == f16["shadow_rows"]
            # The 8-bit margin (about 7e-3 of the norm product) contains the binary16 one (1e-3) several times over; a row the 8-bit bound proves and
            # the binary16 bound cannot needs the codes' error q . (x - s c) — spread about e / sqrt(dim) = 3e-4 .. 4e-4 of the norm product on these
            # rows — to fall more than ten of its standard deviations on the favourable side.  One per cent of the rows read is a generous slack.
            if gaussian:
                assert f8["rejected"] <= f16["rejected"] + f16["shadow_rows"] // 100, (f8, f16)
    return seen


def _check_arrays(gh):
    """rows_b / (s, e) per slot / (s, e) per level-0 edge against the quantiser restated on FetchRows()"""
    rows = gh.FetchRows(); g = gh.ExportRaw()
    codes, meta, adjm = gh.FetchShadow8()
    n = rows.shape[0]
    assert codes.shape == rows.shape and meta.shape == (n, 2) and adjm.shape == g["adj0"].shape + (2,)
    for i in range(n):
        c, s, e = quantise(rows[i])
        assert np.array_equal(codes[i], c), f"slot {i}: codes"
        assert meta[i, 0] == s, f"slot {i}: scale {meta[i, 0]} != {s}"
        if np.isfinite(e):
            exact = float(np.linalg.norm(rows[i].astype(np.float64) - np.float64(s) * c.astype(np.float64)))   # f64: off by 1e-13, the stored value is inflated by 2^-20
            assert exact <= float(meta[i, 1]) <= exact * (1 + 2.0 ** -10) + 1e-300, f"slot {i}: error norm {meta[i, 1]} against {exact}"
        else:
            assert meta[i, 1] == np.inf and meta[i, 0] == 0
    adj = g["adj0"]; listed = adj != 0xFFFFFFFF
    want = np.zeros_like(adjm); want[listed] = meta[adj[listed]]
    assert np.array_equal(want.view(np.uint32), adjm.view(np.uint32)), "adj0_m[slot][j] != meta[adj0[slot][j]]"


@pytest.mark.parametrize("nt", ["0", "1"], ids=["default-loads", "non-temporal-twins"])
@pytest.mark.parametrize("d,n", [(256, 5000), (768, 3000), (512, 2000), (1536, 1500), (1024, 2000), (1280, 1500), (2304, 1000)])
def test_three_sides_equal_the_oracle(gpu, monkeypatch, d, n, nt):
    """256-d and 768-d: rows of 2 / 6 shadow lines, the chunk in one burst; 512-d: 4 lines, the stream with two bursts of 2 per row; 1536-d: 12 lines,
    the stream with two bursts of 6 per row; 1024-d: four bursts of 2; 1280-d: five bursts of 2 (an odd count: the other tail of the ping-pong loop);
    2304-d: three bursts of 6 (and three of 12 binary16 lines).  ef 32 / 128 on the LDS-hash kernel, 256 on the HBM-visited one; growth without Reserve"""
    monkeypatch.setenv("COLTT_ROWS_NT", nt)
    X = O.fill_normal(8000 + d, (n, d)); lv = O.levels(8001 + d, n)
    gh = _gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=60), batch=256)
    assert gh.RowFilterStats()["shadow_bits"] == (8, 16)
    Q = O.fill_normal(8002 + d, (48, d))
    _check(gh, Q, (32, 128, 256), monkeypatch)
    _check(gh, Q, (128,), monkeypatch, k=100)
    if nt == "0":
        _check_arrays(gh)


def _clusters(seed, n, d, nq):
    """20 tight clusters (centre + 1e-2 noise per element); queries: members plus noise"""
    rng = np.random.default_rng(seed)
    centres = O.fill_normal(seed, (20, d))
    X = centres[rng.integers(0, 20, n)] + O.fill_normal(seed + 1, (n, d)) * np.float32(1e-2)
    Q = X[rng.choice(n, nq, replace=False)] + O.fill_normal(seed + 2, (nq, d)) * np.float32(1e-2)
    return np.ascontiguousarray(X, np.float32), np.ascontiguousarray(Q, np.float32)


def _heavy_tails(seed, n, d, nq):
    """Gaussian times lognormal, 90 % zeros: a few elements carry the row, the codes of the rest say little"""
    rng = np.random.default_rng(seed)
    def draw(s, m):
        v = O.fill_normal(s, (m, d)) * rng.lognormal(0.0, 2.0, (m, d)).astype(np.float32)
        v[rng.random((m, d)) < 0.9] = 0
        v[np.arange(m), rng.integers(0, d, m)] += np.float32(1.0)   # (never a zero row)
        return np.ascontiguousarray(v, np.float32)
    return draw(seed, n), draw(seed + 1, nq)


@pytest.mark.parametrize("make", [_clusters, _heavy_tails], ids=["clusters", "heavy-tails"])
@pytest.mark.parametrize("d", [256, 1024])
def test_three_sides_equal_the_oracle_on_rows_that_are_not_gaussian(gpu, monkeypatch, d, make):
    """the collections the Gaussian tests say nothing about: rows that all look alike to the codes, and rows the codes say little about.  Parity with
    the oracle and between the sides, counter equality and the counter identities; how MUCH such data lets the filter reject is printed, not asserted,
    except that each collection rejects something at ef 128 (a filter that never fires proves nothing here)"""
    n = 1500
    X, Q = make(8500 + d, n, d, 32)
    lv = O.levels(8501 + d, n)
    gh = _gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=60), batch=256)
    assert gh.RowFilterStats()["shadow_bits"] == (8, 16)
    seen = _check(gh, Q, (32, 128, 256), monkeypatch, gaussian=False)
    for side in ("8", "16"):
        assert seen[(128, side)]["rejected"] > 0, f"d{d} {make.__name__}: the filter over {side} bits rejected nothing at ef 128"


def test_writers_keep_the_8_bit_arrays(gpu, monkeypatch):
    """rows whose norms differ; Removes, single Inserts on top of them; one row the codes say next to nothing about (a 1e30 outlier)"""
    d, n = 256, 1500
    X = O.fill_normal(8100, (n, d)) * np.linspace(0.5, 4.0, n, dtype=np.float32)[:, None]
    X[7, 3] = np.float32(1e30)
    lv = O.levels(8101, n); ids = (np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(10**9))
    gh = _gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=40), batch=64, ids=ids)
    Q = O.fill_normal(8102, (32, d)) * np.float32(3.0)
    _check(gh, Q, (32, 128, 256), monkeypatch, id_of=ids)
    _check_arrays(gh)
    rng = np.random.default_rng(8)
    dead = rng.choice(n, 200, replace=False)
    for i in dead:
        gh.Remove(int(ids[i]))
    db = np.zeros((n + 31) // 32, np.uint32)
    for i in dead:
        db[i >> 5] |= np.uint32(1 << (i & 31))
    _check(gh, Q, (128,), monkeypatch, del_bits=db, id_of=ids)
    _check_arrays(gh)
    Y = O.fill_normal(8103, (30, d)) * np.linspace(0.1, 9.0, 30, dtype=np.float32)[:, None]; ly = O.levels(8104, 30)
    for j in range(30):
        gh.Insert(5 + j, Y[j], int(ly[j]))
    db2 = np.zeros((n + 30 + 31) // 32, np.uint32); db2[:len(db)] = db
    _check(gh, Q, (32, 128), monkeypatch, del_bits=db2, id_of=np.concatenate([ids, np.uint64(5) + np.arange(30, dtype=np.uint64)]))
    _check_arrays(gh)


def test_commit_load_and_bulk_load_keep_the_8_bit_arrays(gpu, monkeypatch):
    d, n = 256, 1500
    X = O.fill_normal(8200, (n, d)) * np.linspace(0.25, 3.0, n, dtype=np.float32)[:, None]; lv = O.levels(8201, n)
    g1 = _gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=40), batch=64)
    g2 = gpu.Hnsw(d, O.COSINE)
    assert g2.Load(g1.Commit()) == n
    Q = O.fill_normal(8202, (32, d))
    _check(g2, Q, (32, 128, 256), monkeypatch, id_of=g2.Export()["ids"])
    _check_arrays(g2)
    # a second Load into the same (already allocated) index, fewer vertices: every slot's arrays are rewritten with its row
    g3 = _gpu_build(gpu, X[:700] * np.float32(-1.0), lv[:700], gpu.HnswCfg.default(ef_construction=40), batch=64)
    assert g2.Load(g3.Commit()) == 700
    _check(g2, Q, (128,), monkeypatch, id_of=g2.Export()["ids"])
    _check_arrays(g2)
    oh = O.Hnsw(d, O.COSINE); ids = np.arange(600, dtype=np.uint64); oh.insert_many(ids, X[:600], lv[:600])
    g4 = gpu.Hnsw(d, O.COSINE); g4.BulkLoad(oh.export(with_vectors=False), X[:600])
    _check(g4, Q, (32, 128), monkeypatch, id_of=g4.Export()["ids"])
    _check_arrays(g4)


def test_ties_and_near_ties_with_lower_bound(gpu, monkeypatch):
    """the construction of test_gpu_row_filter.py: every base vector stored six times — exact duplicates and copies that differ in one low bit of one or
    two elements — queried by those vectors and small perturbations of them.  The 8-bit shadow cannot tell such rows from the set's worst member: they
    reach the exact f32 evaluation, and admissions at d == lowerBound and one ulp either side of it come out as the oracle's"""
    d, nb, copies = 256, 400, 6
    rng = np.random.default_rng(99)
    base = O.fill_normal(8300, (nb, d))
    base /= np.linalg.norm(base, axis=1, keepdims=True).astype(np.float32)
    X = np.repeat(base, copies, axis=0)
    for i in range(len(X)):
        c = i % copies
        if c % 3 == 1:
            j = int(rng.integers(0, d)); X[i, j] = np.nextafter(X[i, j], np.float32(4), dtype=np.float32)
        elif c % 3 == 2:
            for j in rng.integers(0, d, 2):
                X[i, j] = np.nextafter(X[i, j], np.float32(-4), dtype=np.float32)
    X = X[rng.permutation(len(X))]
    lv = O.levels(8301, len(X))
    gh = _gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=80), batch=64)
    Q = np.concatenate([base[:16], base[16:32] + O.fill_normal(8302, (16, d)) * np.float32(1e-4), O.fill_normal(8303, (16, d))])
    _check(gh, Q, (32, 64, 128, 256), monkeypatch, k=20, sides=("off", "8"), want_survivors=True)


def test_the_kind_an_index_does_not_keep_is_served_by_the_one_it_does(gpu, monkeypatch):
    d, n = 256, 1500
    X = O.fill_normal(8400, (n, d)); lv = O.levels(8401, n)
    Q = O.fill_normal(8402, (16, d))
    cfg = gpu.HnswCfg.default(ef_construction=40)
    monkeypatch.setenv("COLTT_ROW_SHADOW_BITS", "16")
    g16 = _gpu_build(gpu, X, lv, cfg)
    assert g16.RowFilterStats()["shadow"] and g16.RowFilterStats()["shadow_bits"] == (16,)
    with pytest.raises(Exception):
        g16.FetchShadow8()
    _check(g16, Q, (32, 128, 256), monkeypatch, sides=("off", "8"))    # asks for 8, reads binary16: launches still happen, answers are the oracle's
    monkeypatch.setenv("COLTT_ROW_SHADOW_BITS", "8")
    g8 = _gpu_build(gpu, X, lv, cfg)
    assert g8.RowFilterStats()["shadow"] and g8.RowFilterStats()["shadow_bits"] == (8,)
    _check(g8, Q, (32, 128, 256), monkeypatch, sides=("off", "16"))    # asks for 16, reads the codes
    _check_arrays(g8)
    monkeypatch.delenv("COLTT_ROW_SHADOW_BITS")                        # the default: the 8-bit shadow alone
    gd = _gpu_build(gpu, X, lv, cfg)
    assert gd.RowFilterStats()["shadow_bits"] == (8,)
    monkeypatch.setenv("COLTT_ROW_SHADOW", "0")
    monkeypatch.setenv("COLTT_ROW_SHADOW_BITS", "both")
    g0 = _gpu_build(gpu, X, lv, cfg)
    st = g0.RowFilterStats()
    assert not st["shadow"] and st["shadow_bits"] == ()
    monkeypatch.setenv("COLTT_ROW_FILTER", "1")
    g0.Search(Q, 10, ef=128)
    assert g0.RowFilterStats()["launches"] == 0
