"""CPU suite: the oracle against (1) the reference's own C++ SIMD kernels built from /root/reference when present
(oracle/_ref), (2) independent restatements (numpy float16, Python FNV / container-heap), (3) the committed golden
fixtures.  No GPU needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

GOLD = os.path.join(os.path.dirname(__file__), "golden")
sys.path.insert(0, GOLD)
import make_golden as MG  # noqa: E402


def test_distance_orders_equal_reference_sources():
    """the oracle's AVX / SSE orders against the reference's own avx.cpp / sse.cpp: their outputs are stored in golden/ref_simd.npz
    (make_golden.py) and, where oracle/_ref is built, also taken live"""
    g = np.load(os.path.join(GOLD, "ref_simd.npz"))
    pairs = MG.ref_dist_pairs()
    assert MG.pairs_crc(pairs) == int(g["dist_crc"][0]), "the seeded inputs are not the ones ref_simd.npz was made from"
    got = MG.ref_dist_bits(MG.oracle_dist, pairs)
    bad = np.argwhere(got != g["dist"])
    assert len(bad) == 0, bad[:10]
    r = O.ref()
    if r is not None:
        assert np.array_equal(MG.ref_dist_bits(MG.ref_dist(r), pairs), g["dist"])


def test_manhattan_equals_reference_sources_and_native_order():
    """Manhattan.Distance (pkg/distance/space.go:77-79): the oracle against the reference's own avx.cpp / sse.cpp (vector part: sqrt of the
    rounded square, NOT |d|; scalar tail: abs) incl. magnitudes where the two differ — stored in golden/ref_simd.npz and, where oracle/_ref
    is built, also taken live — and the native order against a numpy loop."""
    g = np.load(os.path.join(GOLD, "ref_simd.npz"))
    pairs = MG.ref_manhattan_pairs()
    assert MG.pairs_crc(pairs) == int(g["manhattan_crc"][0]), "the seeded inputs are not the ones ref_simd.npz was made from"
    for t, (a, b) in enumerate(pairs):
        nat = np.float32(0)
        with np.errstate(over="ignore"):
            for i in range(a.size):
                nat = np.float32(nat + np.float32(abs(np.float32(a[i] - b[i]))))
        assert bits(O.manhattan(a, b, O.ORDER_NATIVE)) == bits(nat)
        for j, order in enumerate((O.ORDER_AVX, O.ORDER_SSE)):
            assert O.manhattan(a, b, order).view(np.uint32) == g["manhattan"][t, j], (t, a.size, order)
    r = O.ref()
    if r is not None:
        assert np.array_equal(MG.ref_manhattan_bits(r, pairs), g["manhattan"])
    x = np.array([3e-30] * 8 + [3e-30], np.float32); z = np.zeros(9, np.float32)
    assert O.manhattan(x, z, O.ORDER_AVX) == np.float32(3e-30) and O.manhattan(x, z, O.ORDER_NATIVE) > np.float32(2.6e-29)   # the vector lanes lost their 8 terms


def test_codecs_against_ieee_binary16():
    codes = np.arange(65536, dtype=np.uint16)
    dec = O.f16_decode(codes); ref = codes.view(np.float16).astype(np.float32)
    m = ~np.isnan(ref)
    assert np.array_equal(bits(dec[m]), bits(ref[m])) and np.isnan(dec[~m]).all()
    rng = np.random.default_rng(2)
    x = (rng.standard_normal(300000) * np.exp(rng.uniform(-25, 11, 300000))).astype(np.float32)
    with np.errstate(over="ignore"):
        assert np.array_equal(O.f16_encode(x), x.astype(np.float16).view(np.uint16))
    # encode(decode(c)) == c for every non-NaN code: what lets a binary16 index travel through the reference's f32 stream (coltt_hnsw_commit)
    assert np.array_equal(O.f16_encode(dec[m]), codes[m])
    f8v = O.f8_decode(np.arange(256, dtype=np.uint8))
    assert not np.array_equal(bits(O.f8_decode(O.f8_encode(f8v))), bits(f8v))           # ... and why an "f8" index cannot
    # "bf16" is binary16 in the reference, "f8" decodes to 8 values (SURVEY.md §0 findings 2-3)
    lut = O.f8_decode(np.arange(256, dtype=np.uint8)).view(np.uint32)
    assert sorted(set(lut.tolist())) == [0, 0x8000, 0x33800000, 0x33808000, 0x34000000, 0x34008000, 0x34400000, 0x34408000]


def test_f8_encode_is_low_byte_of_f16_for_finite_non_overflow():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 8, 100000))).astype(np.float32)
    x = x[np.abs(x) < 60000]
    assert np.array_equal(O.f8_encode(x), (O.f16_encode(x) & 0xFF).astype(np.uint8))


def test_fnv_shard():
    def fnv(x, c):
        h = 14695981039346656037
        for i in range(8):
            h ^= (x >> (8 * i)) & 0xFF; h = (h * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h % c
    for i in range(2000):
        x = (i * 0x9E3779B97F4A7C15 + 77) & 0xFFFFFFFFFFFFFFFF
        assert O.shard_vertex(x, 16) == fnv(x, 16)


def test_go_heap_semantics():
    """container/heap restated independently in Python (up/down as in go1.23 heap.go)."""
    def run(is_max, pr, ops):
        less = (lambda a, b: pr[a] > pr[b]) if is_max else (lambda a, b: pr[a] < pr[b])
        h, pops = [], []
        def up(j):
            while True:
                i = (j - 1) // 2 if j > 0 else 0
                if i == j or not less(h[j], h[i]): break
                h[i], h[j] = h[j], h[i]; j = i
        def down(i0, n):
            i = i0
            while True:
                j1 = 2 * i + 1
                if j1 >= n: break
                j = j1
                if j1 + 1 < n and less(h[j1 + 1], h[j1]): j = j1 + 1
                if not less(h[j], h[i]): break
                h[i], h[j] = h[j], h[i]; i = j
        for o in ops:
            if o >= 0: h.append(o); up(len(h) - 1)
            elif h:
                n = len(h) - 1; h[0], h[n] = h[n], h[0]; down(0, n); pops.append(h.pop())
        return pops, h
    rng = np.random.default_rng(9)
    for trial in range(50):
        pr = rng.integers(0, 6, 40).astype(np.float32)  # many ties
        ops = np.array([i if rng.random() < 0.7 else -1 for i in range(40)], np.int32)
        for mx in (0, 1):
            p, f = O.heap_trace(mx, pr, ops); p2, f2 = run(mx, pr, list(ops))
            assert list(p) == p2 and list(f) == f2


def test_edge_queue_keeps_farthest_and_modes_agree():
    """edge.PriorityQueue is a min-heap that pops the minimum: K LARGEST distances survive (finding 1)."""
    n, d = 500, 24
    X = O.fill_normal(3, (n, d)); ids = np.arange(n, dtype=np.uint64)
    f = O.Flat(d, O.L2); f.upsert(ids, X)
    q = O.fill_normal(4, d)
    alld = O.dist_rows(O.L2, q, X)
    i0, s0 = f.search(q, 7, nearest=False, mode=0)
    assert np.array_equal(np.sort(alld)[-7:], s0)               # farthest 7, ascending
    for mode in (1, 2):
        i, s = f.search(q, 7, nearest=False, mode=mode)
        assert np.array_equal(i, i0) and np.array_equal(bits(s), bits(s0))
    i1, s1 = f.search(q, 7, nearest=True, mode=2)
    assert np.array_equal(np.sort(alld)[:7], s1)


def test_hnsw_literal_equals_canonical_and_batched_1():
    n, d = 800, 40
    X = O.fill_normal(11, (n, d)); lv = O.levels(12, n); ids = np.arange(n, dtype=np.uint64)
    a = O.Hnsw(d, O.COSINE); a.insert_many(ids, X, lv)
    b = O.Hnsw(d, O.COSINE, canonical_build=True); b.insert_many(ids, X, lv)
    c = O.Hnsw(d, O.COSINE); c.insert_batched(ids, X, lv, 1)
    assert a.graph_hash() == b.graph_hash() == c.graph_hash()
    e = O.Hnsw(d, O.COSINE, O.default_cfg(algo=1)); e.insert_many(ids, X, lv)   # Heuristic(extend=false) == Simple
    assert e.graph_hash() == a.graph_hash()
    for q in O.fill_normal(13, (25, d)):
        r0 = a.search(q, 10, mode=0, ef=50, with_stats=True); r1 = a.search(q, 10, mode=1, ef=50, with_stats=True)
        assert np.array_equal(r0[0], r1[0]) and np.array_equal(bits(r0[1]), bits(r1[1])) and r0[2] == r1[2]
    assert a.insert(5, X[5], 0) == -2 and a.remove(10**6) == -3
    # export -> import round trip (the invariant hnsw_commit_test.go:127-181 asserts for Commit/Load)
    g = a.export(); z = O.Hnsw(d, O.COSINE); z.load(g)
    assert z.graph_hash() == a.graph_hash() and len(z) == len(a)


def test_golden_kernels():
    g = np.load(os.path.join(GOLD, "kernels.npz"))
    for d in MG.DIST_DIMS:
        a = O.fill_normal(100 + d, (8, d)); b = O.fill_normal(200 + d, (8, d))
        for mname, f in (("cos", O.cosine), ("l2", O.l2)):
            for order in (0, 1, 2):
                got = np.array([f(a[i], b[i], order) for i in range(8)], np.float32).view(np.uint32)
                assert np.array_equal(got, g[f"dist_{mname}_{order}_{d}"]), (mname, order, d)
        assert np.array_equal(O.normalize(a).view(np.uint32), g[f"norm_{d}"])
        assert np.array_equal(np.array([O.pq_dot(a[i], b[i]) for i in range(8)], np.float32).view(np.uint32), g[f"pqdot_{d}"])
        assert np.array_equal(np.array([O.pq_l2sq(a[i], b[i]) for i in range(8)], np.float32).view(np.uint32), g[f"pql2_{d}"])
    x = g["enc_in"].view(np.float32)
    assert np.array_equal(O.f16_encode(x), g["f16_encode"]) and np.array_equal(O.f8_encode(x), g["f8_encode"])
    assert np.array_equal(O.f8_decode(np.arange(256, dtype=np.uint8)).view(np.uint32), g["f8_lut"])
    assert MG.fnv64(O.f16_decode(np.arange(65536, dtype=np.uint16)).tobytes()) == int(g["f16_decode_hash"][0])
    assert np.array_equal(np.array([O.pq_hamming(g["bit_q"], r) for r in g["bit_rows"]], np.float32), g["hamming"])
    for mx in (0, 1):
        p, f = O.heap_trace(mx, g["heap_prios"], g["heap_ops"])
        assert np.array_equal(p, g[f"heap_pops_{mx}"]) and np.array_equal(f, g[f"heap_final_{mx}"])


def test_golden_flat_and_hnsw():
    g = np.load(os.path.join(GOLD, "flat_2048x128.npz"))
    n, d = 2048, 128
    X = O.fill_normal(1, (n, d)); Q = O.fill_normal(99, (16, d))
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(1000003)) % np.uint64(1 << 40)
    for metric, quant in ((0, 0), (1, 1), (0, 2), (1, 3)):
        f = O.Flat(d, metric, quant); f.upsert(ids, X)
        for k, nearest in ((10, 0), (100, 1)):
            for qi in range(16):
                i, s = f.search(Q[qi], k, bool(nearest), 2)
                assert np.array_equal(i, g[f"ids_{metric}_{quant}_{k}_{nearest}"][qi])
                assert np.array_equal(s.view(np.uint32), g[f"sc_{metric}_{quant}_{k}_{nearest}"][qi])
    h = np.load(os.path.join(GOLD, "hnsw.npz"))
    n, d = 1000, 128
    X = O.fill_normal(40 + d, (n, d)); lv = O.levels(41 + d, n); ids = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(11)
    x = O.Hnsw(d, O.COSINE); x.insert_many(ids, X, lv)
    assert x.graph_hash() == int(h["1000x128_cos_graph_hash"][0])
    Q = O.fill_normal(123, (40, d))
    for qi in range(40):
        i, s, c = x.search(Q[qi], 10, mode=1, ef=128, with_stats=True)
        assert np.array_equal(i, h["1000x128_cos_ids_128"][qi]) and np.array_equal(s.view(np.uint32), h["1000x128_cos_sc_128"][qi])
        assert (c["n_dist"], c["n_exp"], c["n_hops"]) == tuple(int(v) for v in h["1000x128_cos_stats_128"][qi])
    rng = np.random.default_rng(40 + d)
    for i in rng.choice(n, 200, replace=False): x.remove(ids[i])
    assert x.graph_hash() == int(h["1000x128_cos_graph_hash_removed"][0])


# ------------------------------------------------------------------ invariants the reference's own tests assert
def test_hnsw_commit_load_round_trip_structural_equality():
    """hnsw_commit_test.go:32-102 — Commit -> Load gives a structurally equal index (config, vertices, edges, entrypoint):
    restated on the oracle's big-endian stream (hnsw_commit.go:69-278), with removals in the graph, and the loaded index
    answers searches identically."""
    n, d = 600, 20
    X = O.fill_normal(21, (n, d)); lv = O.levels(22, n); ids = np.arange(n, dtype=np.uint64) * np.uint64(5) + np.uint64(9)
    for metric in (O.COSINE, O.L2):
        a = O.Hnsw(d, metric, O.default_cfg(efConstruction=48, ef=30)); a.insert_many(ids, X, lv)
        for r in (ids[7], ids[100], ids[599]):
            assert a.remove(int(r)) == 0
        for header in (True, False):
            blob = a.commit(header=header)
            b = O.Hnsw(d, metric, O.default_cfg(efConstruction=48, ef=30))
            assert b.load_stream(blob, header=header) == 0
            assert len(b) == len(a) == n - 3
            ga, gb = a.export(), b.export()
            # tombstoned vertices are not written (hnsw_commit.go skips deleted), and Load appends in stream (shard) order:
            # compare the live vertices per id, not per slot
            la, lb = ga["deleted"] == 0, gb["deleted"] == 0
            assert lb.all()
            ia, ib = np.argsort(ga["ids"][la]), np.argsort(gb["ids"])
            assert np.array_equal(ga["ids"][la][ia], gb["ids"][ib]) and np.array_equal(ga["levels"][la][ia], gb["levels"][ib])
            assert np.array_equal(bits(ga["vectors"][la][ia]), bits(gb["vectors"][ib]))
            assert ga["ids"][a.entry] == gb["ids"][b.entry]
            c = O.Hnsw(d, metric); assert c.load_stream(b.commit(header=True), header=True) == 0   # Commit(Load(.)) is a fixed point
            assert c.graph_hash() == b.graph_hash() and c.commit(header=header) == b.commit(header=header)
            for q in O.fill_normal(23, (12, d)):
                ra, rb = a.search(q, 8, mode=1), b.search(q, 8, mode=1)
                assert np.array_equal(ra[0], rb[0]) and np.array_equal(bits(ra[1]), bits(rb[1]))


@pytest.mark.parametrize("quant", [O.Q_NONE, O.Q_F16, O.Q_F8, O.Q_BF16])
def test_flat_vertex_stream_round_trip(quant):
    """SaveVertex -> LoadVertex (none_vectorstore.go:308-516, f16_vectorstore.go:317-532): same ids, same stored bits, same answers."""
    n, d = 300, 36
    X = O.fill_normal(31, (n, d)); ids = (np.arange(n, dtype=np.uint64) * np.uint64(7919) + np.uint64(13)) % np.uint64(1 << 33)
    a = O.Flat(d, O.COSINE, quant); a.upsert(ids, X); a.remove(ids[5:9])
    blob = a.save_vertex()
    b = O.Flat(d, O.COSINE, quant); b.load_vertex(blob)
    assert len(b) == len(a) == n - 4
    for i in (0, 4, 9, n - 1):
        assert np.array_equal(a.get(ids[i]).view(np.uint8), b.get(ids[i]).view(np.uint8))
    for q in O.fill_normal(32, (6, d)):
        for nearest in (False, True):
            ra, rb = a.search(q, 10, nearest=nearest, mode=2), b.search(q, 10, nearest=nearest, mode=2)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(bits(ra[1]), bits(rb[1]))
    assert b.save_vertex() == blob


def test_random_level_formula():
    """Hnsw.RandomLevel = gomath.Floor(-gomath.Log(u) * levelMultiplier) (hnsw.go:280-282, gomath/math.go:52-62): float32 log
    (through float64), float32 multiply, floor through float64 — against an independent numpy restatement."""
    mult = np.float32(1.0) / np.float32(np.log(np.float64(np.float32(16))))
    rng = np.random.default_rng(3)
    us = np.concatenate([rng.random(5000, dtype=np.float32), np.float32([1e-38, 1e-20, 0.0625, 0.5, 0.99999994])])
    us = us[(us > 0) & (us < 1)]
    for u in us:
        want = int(np.floor(np.float64(np.float32(-np.float32(np.log(np.float64(u)))) * mult)))
        assert O.level_from_u(float(u), float(mult)) == want, u
    lv = O.levels(7, 200000)   # the counter-stream draw used by tests/bench: geometric-like, P(level >= 1) = 1/16
    assert lv.min() == 0 and 0.055 < (lv >= 1).mean() < 0.07 and lv.max() < 12


def test_cflat_weighted_multi_vector_score():
    """experimental MultiVertexSearch (multi_vector_vertex.go:85-137): score = sum over included fields of
    scoreHelper(distance) * ratio / 100, scoreHelper(cos) = ((2 - d) / 2) * 100 (experimental_helper.go:134-139), accumulated
    in field order in f32; the K LARGEST scores are kept, descending."""
    n, d, nf = 200, 16, 3
    X = O.fill_normal(51, (n, nf, d)); ids = np.arange(n, dtype=np.uint64) + np.uint64(1000)
    c = O.CFlat(d, nf, O.COSINE); c.upsert(ids, X)
    q = O.fill_normal(52, (nf, d)); ratios = np.array([50, 30, 20], np.uint32); include = np.array([1, 0, 1], np.uint8)
    got_i, got_s = c.search(q, ratios, include, 7)
    qn = O.normalize(q)
    sc = np.zeros(n, np.float32)
    for f in range(nf):
        if not include[f]:
            continue
        rows = O.normalize(X[:, f, :])
        dist = O.dist_rows(O.COSINE, qn[f], rows)
        term = ((np.float32(2) - dist) / np.float32(2)) * np.float32(100)
        sc = (sc + term * (np.float32(ratios[f]) / np.float32(100))).astype(np.float32)
    order = np.lexsort((ids, -sc.astype(np.float64)))[:7]
    assert np.array_equal(np.sort(got_s)[::-1], got_s)
    assert np.array_equal(bits(got_s), bits(sc[order]))
    assert set(got_i.tolist()) == set(ids[order].tolist())
    c.remove(ids[order[:2]])
    i2, s2 = c.search(q, ratios, include, 7)
    assert not (set(i2.tolist()) & set(ids[order[:2]].tolist()))


def test_hnsw_remove_semantics():
    """Hnsw.Remove (hnsw.go:191-241): the vertex disappears from answers and from its neighbours' rows; removing twice is
    ItemNotFoundError; Len counts live vertices; searching after removing every answer still returns k live ids."""
    n, d = 400, 12
    X = O.fill_normal(61, (n, d)); lv = O.levels(62, n); ids = np.arange(n, dtype=np.uint64)
    h = O.Hnsw(d, O.L2); h.insert_many(ids, X, lv)
    q = O.fill_normal(63, d)
    i0, s0 = h.search(q, 5, mode=1, ef=40)
    removed = []
    for v in (int(x) for x in i0[:3]):
        if h.remove(v) == 0:           # (removing the entrypoint's last neighbour can be refused; not the case here)
            removed.append(v)
            assert h.remove(v) == -3   # ItemNotFoundError the second time
    assert len(removed) == 3
    assert len(h) == n - len(removed)
    i1, s1 = h.search(q, 5, mode=1, ef=40)
    assert len(i1) == 5 and not (set(i1.tolist()) & set(removed))
    g = h.export()
    assert int(g["deleted"].sum()) == len(removed)
    # Remove unlinks the vertex from the rows of ITS OWN neighbours (hnsw.go:234-236); vertices that merely pointed at it keep
    # the stale edge, which searchLevel skips through the tombstone (hnsw_vertex.go:70-76).
    first_row = np.concatenate([[0], np.cumsum(g["levels"].astype(np.int64) + 1)])
    def row(slot, level):
        r = first_row[slot] + level
        return g["nbr"][g["row_offsets"][r]:g["row_offsets"][r + 1]]
    for v in np.nonzero(g["deleted"])[0]:
        for level in range(int(g["levels"][v]) + 1):
            for u in row(v, level):
                if u >= 0 and not g["deleted"][u] and int(g["levels"][u]) >= level:
                    assert v not in row(int(u), level).tolist(), (v, u, level)


def _csr_from_export(g, w0, wu):
    """export() dict -> the padded arrays the GPU keeps in HBM (adj0 [n][w0], upper_off [n], adjU [rows][wu])."""
    n = len(g["levels"])
    first_row = np.concatenate([[0], np.cumsum(g["levels"].astype(np.int64) + 1)])
    adj0 = np.full((n, w0), 0xFFFFFFFF, np.uint32)
    upper_off = np.full(n, 0xFFFFFFFF, np.uint32)
    n_upper = int(g["levels"].sum())
    adjU = np.full((max(n_upper, 1), wu), 0xFFFFFFFF, np.uint32)
    u = 0
    for s in range(n):
        for l in range(int(g["levels"][s]) + 1):
            r = first_row[s] + l
            row = g["nbr"][g["row_offsets"][r]:g["row_offsets"][r + 1]].astype(np.uint32)
            if l == 0:
                adj0[s, :len(row)] = row
            else:
                if l == 1:
                    upper_off[s] = u
                adjU[u, :len(row)] = row
                u += 1
    return adj0, upper_off, adjU


@pytest.mark.parametrize("metric,quant", [(O.COSINE, O.Q_NONE), (O.L2, O.Q_NONE), (O.L2, O.Q_F16)])
def test_csr_search_equals_canonical_search(metric, quant):
    """bench.py's cpu_baseline leg walks the arrays copied out of HBM with orc_csr_search; here the same function over arrays
    rebuilt from the oracle's own export equals Hnsw.search (canonical form): slots, score bits and the traversal counters."""
    n, d, k, ef = 1200, 24, 10, 48
    X = O.fill_normal(71, (n, d)); lv = O.levels(72, n); ids = np.arange(n, dtype=np.uint64)
    Xs = O.f16_decode(O.lower(quant, X)) if quant == O.Q_F16 else X       # what a quantised index stores, decoded
    h = O.Hnsw(d, metric); h.insert_many(ids, Xs, lv)
    for v in (3, 77, 500):
        assert h.remove(v) == 0
    g = h.export()
    adj0, upper_off, adjU = _csr_from_export(g, 32, 16)
    del_bits = np.zeros((n + 31) // 32, np.uint32)
    for s in np.nonzero(g["deleted"])[0]:
        del_bits[s >> 5] |= np.uint32(1) << np.uint32(s & 31)
    rows = np.ascontiguousarray(O.lower(quant, X)) if quant == O.Q_F16 else np.ascontiguousarray(g["vectors"], np.float32)
    Q = O.fill_normal(73, (30, d))
    sl = np.empty((len(Q), k), np.int32); sc = np.empty((len(Q), k), np.float32); cn = np.empty(len(Q), np.int32); st = (C.c_uint64 * 3)()
    L = O.lib()
    L.orc_csr_search(rows.ctypes.data_as(C.c_void_p), int(quant), adj0.ctypes.data_as(C.c_void_p), upper_off.ctypes.data_as(C.c_void_p),
                     adjU.ctypes.data_as(C.c_void_p), del_bits.ctypes.data_as(C.c_void_p), C.c_uint32(32), C.c_uint32(16), C.c_uint32(d),
                     int(metric), 0, C.c_int32(h.entry), C.c_int32(int(g["levels"][h.entry])), Q.ctypes.data_as(C.c_void_p),
                     C.c_size_t(len(Q)), k, ef, sl.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), cn.ctypes.data_as(C.c_void_p), st)
    tot = np.zeros(3, np.int64)
    Qs = O.f16_decode(O.lower(quant, Q)) if quant == O.Q_F16 else Q       # the quantised stores lower the query too
    for qi in range(len(Q)):
        wi, ws, wst = h.search(Qs[qi], k, mode=1, ef=ef, with_stats=True)
        assert cn[qi] == len(wi)
        assert np.array_equal(g["ids"][sl[qi, :cn[qi]]], wi) and np.array_equal(bits(sc[qi, :cn[qi]]), bits(ws)), qi
        tot += np.array([wst["n_dist"], wst["n_exp"], wst["n_hops"]], np.int64)
    assert [int(st[0]), int(st[1]), int(st[2])] == tot.tolist()


def test_cpu_baseline_mt_drivers_equal_serial_oracle():
    """bench.py's cpu_baseline runs native pinned threads inside the oracle (orc_csr_search_mt / orc_flat_scan_mt) over a
    NUMA-interleaved copy of the corpus.  Threading must not change a bit: same slots, score bits and counters as the serial
    calls; the FLAT driver (both `highCpu` split and one-query-per-thread, both decode shapes and the reference's memory shape — 16
    maps of per-vector allocations) equals Flat.search's canonical mode."""
    n, d, k, ef = 1500, 40, 10, 64
    X = O.fill_normal(171, (n, d)); lv = O.levels(172, n); ids = np.arange(n, dtype=np.uint64)
    for metric, quant in ((O.COSINE, O.Q_NONE), (O.COSINE, O.Q_BF16), (O.L2, O.Q_F8)):
        h = O.Hnsw(d, O.L2 if quant != O.Q_NONE else metric); h.insert_many(ids, X, lv)   # any valid graph will do
        g = h.export()
        adj0, upper_off, adjU = _csr_from_export(g, 32, 16)
        f = O.Flat(d, metric, quant); f.upsert(ids, X)
        stored = np.stack([f.get(i) for i in ids])                                         # Normalize + Lower applied
        na = O.NumaArray(stored.shape, stored.dtype, threads=4); na.a[:] = stored
        Q = O.fill_normal(173, (24, d))
        ent, el = h.entry, int(g["levels"][h.entry])
        s1 = O.csr_search(na.a, quant, adj0, upper_off, adjU, d, metric, ent, el, Q, k, ef, threads=1)
        s4 = O.csr_search(na.a, quant, adj0, upper_off, adjU, d, metric, ent, el, Q, k, ef, threads=5)
        assert np.array_equal(s1[0], s4[0]) and np.array_equal(bits(s1[1]), bits(s4[1])) and np.array_equal(s1[2], s4[2]) and s1[3] == s4[3]
        for nearest in (True, False):
            for shape, split, th in ((0, 1, 3), (1, 1, 4), (0, 16, 16), (1, 4, 4), (2, 1, 1), (2, 1, 3), (2, 16, 16)):   # 2 = reference memory shape
                sl, sc, cn, _ = O.flat_scan(na.a, quant, d, metric, Q, k, nearest=nearest, shape=shape, split=split, threads=th)
                for qi in range(len(Q)):
                    wi, ws = f.search(Q[qi], k, nearest=nearest, mode=2)
                    assert np.array_equal(sl[qi], wi) and np.array_equal(bits(sc[qi]), bits(ws)), (metric, quant, nearest, shape, split, qi)
        na.close()


def test_canonical_form_equals_literal_go_heaps_on_random_configurations():
    """The foundation of every HNSW parity claim: the closed form the GPU runs (sorted result set, ascending-slot neighbour
    order, stale lowerBound, first ef-len0 admitted unconditionally) is the SAME function as the literal restatement with Go's
    container/heap and per-candidate lowerBound sampling (hnsw.go:345-389) — checked over random sizes, dims, M, ef, k,
    metrics, algorithms and removals: graph hash of the builds, answers, score bits and the n_dist/n_exp/n_hops counters."""
    rng = np.random.default_rng(20250328)
    for trial in range(120):
        n = int(rng.integers(30, 420)); d = int(rng.integers(2, 48)); m = int(rng.choice([4, 6, 8, 16]))
        metric = int(rng.integers(0, 2)); efc = int(rng.integers(max(m, 8), 96)); algo = int(rng.integers(0, 2))
        X = O.fill_normal(1000 + trial, (n, d))
        mult = np.float32(1.0) / np.float32(np.log(np.float64(np.float32(m))))
        lv = np.array([O.level(2000 + trial, i, float(mult)) for i in range(n)], np.int32)
        ids = rng.permutation(n).astype(np.uint64) * np.uint64(17) + np.uint64(3)
        cfg = dict(m=m, efConstruction=efc, algo=algo)
        a = O.Hnsw(d, metric, O.default_cfg(**cfg)); a.insert_many(ids, X, lv)                          # literal
        b = O.Hnsw(d, metric, O.default_cfg(**cfg), canonical_build=True); b.insert_many(ids, X, lv)    # closed form
        assert a.graph_hash() == b.graph_hash(), (trial, n, d, m, metric, efc, algo)
        for v in rng.choice(ids, size=int(rng.integers(0, max(1, n // 6))), replace=False):
            ra, rb = a.remove(int(v)), b.remove(int(v))
            assert ra == rb
        assert a.graph_hash() == b.graph_hash(), ("after removals", trial)
        for q in O.fill_normal(3000 + trial, (6, d)):
            k = int(rng.integers(1, 25)); ef = int(rng.integers(1, 90))
            r0 = a.search(q, k, mode=0, ef=ef, with_stats=True); r1 = a.search(q, k, mode=1, ef=ef, with_stats=True)
            assert np.array_equal(r0[0], r1[0]) and np.array_equal(bits(r0[1]), bits(r1[1])) and r0[2] == r1[2], (trial, k, ef)


def test_flat_canonical_equals_literal_queue_on_random_configurations():
    """FLAT: the canonical select the GPU implements (mode 2) == the literal edge.PriorityQueue run (mode 0: per-shard Go map
    walk + container/heap pop-min; mode 1: the 16-goroutine highCpu split with local queues merged) over random sizes, dims,
    k, metrics and the four quantisations — ids, order and score bits."""
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(1, 700)); d = int(rng.integers(1, 72)); k = int(rng.integers(1, 48))
        metric = int(rng.integers(0, 2)); quant = int(rng.integers(0, 4))
        X = O.fill_normal(5000 + trial, (n, d)); ids = rng.permutation(4 * n)[:n].astype(np.uint64) + np.uint64(1)
        f = O.Flat(d, metric, quant); f.upsert(ids, X)
        if n > 4:
            f.remove(ids[: n // 5])
        for q in O.fill_normal(6000 + trial, (3, d)):
            ref = f.search(q, k, nearest=False, mode=2)
            for mode in (0, 1):
                got = f.search(q, k, nearest=False, mode=mode)
                assert np.array_equal(got[0], ref[0]) and np.array_equal(bits(got[1]), bits(ref[1])), (trial, n, d, k, metric, quant, mode)
            near = f.search(q, k, nearest=True, mode=2)
            assert len(near[0]) == min(k, len(f)) and np.all(np.diff(near[1]) >= 0)


@pytest.mark.parametrize("dim", [128, 384, 768])
def test_the_reference_codec_loss_property(dim):
    """pkg/compresshelper/compresshelper_test.go:38-412 (TestF16/BF16/F8Losses{128,384,768,1536}dim): for rand.Float32() vectors,
    |((d + 1) / 2 * 100)(raw pair) - (the same)(encode -> decode of both)| <= 1 with d = Cosine.Distance.  Restated over the oracle's
    codecs and AVX-order cosine: binary16 ("f16" and the reference's "bf16") holds it with four decimal places to spare.  The reference's
    f8 case can never fail there (its failure branch is `assert.Error(t, errors.New(...))`, which passes); restated honestly it does not
    hold — that codec keeps the low byte of the binary16 code (SURVEY §0 finding 3), so decoded vectors are near-zero noise."""
    rng = np.random.default_rng(1000 + dim)
    worst16 = 0.0; f8_fail = 0; pairs = 400
    for _ in range(pairs):
        a = rng.random(dim, dtype=np.float32); b = rng.random(dim, dtype=np.float32)
        raw = (float(O.cosine(a, b)) + 1) / 2 * 100
        a16 = O.f16_decode(O.f16_encode(a)); b16 = O.f16_decode(O.f16_encode(b))
        worst16 = max(worst16, abs(raw - (float(O.cosine(a16, b16)) + 1) / 2 * 100))
        a8 = O.f8_decode(O.f8_encode(a)); b8 = O.f8_decode(O.f8_encode(b))
        d8 = float(O.cosine(a8, b8))
        if not np.isfinite(d8) or abs(raw - (d8 + 1) / 2 * 100) > 1:
            f8_fail += 1
    assert worst16 < 1e-2, worst16
    assert f8_fail > pairs // 2, f8_fail


def test_the_reference_shard_vertex_cases():
    """pkg/sharding/shard_test.go:40-63: ShardVertex is a pure function of (id, shards) — the reference checks one id 10 000 times — and
    snowflake-shaped ids spread over all 16 shards.  Restated: the oracle and the library's host entry point (FNV-1a on the CPU, no device)
    agree on that id and on 10 000 ids of the snowflake shape (time << 22 | node << 12 | sequence), and every shard is used."""
    from coltt_amd.group import shard_vertex_host
    dummy = 128545215
    want = O.shard_vertex(dummy, 16)
    assert all(O.shard_vertex(dummy, 16) == want for _ in range(100)) and shard_vertex_host(dummy, 16) == want
    t0 = 1_700_000_000_000 - 1288834974657
    ids = [((t0 + i // 7) << 22) | (i % 4096) for i in range(10_000)]
    sh = [O.shard_vertex(i, 16) for i in ids]
    assert set(sh) == set(range(16))
    counts = np.bincount(np.array(sh, np.int64), minlength=16)
    assert counts.min() > 10_000 // 16 // 2, counts
    assert [shard_vertex_host(i, 16) for i in ids[:2000]] == sh[:2000]
