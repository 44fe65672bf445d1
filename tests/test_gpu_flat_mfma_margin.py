"""COLTT_MODE_MFMA against the ORACLE on data that attacks the candidate margin (the data sets of tests/flat_mfma_ref.py, shared with
tests/test_flat_mfma_margin_host.py): near ties at the k-th place, no cancellation, stores scaled into binary16's subnormal range, a
candidate list that overflows, and stores on both sides of the cosine latch.  Every comparison is ids, ranks and score bits; Stats()
deltas say which path served the call.  Batches of >= 5 queries throughout (1 - 4 take the one-launch kernel whatever the mode)."""
import numpy as np
import pytest

import flat_mfma_ref as R
from oracle import oracle as O
from util import assert_same_results

pytestmark = pytest.mark.gpu
ID0 = np.uint64(5)


def store(gpu, metric, quant, X):
    gf = gpu.FlatSpace(X.shape[1], metric, quant)
    gf.ChangedVertex(np.arange(len(X), dtype=np.uint64) + ID0, X)
    return gf, gf.FetchRows()


def check(gpu, gf, rows, Q, k, nearest, tag, groups=1, fallbacks=0):
    """one MODE_MFMA call == the oracle's scan over the store's own rows, and the path it took"""
    st0 = gf.Stats()
    mi, ms, mc = gf.VertexSearch(Q, k, gpu.SELECT_NEAREST if nearest else gpu.SELECT_REFERENCE, gpu.MODE_MFMA)
    st1 = gf.Stats()
    sl, sc, cn, _ = O.flat_scan(rows, gf.quantization, gf.dim, gf.distance, Q, k, nearest=nearest, threads=4)
    for qi in range(len(Q)):
        assert_same_results(mi[qi, :mc[qi]], ms[qi, :mc[qi]], sl[qi, :cn[qi]] + ID0, sc[qi, :cn[qi]], f"{tag} k{k} nearest{nearest} q{qi}")
    assert st1["mfma_groups"] - st0["mfma_groups"] == groups, (tag, k, nearest, st0, st1)
    assert st1["mfma_fallbacks"] - st0["mfma_fallbacks"] == fallbacks, (tag, k, nearest, st0, st1)


BANDS = [(O.COSINE, 1.0), (O.L2, 1.0), (O.L2, 100.0)]


@pytest.mark.parametrize("quant", [O.Q_NONE, O.Q_F16, O.Q_BF16])
@pytest.mark.parametrize("metric,norm", BANDS)
def test_near_tie_bands(gpu, metric, norm, quant):
    """6 000 x 128, 16 queries, 200 planted rows per query in a band 4e-4 wide at the k-th place (the host test's data: a margin of zero
    loses 66 - 75 of the 160 top-10 members of each set in the model): the matrix cores serve every call and the answers are the oracle's."""
    for base in (0.05, 0.9, 1.9):
        X, Q = R.band_set((7000 if metric == O.COSINE else 7100) + 128, 128, 16, 2800, base, scale=norm)
        gf, rows = store(gpu, metric, quant, X)
        for k in (1, 10, 100):
            for nearest in (True, False):
                check(gpu, gf, rows, Q, k, nearest, f"m{metric} q{quant} norm{norm} base{base}")
        gf.close()


@pytest.mark.parametrize("quant", [O.Q_NONE, O.Q_F16])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_all_positive_rows_at_4096(gpu, metric, quant):
    """|Gaussian| rows and queries at the largest dimension: sum |a_i b_i| is the dot product itself, the accumulation error's worst case"""
    X, Q = R.positive_set(7200, 2000, 4096, 8)
    gf, rows = store(gpu, metric, quant, X)
    for nearest in (True, False):
        check(gpu, gf, rows, Q, 10, nearest, f"positive m{metric} q{quant}")


@pytest.mark.parametrize("metric,quant", [(O.COSINE, O.Q_NONE), (O.L2, O.Q_F16)])
def test_near_tie_band_through_the_gather_kernel(gpu, metric, quant):
    """FilterableVertexSearch with a candidate list that keeps every other row: half of each band, through flat_mfma3_kernel's GATHER mode"""
    X, Q = R.band_set(7000 + 128, 128, 16, 2800, 0.05)
    gf, rows = store(gpu, metric, quant, X)
    live = np.arange(0, len(X), 2)
    sub = np.ascontiguousarray(rows[live])
    for k in (10, 100):
        for nearest in (True, False):
            st0 = gf.Stats()
            mi, ms, mc = gf.FilterableVertexSearch(live.astype(np.uint64) + ID0, Q, k, gpu.SELECT_NEAREST if nearest else gpu.SELECT_REFERENCE, gpu.MODE_MFMA)
            st1 = gf.Stats()
            sl, sc, cn, _ = O.flat_scan(sub, quant, 128, metric, Q, k, nearest=nearest, threads=4)
            for qi in range(len(Q)):
                assert_same_results(mi[qi, :mc[qi]], ms[qi, :mc[qi]], live[sl[qi, :cn[qi]].astype(np.int64)].astype(np.uint64) + ID0, sc[qi, :cn[qi]],
                                    f"gather m{metric} k{k} nearest{nearest} q{qi}")
            assert st1["mfma_groups"] == st0["mfma_groups"] + 1 and st1["mfma_fallbacks"] == st0["mfma_fallbacks"]


@pytest.mark.parametrize("s", [1e-5, 1e-6, 1e-7])
@pytest.mark.parametrize("quant", [O.Q_NONE, O.Q_F16, O.Q_BF16])
def test_tiny_magnitude_euclidean_stores(gpu, quant, s):
    """20 000 x 128 Gaussian rows and 32 queries times s.  f32 rows: below ~3e-6 the cast to binary16 rounds with an absolute error and the
    relative margin alone loses true neighbours (7 / 22 / 95 of 320 in the model at 1e-6 / 3e-7 / 1e-7); the absolute term of flat.hip's
    l2_abs keeps them, and where it exceeds the distances themselves (1e-7) every row is kept and re-scored — 20 000 rows fit the
    candidate list, so the call still counts as a matrix-core group with no re-run.  2-byte rows at 1e-6 and 1e-7 hold binary16 SUBNORMAL
    codes: their products are exact only if neither the fragment loads nor the matrix cores flush denormals — this is the probe for that."""
    X, Q = R.scaled_set(7300 + 128, 20000, 128, 32, s)
    gf, rows = store(gpu, O.L2, quant, X)
    for nearest in (True, False):
        check(gpu, gf, rows, Q, 10, nearest, f"tiny q{quant} s{s}")


def test_near_tie_band_f8(gpu):
    """cosine "f8" rows go through a derived binary16 copy (flat.hip: f8_expand_kernel): a band of 200 rows per query whose scores differ
    only through the codec's 2^-8 steps — ~190 distinct scores inside 3e-4 — at the k-th place"""
    d = 128
    X, codes, Q = R.f8_band_set(7800, d, 16, 2800)
    ids = np.arange(len(X), dtype=np.uint64) + ID0
    src = O.Flat(d, O.L2, O.Q_F8); src.upsert(ids, X)
    stream = src.save_vertex()
    of = O.Flat(d, O.COSINE, O.Q_F8); assert of.load_vertex(stream) == 0
    gf = gpu.FlatSpace(d, O.COSINE, O.Q_F8); assert gf.LoadVertex(stream) == len(X)
    rows, row_ids = gf.FetchRows(with_ids=True)                  # a loaded store keeps the stream's (shard) order
    assert np.array_equal(rows, codes[(row_ids - ID0).astype(np.int64)])
    wi, ws = of.search(Q[0], 201, nearest=True, mode=2)          # the data is what the docstring says
    assert ws[199] - ws[0] < 3e-4 and ws[200] - ws[199] > 0.05 and len(np.unique(ws[:200])) > 150 and not np.isnan(ws).any()
    _check_stream(gpu, gf, of, Q, (1, 10, 100), 1, "f8 band")


def _overflow_rows(metric, n, d, seed):
    """cosine: 65 990 copies of one vector at cosine 0.8 from the query q, and 10 rows at cosine 0.8 + 5e-5 i: strictly better than the
    copies, by less than MF_MARGIN — the copies stay within the margin of the 10th best (for the query -q they are strictly FARTHER by the
    same steps).  Euclidean: a cluster of radius ~1e-3 at distance 100 from the origin — every row within the margin of every other."""
    v = O.fill_normal(seed, (1, d)).astype(np.float64)
    v /= np.sqrt((v * v).sum())
    w = O.fill_normal(seed + 1, (1, d)).astype(np.float64)
    w -= (w @ v.T) * v; w /= np.sqrt((w * w).sum())
    if metric == O.L2:
        X = (100.0 * v + 1e-3 * O.fill_normal(seed + 2, (n, d))).astype(np.float32)
        return X, (100.0 * v).astype(np.float32), None
    q = 0.8 * v + 0.6 * w
    u = 0.6 * v - 0.8 * w                                     # orthogonal to the query: v = 0.8 q + 0.6 u
    X = np.repeat(v, n, axis=0)
    c = 0.8 + 5e-5 * np.arange(1, 11)[:, None]
    pos = np.arange(10) * 6007 + 123                          # spread over the scan's segments
    X[pos] = c * q + np.sqrt(1.0 - c * c) * u
    return X.astype(np.float32), q.astype(np.float32), pos


@pytest.mark.parametrize("metric,quant", [(O.COSINE, O.Q_F16), (O.L2, O.Q_NONE)])
def test_an_overflowing_candidate_list_is_rerun_exactly(gpu, metric, quant):
    """66 000 rows of which (nearly) all lie within the margin of the k-th best: the candidate list of a query overflows its 65 536 entries,
    the group's flag is raised, mfma_fallbacks rises by exactly the one group and search_group_exact serves all 16 queries of it — the
    8 matching ones and the 8 random ones — with the oracle's answers; among the tied copies the smallest ids win (the largest in the farthest direction: the queue keeps the
    k largest (score, id) pairs)."""
    n, d, k = 66000, 32, 10
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(40503)) % np.uint64(66029) + ID0     # a permutation: id order is not slot order
    X, q, pos = _overflow_rows(metric, n, d, 7600)
    gf = gpu.FlatSpace(d, metric, quant); gf.ChangedVertex(ids, X)
    of = O.Flat(d, metric, quant); of.upsert(ids, X)
    special = set() if pos is None else set(int(i) for i in ids[pos])
    copies = sorted(int(i) for i in ids if int(i) not in special)
    for nearest in (True, False):
        qm = q if nearest or metric == O.L2 else -q
        Q = np.concatenate([np.repeat(qm.reshape(1, d), 8, axis=0), O.fill_normal(7610, (8, d))])
        st0 = gf.Stats()
        mi, ms, mc = gf.VertexSearch(Q, k, gpu.SELECT_NEAREST if nearest else gpu.SELECT_REFERENCE, gpu.MODE_MFMA)
        st1 = gf.Stats()
        assert st1["mfma_groups"] == st0["mfma_groups"] + 1 and st1["mfma_fallbacks"] == st0["mfma_fallbacks"] + 1, (nearest, st0, st1)
        for qi in range(len(Q)):
            wi, ws = of.search(Q[qi], k, nearest=nearest, mode=2)
            assert_same_results(mi[qi, :mc[qi]], ms[qi, :mc[qi]], wi, ws, f"overflow m{metric} nearest{nearest} q{qi}")
        if metric == O.COSINE:
            # the data is what the docstring says: by the oracle's exact scores the ten rows beat the copies, by less than MF_MARGIN
            wi, ws = of.search(Q[0], k + 1, nearest=nearest, mode=2)
            cs = ws[[int(i) not in special for i in wi]]; sp = ws[[int(i) in special for i in wi]]
            assert len(cs) == 1 and len(np.unique(sp)) == 10 and ((sp < cs[0]).all() if nearest else (sp > cs[0]).all())
            assert np.abs(sp - cs[0]).max() < 5.8e-4 < R.constants()["MF_MARGIN"]
            assert set(int(i) for i in mi[0]) == special
            n_tied = 0
            for qi in range(8, 16):                                       # random queries: the copies in their answers tie
                tied = [int(i) for i in mi[qi] if int(i) not in special]
                # canonical (score, id) order: the k nearest are the k SMALLEST pairs, the k farthest the k LARGEST (edge/priority_queue.go:39-69)
                assert tied == (copies[:len(tied)] if nearest else copies[len(copies) - len(tied):]), "tie winners are the smallest (farthest: largest) ids"
                n_tied += len(tied)
            assert n_tied >= 10
    gf.close()


def _stream_stores(gpu, quant, d, X):
    """X as a LOADED stream (stored as it is, never re-normalised) in a cosine store of the GPU and of the oracle"""
    ids = np.arange(len(X), dtype=np.uint64) + ID0
    src = O.Flat(d, O.L2, quant); src.upsert(ids, X)             # an L2 store keeps the rows unnormalised; the stream is metric-agnostic
    stream = src.save_vertex()
    of = O.Flat(d, O.COSINE, quant); assert of.load_vertex(stream) == 0
    gf = gpu.FlatSpace(d, O.COSINE, quant); assert gf.LoadVertex(stream) == len(X)
    return gf, of


def _check_stream(gpu, gf, of, Q, ks, groups, tag):
    for k in ks:
        for nearest in (True, False):
            st0 = gf.Stats()
            mi, ms, mc = gf.VertexSearch(Q, k, gpu.SELECT_NEAREST if nearest else gpu.SELECT_REFERENCE, gpu.MODE_MFMA)
            st1 = gf.Stats()
            for qi in range(len(Q)):
                wi, ws = of.search(Q[qi], k, nearest=nearest, mode=2)
                assert_same_results(mi[qi, :mc[qi]], ms[qi, :mc[qi]], wi, ws, f"{tag} k{k} nearest{nearest} q{qi}")
            assert st1["mfma_groups"] - st0["mfma_groups"] == groups and st1["mfma_fallbacks"] == st0["mfma_fallbacks"], (tag, k, nearest, st0, st1)


def test_cosine_f16_stream_of_odd_norms_stays_on_the_exact_scan(gpu):
    """the round-3 latch test has f32 rows only: a cosine F16 store loaded with ||row||^2 outside [1/4, 4] answers MODE_MFMA through the
    exact scan — and says so through NormBounds"""
    n, d = 4000, 128
    X = O.fill_normal(7700, (n, d))
    X[::3] *= np.float32(1e-2 / np.sqrt(d)); X[1::3] *= np.float32(30 / np.sqrt(d)); X[2::3] *= np.float32(1 / np.sqrt(d))
    gf, of = _stream_stores(gpu, O.Q_F16, d, X)
    mn, mx, open_ = gf.NormBounds()
    assert not open_ and mn < 1e-3 and mx > 100 and not gpu.FlatSpace.MfmaEligible(O.COSINE, O.Q_F16, d, mn, mx)
    _check_stream(gpu, gf, of, O.fill_normal(7701, (24, d)), (10,), 0, "odd norms f16")


@pytest.mark.parametrize("quant", [O.Q_NONE, O.Q_F16])
def test_cosine_stream_inside_the_latch_but_far_from_one(gpu, quant):
    """rows of norm 0.55 and 1.9 (||row||^2 = 0.30 and 3.61: inside [1/4, 4], far from 1) carrying a near-tie band: the matrix cores serve
    the store and the margin — proved for norm ~1 — still holds"""
    d = 128
    X, Q = R.band_set(7000 + d, d, 16, 2800, 0.05)
    X[::2] *= np.float32(0.55); X[1::2] *= np.float32(1.9)
    gf, of = _stream_stores(gpu, quant, d, X)
    mn, mx, open_ = gf.NormBounds()
    assert open_ and 0.25 < mn < 0.32 and 3.5 < mx < 4.0 and gpu.FlatSpace.MfmaEligible(O.COSINE, quant, d, mn, mx)
    _check_stream(gpu, gf, of, Q, (1, 10, 100), 1, f"norms 0.55 / 1.9 q{quant}")
