"""Filtered search over the product-quantised HNSW walk on the GPU (coltt_hnsw_pq_search_filtered; include/coltt_gpu.h) against its CPU
restatement (tests/filtered_pq_ref.py) over GPU-built graphs: WALK (ids, exact score bits, counts, counters) over the LDS-hash walk, the
byte-map walk with neighbourhood blocks and the byte-map walk that gathers, every kernel form of the (LS, NP) dispatch and rows of 64;
counts; tombstones and later inserts; answer quality against a post-filter (a property, no measured threshold); EXACT and AUTO; errors;
concurrency with inserts; PqSearch unchanged."""
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


def _consts(gpu, case):
    metric, quant = case[0], case[1]
    return (gpu.COSINE if metric == "cos" else gpu.EUCLIDEAN, gpu.Q_NONE if quant == "f32" else gpu.Q_F16,
            O.COSINE if metric == "cos" else O.L2, O.Q_NONE if quant == "f32" else O.Q_F16)


def _make(gpu, case, n, graph):
    """index (graph built on the GPU, as test_gpu_round5._pq_case does) + a quantiser trained on its stored rows, attached"""
    import torch
    M, Qn, om, oq = _consts(gpu, case)
    d, m, c, pqm = case[2], case[3], case[4], case[5]
    X, lv, Q = P.case_data(case, n)
    h = gpu.Hnsw(d, M, gpu.HnswCfg.default(**graph), quantization=Qn)
    xd = torch.from_numpy(X).to("cuda:0"); torch.cuda.synchronize()
    h.InsertBatchDevice(xd.data_ptr(), n, lv, batch=64)
    seen = F.decode(oq, h.FetchRows())
    pq = gpu.PQSpace(d, pqm, m, c)
    pq.Fit(seen[: max(c, min(n, 2000))], iterations=4)
    h.PqAttach(pq)
    return h, pq.Codebooks(), Q


class _View:
    """what the restatement reads, taken from the index as it is now"""

    def __init__(self, gpu, h, case, cb):
        _, _, self.om, self.oq = _consts(gpu, case)
        self.g = h.ExportRaw(); self.rows = F.decode(self.oq, h.FetchRows()); self.codes = h.PqCodes(); self.cb = cb; self.pqm = case[5]
        ex = h.Export()
        self.ids = ex["ids"]; self.deleted = ex["deleted"].astype(bool); self.n = len(self.ids)
        self._walks = {}

    def walk(self, query, qi, ef):
        """the restated walk, once per (query, ef): it depends on neither the filter nor rerank"""
        if (qi, ef) not in self._walks:
            q = F.prep_query(self.om, self.oq, query)
            dall = P.table_distances(self.cb, self.pqm, self.codes, q)
            g = self.g
            self._walks[(qi, ef)] = (q, dall) + P.walk(g["adj0"], g["upper_off"], g["adjU"], g["entry"], g["entry_level"], dall, ef, self.deleted)
        return self._walks[(qi, ef)]

    def answer(self, query, qi, ef, allow, k, rerank):
        q, dall, res, expanded, ep, st = self.walk(query, qi, ef)
        _, R = P.allowed_set(self.g["adj0"], expanded, ep, dall, allow, self.deleted, P.cap_of(ef, k, rerank))
        s, v = P.rerank_set(self.rows, self.om, q, R, k)
        return s, v, len(R), st


_CACHE = {}


def _index(gpu, case, n, graph):
    """one index + view per case, shared by the tests that do not change it"""
    if case not in _CACHE:
        h, cb, Q = _make(gpu, case, n, graph)
        _CACHE[case] = (h, _View(gpu, h, case, cb), Q)
    return _CACHE[case]


def _check(gpu, h, v, Q, flt, allow, ef, rerank, k=K, tag=()):
    gi, gs, gc, st = h.PqSearchFiltered(Q, k, flt, ef=ef, rerank=rerank, mode=gpu.FILTER_WALK, with_stats=True)
    assert st["path"] == gpu.FILTER_WALK and st["ef_walk"] == max(ef, k) and st["n_visit_resets"] == 0, (tag, st)
    tot = {"n_dist": 0, "n_exp": 0, "n_hops": 0}; nr = 0
    for qi in range(len(Q)):
        s, val, r, t = v.answer(Q[qi], qi, max(ef, k), allow, k, rerank)
        c = int(gc[qi])
        assert c == len(s) == min(k, r), (tag, qi, c, len(s), r)
        assert np.array_equal(gi[qi, :c], v.ids[s]), (tag, qi, gi[qi, :c], s)
        assert np.array_equal(bits(gs[qi, :c]), bits(val)), (tag, qi)
        nr += r
        for kk in tot:
            tot[kk] += t[kk]
    assert {kk: st[kk] for kk in tot} == tot, (tag, st, tot)
    assert st["n_exact_rows"] == nr, (tag, st["n_exact_rows"], nr)
    return st


@pytest.mark.parametrize("case,n,graph", ALL)
def test_walk_equals_the_restatement(gpu, monkeypatch, case, n, graph):
    h, v, Q = _index(gpu, case, n, graph)
    plain = {ef: h.PqSearch(Q, K, ef=ef, with_stats=True)[3] for ef in P.WALK_EFS}
    for frac in P.WALK_FRACS:
        allow = P.allow_mask(case, n, frac)
        with h.Filter(np.nonzero(allow)[0]) as flt:
            assert flt.allowed == int(allow.sum())
            # ef 48: LDS hash | ef 300: byte map with the neighbourhood blocks, and the same walk gathering code rows by neighbour slot
            for ef, nbr in ((48, None), (300, None), (300, "0")):
                if nbr is not None:
                    monkeypatch.setenv("COLTT_PQ_NBR", nbr)
                try:
                    for rerank in P.WALK_RERANKS:      # 0: all of R | 12 | 3 -> r = k | 1000 -> capped at ef
                        st = _check(gpu, h, v, Q, flt, allow, ef, rerank, tag=(frac, ef, nbr, rerank))
                        assert {kk: st[kk] for kk in ("n_dist", "n_exp", "n_hops")} == {kk: plain[ef][kk] for kk in ("n_dist", "n_exp", "n_hops")}, (frac, ef, nbr)
                finally:
                    if nbr is not None:
                        monkeypatch.delenv("COLTT_PQ_NBR")


def test_counts(gpu):
    case, n, graph = ALL[0]
    h, v, Q = _index(gpu, case, n, graph)
    # k larger than |R|: count = |R|
    allow = P.allow_mask(case, n, 0.01)
    with h.Filter(np.nonzero(allow)[0]) as flt:
        for ef in (48, 300):
            _check(gpu, h, v, Q, flt, allow, ef, 0, k=40, tag=("k > |R|", ef))
        sizes = [v.answer(Q[qi], qi, 48, allow, 40, 0)[2] for qi in range(len(Q))]
        assert min(sizes) < 40, sizes                      # the case does exercise count < k
    # an empty filter: counts 0 through every mode, no error
    with h.Filter([10 ** 12]) as empty:
        assert empty.allowed == 0
        for mode in (gpu.FILTER_WALK, gpu.FILTER_EXACT, gpu.FILTER_AUTO):
            _, _, gc = h.PqSearchFiltered(Q, K, empty, ef=48, mode=mode)
            assert (gc == 0).all(), mode
    # an all-ones filter
    ones = np.ones(n, bool)
    with h.Filter(np.arange(n)) as flt:
        for ef in (48, 300):
            _check(gpu, h, v, Q, flt, ones, ef, 0, tag=("all ones", ef))
    # a filter whose only member is query 0's level-0 entry point
    ep = v.walk(Q[0], 0, 48)[4]
    only = np.zeros(n, bool); only[ep] = True
    with h.Filter([int(v.ids[ep])]) as flt:
        _check(gpu, h, v, Q, flt, only, 48, 0, tag=("entry point only",))
        gi, _, gc = h.PqSearchFiltered(Q[:1], K, flt, ef=48, mode=gpu.FILTER_WALK)
        assert gc[0] == 1 and gi[0, 0] == v.ids[ep]
    # nq == 0 is not an error
    with h.Filter(np.arange(n)) as flt:
        gi, gs, gc = h.PqSearchFiltered(np.zeros((0, case[2]), np.float32), K, flt)
        assert gc.shape == (0,)


def test_tombstones_and_later_inserts(gpu):
    import torch
    case, n, graph = P.CASES[0], P.N, P.GRAPH
    h, cb, Q = _make(gpu, case, n, graph)
    allow = P.allow_mask(case, n, 0.3)
    flt = h.Filter(np.nonzero(allow)[0])
    gone = np.random.default_rng(17).choice(n, n // 20, replace=False)      # 5 % of the vertices, after the attach
    assert allow[gone].any() and not allow[gone].all()
    for i in gone:
        h.Remove(int(i))
    v = _View(gpu, h, case, cb)
    assert v.deleted.sum() == len(gone)
    for ef in (48, 300):
        for rerank in (0, 12):
            _check(gpu, h, v, Q, flt, allow, ef, rerank, tag=("removed", ef, rerank))
    gi, _, gc = h.PqSearchFiltered(Q, K, flt, ef=300, mode=gpu.FILTER_WALK)
    assert not set(int(x) for qi in range(len(Q)) for x in gi[qi, :gc[qi]]) & set(int(x) for x in gone)
    # 200 rows inserted after the filter exists: never returned, and the walk over the new graph still equals the restatement
    d = case[2]
    X2 = np.concatenate([Q, O.fill_normal(7999, (200 - len(Q), d))]); lv2 = O.levels(8000, 200)   # copies of the queries: they would be the nearest
    x2 = torch.from_numpy(np.ascontiguousarray(X2)).to("cuda:0"); torch.cuda.synchronize()
    h.InsertBatchDevice(x2.data_ptr(), 200, lv2, batch=16, first_id=n)
    v2 = _View(gpu, h, case, cb)
    assert v2.n == n + 200 and len(v2.codes) == n + 200
    for ef in (48, 300):
        _check(gpu, h, v2, Q, flt, allow, ef, 0, tag=("inserted", ef))
        gi, _, gc = h.PqSearchFiltered(Q, K, flt, ef=ef, mode=gpu.FILTER_WALK)
        assert all(int(x) < n for qi in range(len(Q)) for x in gi[qi, :gc[qi]])
    flt.close()


@pytest.mark.parametrize("case,n,graph", ALL)
def test_answer_is_no_worse_than_a_post_filter(gpu, case, n, graph):
    """A property, no measured threshold: the filtered answer is element-wise <= the post-filter of PqSearch(k = ef, rerank = 0) — the allowed
    members of the walk's re-ranked result set — by (score bits, id), and holds at least as many (tests/test_filtered_pq_ref.py: R holds the
    allowed part of the result set, and every member of R is re-ranked)."""
    h, v, Q = _index(gpu, case, n, graph)
    ef = P.PROP_EF
    pi, ps, pc = h.PqSearch(Q, ef, ef=ef, rerank=0)
    for frac in P.PROP_FRACS:
        allow = P.allow_mask(case, n, frac)
        with h.Filter(np.nonzero(allow)[0]) as flt:
            gi, gs, gc = h.PqSearchFiltered(Q, K, flt, ef=ef, rerank=0, mode=gpu.FILTER_WALK)
        for qi in range(len(Q)):
            post = [((int(b) << 32) | int(i)) for b, i in zip(bits(ps[qi, :pc[qi]]), pi[qi, :pc[qi]]) if allow[int(i)]][:K]
            got = [((int(b) << 32) | int(i)) for b, i in zip(bits(gs[qi, :gc[qi]]), gi[qi, :gc[qi]])]   # ids ascend with slots here
            assert len(got) >= len(post), (frac, qi, len(got), len(post))
            assert all(a <= b for a, b in zip(got, post)), (frac, qi)
            assert all(allow[int(i)] for i in gi[qi, :gc[qi]])


def test_exact_and_auto_paths(gpu):
    case, n, graph = ALL[0]
    h, v, Q = _index(gpu, case, n, graph)
    allow = P.allow_mask(case, n, 0.1)
    with h.Filter(np.nonzero(allow)[0]) as flt:      # EXACT: the row walk's exact path, bit for bit
        for k in (K, 400):
            a = h.PqSearchFiltered(Q, k, flt, rerank=12, mode=gpu.FILTER_EXACT, with_stats=True)
            b = h.SearchFiltered(Q, k, flt, mode=gpu.FILTER_EXACT, with_stats=True)
            assert np.array_equal(a[2], b[2]) and a[3] == b[3] and a[3]["path"] == gpu.FILTER_EXACT
            for qi in range(len(Q)):
                c = a[2][qi]
                assert np.array_equal(a[0][qi, :c], b[0][qi, :c]) and np.array_equal(bits(a[1][qi, :c]), bits(b[1][qi, :c]))
    n_live = h.Len()
    rng = np.random.default_rng(9)
    walked = 0
    for frac in (1.0, 0.9, 0.5, 0.1, 0.01):          # AUTO: the grid of test_gpu_hnsw_filter.test_auto_follows_the_rule
        al = rng.random(n) < frac
        with h.Filter(np.nonzero(al)[0]) as flt:
            for ef in (20, 64, 128):
                for k in (10, 100):
                    gi, gs, gc, st = h.PqSearchFiltered(Q, k, flt, ef=ef, with_stats=True)
                    want = F.auto_path(flt.allowed, n_live, max(ef, k))
                    assert (st["path"], st["ef_walk"]) == want, (frac, ef, k, st)
                    _, _, _, rst = h.SearchFiltered(Q, k, flt, ef=ef, with_stats=True)
                    assert (rst["path"], rst["ef_walk"]) == want          # one filter, one path through either entry point
                    if want[0] == F.WALK:
                        walked += 1
                        for qi in range(len(Q)):
                            s, val, r, _ = v.answer(Q[qi], qi, want[1], al, k, 0)
                            assert gc[qi] == len(s) and np.array_equal(gi[qi, :gc[qi]], v.ids[s]) and np.array_equal(bits(gs[qi, :gc[qi]]), bits(val))
    assert walked >= 3


def test_errors(gpu):
    import torch
    case, n, graph = ALL[0]
    h, v, Q = _index(gpu, case, n, graph)
    d = case[2]
    X, lv, _ = P.case_data(case, 600)
    bare = gpu.Hnsw(d, gpu.EUCLIDEAN, gpu.HnswCfg.default(**graph))
    xd = torch.from_numpy(X).to("cuda:0"); torch.cuda.synchronize()
    bare.InsertBatchDevice(xd.data_ptr(), 600, lv, batch=64)
    # no quantiser attached: COLTT_E_INVALID, for every mode — and before the filter is looked at
    with bare.Filter(np.arange(100)) as bf, h.Filter(np.arange(100)) as hf:
        for mode in (gpu.FILTER_AUTO, gpu.FILTER_WALK, gpu.FILTER_EXACT):
            for f in (bf, hf):
                with pytest.raises(gpu.ColttError) as e:
                    bare.PqSearchFiltered(Q, K, f, mode=mode)
                assert e.value.code == -1, mode
        # a filter of another index
        with pytest.raises(gpu.ColttError) as e:
            h.PqSearchFiltered(Q, K, bf)
        assert e.value.code == -1
        # ef 5 000
        with pytest.raises(gpu.ColttError) as e:
            h.PqSearchFiltered(Q, K, hf, ef=5000)
        assert e.value.code == -4
        # an unknown mode
        with pytest.raises(gpu.ColttError) as e:
            h.PqSearchFiltered(Q, K, hf, mode=7)
        assert e.value.code == -1
    # a closed (unknown) filter handle
    import ctypes
    dead = h.Filter(np.arange(10)); raw = ctypes.c_uint64(dead.h.value); dead.close()
    dead.h = raw                                      # the handle of a destroyed filter: COLTT_E_NOT_FOUND, as SearchFiltered
    for call in (h.PqSearchFiltered, h.SearchFiltered):
        with pytest.raises(gpu.ColttError) as e:
            call(Q, K, dead)
        assert e.value.code == -3
    dead.h = None
    # a filter made stale by Load
    h2, cb2, _ = _make(gpu, case, 600, graph)
    stale = h2.Filter(np.arange(50))
    h2.Load(bare.Commit())
    with pytest.raises(gpu.ColttError) as e:
        h2.PqSearchFiltered(Q, K, stale, mode=gpu.FILTER_WALK)
    assert e.value.code == -1
    stale.close()
    # an empty index that carries a quantiser: counts 0, no error
    e_idx = gpu.Hnsw(d, gpu.EUCLIDEAN)
    pq = gpu.PQSpace(d, case[5], case[3], case[4]); pq.SetCodebooks(cb2)
    e_idx.PqAttach(pq)
    with e_idx.Filter([1, 2]) as f0:
        for mode in (gpu.FILTER_AUTO, gpu.FILTER_WALK, gpu.FILTER_EXACT):
            _, _, gc = e_idx.PqSearchFiltered(Q, K, f0, mode=mode)
            assert (gc == 0).all()


def test_concurrent_searches_with_inserts(gpu):
    case, n, graph = P.CASES[0], P.N, P.GRAPH
    h, cb, Q = _make(gpu, case, n, graph)
    d = case[2]
    allow_ids = np.arange(1, n, 3, dtype=np.uint64)
    ok_set = set(int(x) for x in allow_ids)
    flt = h.Filter(allow_ids)
    errors = []
    stop = threading.Event()

    def searcher(ef):
        try:
            for _ in range(15):
                gi, gs, gc = h.PqSearchFiltered(Q, K, flt, ef=ef, rerank=0, mode=gpu.FILTER_WALK)
                for qi in range(len(Q)):
                    if gc[qi] != K or not set(int(x) for x in gi[qi, :gc[qi]]) <= ok_set:
                        errors.append((ef, qi, int(gc[qi])))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    def inserter():
        try:
            Y = O.fill_normal(84, (120, d))
            for j in range(120):
                if stop.is_set():
                    break
                h.Insert(n + j, Y[j], 0)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=searcher, args=(ef,)) for ef in (64, 300)]
    ti = threading.Thread(target=inserter)
    for t in ts + [ti]:
        t.start()
    for t in ts:
        t.join()
    stop.set(); ti.join()
    flt.close()
    assert not errors, errors[:5]


def test_pq_search_is_unchanged_by_a_filtered_call(gpu):
    case, n, graph = ALL[1]
    h, v, Q = _index(gpu, case, n, graph)
    allow = P.allow_mask(case, n, 0.1)
    for ef, rr in ((48, 0), (300, 0), (300, 12)):
        before = h.PqSearch(Q, K, ef=ef, rerank=rr, with_stats=True)
        with h.Filter(np.nonzero(allow)[0]) as flt:
            h.PqSearchFiltered(Q, K, flt, ef=ef, rerank=rr, mode=gpu.FILTER_WALK)
        after = h.PqSearch(Q, K, ef=ef, rerank=rr, with_stats=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(bits(before[1]), bits(after[1])) and np.array_equal(before[2], after[2])
        assert before[3] == after[3], (ef, rr)
