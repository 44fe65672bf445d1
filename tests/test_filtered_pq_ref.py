"""CPU suite for the restatement of filtered search over the product-quantised walk (tests/filtered_pq_ref.py): its walk alone is the
oracle's csr_search_pq (slots, score bits, counters; with and without tombstones); on the GPU suite's own inputs its allowed set holds
every allowed member of the walk's result set (what the GPU property test rests on); with an all-ones filter R is element-wise <= the
result set; AUTO is the row walk's rule.  No GPU needed."""
import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import filtered_ref as F
import filtered_pq_ref as P

_CACHE = {}


def _case(case, n, graph):
    """graph by oracle.Hnsw, quantiser by oracle.pq_train, codes by oracle.pq_encode — computed once per case, never changed"""
    key = (case, n)
    if key not in _CACHE:
        metric, quant, d, m, c, pqm = case
        M = O.COSINE if metric == "cos" else O.L2
        Qn = O.Q_NONE if quant == "f32" else O.Q_F16
        X, lv, Q = P.case_data(case, n)
        h = O.Hnsw(d, M, cfg=O.default_cfg(**graph), canonical_build=True)
        h.insert_many(np.arange(n, dtype=np.uint64), X, lv)
        g = h.export()
        adj0, uo, adjU = F.csr_from_export(g, h.cfg.mMax0, h.cfg.mMax)
        stored = g["vectors"] if Qn == O.Q_NONE else O.lower(Qn, g["vectors"])      # what the index keeps
        rows = F.decode(Qn, stored)                                                  # ... as its distance sees it
        cb = O.pq_train(rows[: max(c, min(n, 2000))], m, c, 4)
        codes = O.pq_encode(cb, rows)
        gg = {"adj0": adj0, "upper_off": uo, "adjU": adjU, "entry": g["entry"], "entry_level": int(g["levels"][g["entry"]])}
        _CACHE[key] = (M, Qn, d, pqm, stored, rows, gg, cb, codes, Q)
    return _CACHE[key]


def _del_bits(deleted):
    b = np.packbits(deleted.astype(np.uint8), bitorder="little")
    return np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)]).view(np.uint32)


ALL = [(c, P.N, P.GRAPH) for c in P.CASES] + [(P.WIDE, P.N_WIDE, P.GRAPH_WIDE)]


@pytest.mark.parametrize("tomb", [False, True])
@pytest.mark.parametrize("case,n,graph", ALL)
def test_restated_walk_is_csr_search_pq(case, n, graph, tomb):
    """the walk alone == oracle.csr_search_pq(k = ef, rerank = 0): the whole result set re-ranked — same slots, same exact score bits,
    same n_dist / n_exp / n_hops — without tombstones and with them"""
    M, Qn, d, pqm, stored, rows, g, cb, codes, Q = _case(case, n, graph)
    deleted = None
    if tomb:
        deleted = np.random.default_rng(5).random(n) < 0.05
        deleted[g["entry"]] = False
    for ef in (48, 300):
        sl, sc, cn, ost, _ = O.csr_search_pq(stored, Qn, g["adj0"], g["upper_off"], g["adjU"], d, M, g["entry"], g["entry_level"], codes, cb, pqm, Q, ef, ef,
                                             rerank=0, del_bits=_del_bits(deleted) if tomb else None)
        tot = {"n_dist": 0, "n_exp": 0, "n_hops": 0}
        for qi in range(len(Q)):
            q = F.prep_query(M, Qn, Q[qi])
            dall = P.table_distances(cb, pqm, codes, q)
            res, _, _, st = P.walk(g["adj0"], g["upper_off"], g["adjU"], g["entry"], g["entry_level"], dall, ef, deleted)
            s, v = P.rerank_set(rows, M, q, res, ef)
            assert len(s) == cn[qi], (ef, qi)
            assert np.array_equal(s, sl[qi, :cn[qi]].astype(np.int64)), (ef, qi)
            assert np.array_equal(bits(v), bits(sc[qi, :cn[qi]])), (ef, qi)
            if tomb:
                assert not deleted[s].any()
            for kk in tot:
                tot[kk] += st[kk]
        assert tot == {kk: ost[kk] for kk in tot}, (ef, tot, ost)
        assert ost["n_exact"] == int(cn.sum())


@pytest.mark.parametrize("case,n,graph", ALL)
def test_allowed_set_holds_the_allowed_part_of_the_result_set(case, n, graph):
    """On the GPU suite's inputs: R (cap = ef) ⊇ result set ∩ allowed.  A member of the result set was listed by an expanded vertex (or is
    the entry point) and is live, so it is in C when it is allowed; a member of C outside the result set was refused by a lowerBound that
    only fell afterwards, so it does not sort before a member — short of a tie in the distance bits, which these inputs do not have."""
    M, Qn, d, pqm, stored, rows, g, cb, codes, Q = _case(case, n, graph)
    for ef, fracs in [(P.PROP_EF, P.PROP_FRACS)] + [(e, P.WALK_FRACS) for e in P.WALK_EFS]:
        for qi in range(len(Q)):
            q = F.prep_query(M, Qn, Q[qi])
            dall = P.table_distances(cb, pqm, codes, q)
            res, expanded, ep, _ = P.walk(g["adj0"], g["upper_off"], g["adjU"], g["entry"], g["entry_level"], dall, ef)
            for frac in fracs:
                allow = P.allow_mask(case, n, frac)
                C, R = P.allowed_set(g["adj0"], expanded, ep, dall, allow, None, ef)
                want = set(x for x in res if allow[x & 0xFFFFFFFF])
                assert want <= set(R), (ef, frac, qi)
                assert all(allow[x & 0xFFFFFFFF] for x in R) and R == sorted(R) and len(R) == min(ef, len(C))


@pytest.mark.parametrize("case,n,graph", ALL)
def test_all_ones_allowed_set_is_elementwise_below_the_result_set(case, n, graph):
    M, Qn, d, pqm, stored, rows, g, cb, codes, Q = _case(case, n, graph)
    allow = np.ones(n, bool)
    for ef in (48, 300):
        for qi in range(len(Q)):
            w = P.Walked(rows, g, M, cb, pqm, codes, F.prep_query(M, Qn, Q[qi]), ef, allow)
            assert len(w.R) >= len(w.res) and all(a <= b for a, b in zip(w.R, w.res)), (ef, qi)
            s, v, nr = w.answer(P.K, 0)
            assert nr == len(w.R) and len(s) == min(P.K, nr)


def test_rerank_caps_and_counts():
    case, n, graph = ALL[0]
    M, Qn, d, pqm, stored, rows, g, cb, codes, Q = _case(case, n, graph)
    assert [P.cap_of(300, 10, r) for r in (0, 12, 3, 1000)] == [300, 12, 10, 300]
    allow = P.allow_mask(case, n, 0.01)
    w = P.Walked(rows, g, M, cb, pqm, codes, F.prep_query(M, Qn, Q[0]), 48, allow)
    assert 0 < len(w.R) < 48                     # a selective filter: fewer allowed vertices met than the cap
    s, v, nr = w.answer(100, 0)                  # k larger than |R|: count = |R|
    assert len(s) == nr == len(w.R)
    s3, _, n3 = w.answer(2, 3)                   # rerank 3, k 2: cap 3
    assert n3 == min(3, len(w.R)) and len(s3) == min(2, n3)
    keys = [(int(b), int(x)) for b, x in zip(bits(v), s)]
    assert keys == sorted(keys) and allow[s].all()


@pytest.mark.parametrize("A,n_live,ef,want", [
    (2000, 2000, 64, (F.EXACT, 0)),              # a small index: A <= 32 x ef_walk = 2048
    (3000, 3000, 64, (F.WALK, 64)),              # the GPU suite's index under an all-ones filter: 3000 > 2048
    (100_000, 100_000, 128, (F.WALK, 128)),
    (50_000, 100_000, 128, (F.WALK, 256)),
    (10_000, 100_000, 128, (F.EXACT, 0)),        # 10 % of 100 k: ef_walk 1280, 32 x 1280 >= A
    (100_000, 1_000_000, 128, (F.WALK, 1280)),   # 10 % of 1 M: the breadth where the walk over codes is at home
    (1_000, 1_000_000, 64, (F.EXACT, 0)),        # ef_need > 4096
    (0, 1000, 64, (F.EXACT, 0)),
])
def test_auto_is_the_row_walks_rule(A, n_live, ef, want):
    assert F.auto_path(A, n_live, ef) == want
    assert F.auto_path(A, n_live, ef, F.WALK) == (F.WALK, ef)
