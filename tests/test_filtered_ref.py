"""CPU suite for the filtered-search restatement (tests/filtered_ref.py): with an all-ones filter its walk is the oracle's canonical
csr_search (ids, score bits, counters); its EXACT is a brute force over the allowed rows; its AUTO rule is the documented one.
No GPU needed."""
import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import filtered_ref as F


def _graph(n, d, metric, seed, m=8):
    X = O.fill_normal(seed, (n, d)); lv = O.levels(seed + 1, n, m)
    cfg = O.default_cfg(m=m, ef_construction=48)
    h = O.Hnsw(d, metric, cfg=cfg, canonical_build=True)
    h.insert_many(np.arange(n, dtype=np.uint64), X, lv)
    g = h.export()
    adj0, uo, adjU = F.csr_from_export(g, h.cfg.mMax0, h.cfg.mMax)
    entry = g["entry"]
    return g["vectors"], adj0, uo, adjU, entry, int(g["levels"][entry])


def _keys(b, s):
    return [(int(x) << 32) | int(y) for x, y in zip(b, s)]


@pytest.mark.parametrize("metric,quant", [(O.COSINE, O.Q_NONE), (O.L2, O.Q_NONE), (O.L2, O.Q_F16)])
def test_all_ones_walk_is_csr_search_plus_the_evaluated_neighbours(metric, quant):
    """All-ones filter: the walk IS the canonical csr_search (same counters), and R is the k smallest of everything the level-0 walk
    evaluated.  That is a superset of the walk's result set: a neighbour refused by the stale lowerBound (sampled once per pop, before
    the free slots fill) can beat the result set's k-th member.  So R is element-wise <= the unfiltered answer, and equal to it when no
    such neighbour exists (most queries; always at ef >> k on these graphs)."""
    n, d, k = 700, 24, 10
    V, adj0, uo, adjU, entry, el = _graph(n, d, metric, 11 + metric)
    stored = V if quant == O.Q_NONE else O.lower(quant, V)   # what the index keeps
    rows = F.decode(quant, stored)
    Q = O.fill_normal(99, (12, d))
    allow = np.ones(n, bool)
    for ef in (16, 64):
        sl, sc, cn, st, _ = O.csr_search(stored, quant, adj0, uo, adjU, d, metric, entry, el, Q, k, ef)
        tot = {"n_dist": 0, "n_exp": 0, "n_hops": 0}
        same = 0
        for i in range(len(Q)):
            q = F.prep_query(metric, quant, Q[i])
            s, v, t = F.walk(rows, adj0, uo, adjU, metric, entry, el, q, k, ef, allow)
            got, want = _keys(bits(v), s), _keys(bits(sc[i, :cn[i]]), sl[i, :cn[i]])
            assert len(got) == len(want) and all(a <= b for a, b in zip(got, want)), (ef, i)
            same += got == want
            for key in tot:
                tot[key] += t[key]
        assert tot == st, (ef, tot, st)
        assert same >= (len(Q) * 2) // 3, (ef, same)
        if ef == 64:
            assert same == len(Q)


def test_walk_keeps_only_allowed_and_is_a_top_k_of_what_it_evaluated():
    n, d, k, ef = 600, 16, 8, 32
    V, adj0, uo, adjU, entry, el = _graph(n, d, O.L2, 5)
    rng = np.random.default_rng(3)
    allow = rng.random(n) < 0.3
    q = F.prep_query(O.L2, O.Q_NONE, O.fill_normal(7, (1, d))[0])
    s, v, st = F.walk(V, adj0, uo, adjU, O.L2, entry, el, q, k, ef, allow)
    s1, v1, st1 = F.walk(V, adj0, uo, adjU, O.L2, entry, el, q, k, ef, np.ones(n, bool))
    assert st == st1                         # the walk itself does not depend on the filter
    assert len(s) <= k and allow[s].all()
    keys = [(int(b), int(x)) for b, x in zip(bits(v), s)]
    assert keys == sorted(keys)


def test_exact_equals_brute_force():
    n, d = 500, 20
    rng = np.random.default_rng(1)
    rows = O.fill_normal(2, (n, d))
    for metric in (O.COSINE, O.L2):
        stored = O.normalize(rows) if metric == O.COSINE else rows
        allow = rng.random(n) < 0.2; deleted = rng.random(n) < 0.1
        q = F.prep_query(metric, O.Q_NONE, O.fill_normal(3, (1, d))[0])
        for k in (5, 10, 1000):              # including k > A
            s, v = F.exact(stored, metric, q, k, allow, deleted)
            want = []
            for i in range(n):
                if allow[i] and not deleted[i]:
                    dv = O.cosine(q, stored[i]) if metric == O.COSINE else O.l2(q, stored[i])
                    want.append((int(np.float32(dv).view(np.uint32)), i))
            want = sorted(want)[:k]
            assert [(int(b), int(x)) for b, x in zip(bits(v), s)] == want, (metric, k)
            assert len(s) == min(k, int((allow & ~deleted).sum()))


@pytest.mark.parametrize("A,n_live,ef,want", [
    (100_000, 100_000, 128, (F.WALK, 128)),      # everything allowed: the walk at ef
    (50_000, 100_000, 128, (F.WALK, 256)),       # half: ef_need = 256
    (10_000, 100_000, 128, (F.EXACT, 0)),        # 10 %: ef_walk 1280, 32 x 1280 = 40 960 >= A
    (200_000, 1_000_000, 128, (F.WALK, 640)),    # 20 % of 1 M: 32 x 640 = 20 480 < A
    (40_960, 100_000, 128, (F.WALK, 313)),       # ef_need = ceil(312.5) = 313; 32 x 313 = 10 016 < A
    (1_000, 1_000_000, 64, (F.EXACT, 0)),        # ef_need = 64 000 > 4096
    (4_096, 4_096, 128, (F.EXACT, 0)),           # a small index: A <= 32 x 128
    (0, 1000, 64, (F.EXACT, 0)),                 # empty filter
])
def test_auto_rule(A, n_live, ef, want):
    assert F.auto_path(A, n_live, ef) == want


def test_auto_rule_at_the_boundary_and_forced_modes():
    # the rule as documented, over a range of A that crosses the boundary
    n_live, ef = 1_000_000, 128
    for A in range(40_000, 60_000, 7):
        p, e = F.auto_path(A, n_live, ef)
        ef_need = -(-ef * n_live // A)
        ew = min(4096, max(ef, ef_need))
        assert (p == F.EXACT) == (ef_need > 4096 or A <= 32 * ew)
    assert F.auto_path(10, 10_000, 64, F.WALK) == (F.WALK, 64)
    assert F.auto_path(10_000, 10_000, 64, F.EXACT) == (F.EXACT, 0)
