"""experimental CFLAT (multi-vector weighted scan) on the CPU: the C++ oracle (O.CFlat) against the independent pure-Python restatement
(tests/cflat_ref.py) and against the committed record made from that restatement (tests/golden/cflat.npz).  Ids, order and f32 score
bits are compared exactly.  No GPU needed."""
import os

import numpy as np
import pytest

import cflat_ref as R
from oracle import oracle as O
from util import assert_same_results, cflat_ratio_sets, cflat_scaled_rows

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cflat.npz")
N = 200
KS = (1, 7, 200, 250)


def _ids(n):
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(11)) % np.uint64(1 << 40)


@pytest.mark.parametrize("dim", [4, 12, 20, 64])
@pytest.mark.parametrize("nf", [1, 3, 8])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_oracle_equals_python_restatement(metric, nf, dim):
    """every ratio / include set and k in (1, 7, n, n + 50); for L2 the rows are scaled 1x / 6x / 50x and the clamp of scoreHelper must be
    seen both firing (score == 0) and not firing (score > 0).  With one included field the score IS that field's clamped term times a
    positive weight, so the count is taken there: with several included fields at dim 4 a row scores 0 only when every field clamps at
    once, which the 50x rows (distance about 50 * chi(4): around 100) need not do."""
    X = O.fill_normal(7000 + 10 * nf + dim, (N, nf, dim)); ids = _ids(N)
    if metric == O.L2:
        X = cflat_scaled_rows(X)
    q = O.fill_normal(7500 + 10 * nf + dim, (nf, dim))
    oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
    ref = R.CFlatRef(dim, nf, metric); ref.upsert(ids, X)
    for si, (ratios, inc) in enumerate(cflat_ratio_sets(nf)):
        ri, rs = ref.rank(q, ratios, inc)
        assert len(ri) == N
        for k in KS:
            wi, ws = oc.search(q, ratios, inc, k)
            assert len(wi) == min(k, N)
            assert_same_results(wi, ws, ri[:k], rs[:k], f"metric {metric} nf {nf} dim {dim} set {si} k {k}")
        if not any(inc):
            assert np.array_equal(rs.view(np.uint32), np.zeros(N, np.uint32)), "every field excluded: every score is +0"
            assert np.array_equal(ri, np.sort(ids)[::-1]), "all tie: descending id"
        if metric == O.L2 and si == 4:           # the one-included-field set (its ratio is not 0)
            assert (rs == 0).sum() > 0 and (rs > 0).sum() > 0, ((rs == 0).sum(), (rs > 0).sum())
    # an upsert that overwrites (one id twice in the call: the last wins) and a remove (one unknown id) keep the two sides together
    up_ids = np.concatenate([ids[20:50], ids[20:21]]); up = O.fill_normal(7900 + dim, (len(up_ids), nf, dim))
    oc.upsert(up_ids, up); ref.upsert(up_ids, up)
    rm = np.concatenate([ids[60:90], np.array([2**41], np.uint64)])
    oc.remove(rm); ref.remove(rm)
    assert len(ref) == N - 30
    ratios, inc = cflat_ratio_sets(nf)[0]
    ri, rs = ref.rank(q, ratios, inc)
    for k in (7, N):
        wi, ws = oc.search(q, ratios, inc, k)
        assert_same_results(wi, ws, ri[:k], rs[:k], f"after upsert + remove, k {k}")


def test_restatement_helpers():
    """scoreHelper and the weight at the values where a wrong reading shows: the clamp boundary, a ratio above 100, ratio 0"""
    f = np.float32
    assert R.score_helper(f(100), R.L2) == 0 and not np.signbit(R.score_helper(f(100), R.L2))
    assert R.score_helper(f(250), R.L2) == 0 and not np.signbit(R.score_helper(f(250), R.L2))
    assert R.score_helper(np.nextafter(f(100), f(0)), R.L2) == f(100) - np.nextafter(f(100), f(0)) > 0
    assert R.score_helper(f(0), R.COSINE) == 100 and R.score_helper(f(2), R.COSINE) == 0 and R.score_helper(f(1), R.COSINE) == 50
    assert R.weight(250) == f(2.5) and R.weight(0) == 0 and R.weight(30).view(np.uint32) == (f(30) / f(100)).view(np.uint32)


def test_oracle_equals_golden():
    g = np.load(GOLD)
    X = g["x_bits"].view(np.float32); Q = g["q_bits"].view(np.float32); ids = g["ids"]; k = int(g["k"][0])
    n, nf, dim = X.shape
    assert (n, nf, dim, len(Q), k) == (300, 3, 12, 4, 10)
    for metric in (O.COSINE, O.L2):
        oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
        for si in range(len(g["ratios"])):
            for qi in range(len(Q)):
                wi, ws = oc.search(Q[qi], g["ratios"][si], g["include"][si], k)
                assert_same_results(wi, ws, g[f"ids_{metric}_{si}"][qi], g[f"scores_{metric}_{si}"][qi].view(np.float32), f"metric {metric} set {si} q{qi}")


def test_golden_is_what_its_script_makes():
    """the committed record equals what make_golden_cflat.py computes today, array by array: neither the restatement nor the input
    generator has drifted from the file"""
    import sys
    sys.path.insert(0, os.path.dirname(GOLD))
    import make_golden_cflat as MG
    g = np.load(GOLD); now = MG.arrays()
    assert sorted(g.files) == sorted(now)
    for name in g.files:
        assert g[name].dtype == now[name].dtype and np.array_equal(g[name], now[name]), name
