"""The frozen-graph replay (insert_replay_ref.py) against the oracle's batched Insert, on the CPU: for a graph G0 and one batch of level-0
vectors, the replay fed with Hnsw.Search(k = m, ef = efConstruction) on G0 gives the oracle's graph after insert_batched, bit for bit —
own rows, back rows (overflow, tombstoned neighbours, more than 128 requests for one row), everything else unchanged.  This pins the definition
test_gpu_build_parity.py holds the GPU builder against where the oracle's f32 index cannot go."""
import numpy as np
import pytest

from oracle import oracle as O
import insert_replay_ref as R

# metric, dim, m, n0, B, efConstruction, removes before the batch, seed of the vectors, seed of the levels
CASES = [
    pytest.param(O.COSINE, 32, 16, 1000, 400, 64, 0, 11, 12, id="cosine-32d-m16"),
    pytest.param(O.L2, 24, 4, 1000, 400, 40, 0, 21, 22, id="l2-24d-m4"),
    pytest.param(O.L2, 16, 32, 800, 600, 100, 0, 1, 2, id="l2-16d-m32-fan-in"),
    pytest.param(O.COSINE, 32, 16, 1200, 400, 64, 300, 31, 32, id="cosine-32d-m16-tombstones"),
    pytest.param(O.L2, 16, 32, 1100, 600, 100, 300, 41, 42, id="l2-16d-m32-tombstones"),
]


def _g0(metric, d, m, n0, B, efc, removes, sx, sl):
    X = O.fill_normal(sx, (n0 + B, d)); lv = O.levels(sl, n0 + B, m); lv[n0:] = 0
    ids = np.arange(n0 + B, dtype=np.uint64) * np.uint64(5) + np.uint64(3)
    oh = O.Hnsw(d, metric, O.default_cfg(m=m, efConstruction=efc))
    oh.insert_batched(ids[:n0], X[:n0], lv[:n0], 0, schedule=lambda i: max(1, min(128, i // 16)))
    rng = np.random.default_rng(sx)
    for v in rng.choice(n0, removes, replace=False):
        assert oh.remove(ids[v]) == 0
    return X, lv, ids, oh


@pytest.mark.parametrize("metric,d,m,n0,B,efc,removes,sx,sl", CASES)
def test_replay_equals_oracle_batched_insert(metric, d, m, n0, B, efc, removes, sx, sl):
    X, lv, ids, oh = _g0(metric, d, m, n0, B, efc, removes, sx, sl)
    g0 = oh.export(with_vectors=False)
    slot_of = {int(v): s for s, v in enumerate(g0["ids"])}
    sl_ = np.zeros((B, m), np.int32); sc_ = np.zeros((B, m), np.float32); cn_ = np.zeros(B, np.int32)
    for b in range(B):
        wi, ws = oh.search(X[n0 + b], m, mode=1, ef=efc)
        cn_[b] = len(wi); sl_[b, :len(wi)] = [slot_of[int(v)] for v in wi]; sc_[b, :len(wi)] = ws
    want, book = R.replay_insert_batch(g0, ids[n0:], sl_, sc_, cn_, m, oh.cfg.mMax0)
    oh.insert_batched(ids[n0:], X[n0:], lv[n0:], B)
    g1 = oh.export(with_vectors=False)
    for k in ("ids", "levels", "deleted", "row_offsets", "nbr"):
        assert np.array_equal(want[k], g1[k]), k
    assert np.array_equal(want["nbr_dist"].view(np.uint32), g1["nbr_dist"].view(np.uint32)), "edge distances"
    assert want["entry"] == g1["entry"]
    # the counts read off the oracle's exports are the replay's own
    seen = R.link_bookkeeping(g0, g1, oh.cfg.mMax0, oh.cfg.mMax)
    assert seen == {k: book[k] for k in seen}, (seen, book)
    print(f"replay bookkeeping: {book}")
    # the cases are not vacuous
    assert book["full_own_rows"] == B
    assert book["overflow"] >= 50, book
    if removes:
        assert book["overflow_with_tombstone"] >= 5, book
    if m == 32 and not removes:
        assert book["max_fan_in"] > 128, book      # the link kernel merges such a row in three rounds


def test_prune_row_rule():
    """the back-row rule on a hand-made row: fits -> union; overflows -> tombstoned targets leave, then the nearest stay, the slot breaking ties"""
    dele = np.zeros(20, np.uint8); dele[[2, 9]] = 1
    s, d, over, tie = R.prune_row([1, 2, 5], [.3, .1, .2], dele, 4)
    assert s.tolist() == [1, 2, 5] and not over and not tie                      # a tombstoned target stays while the row fits
    s, d, over, tie = R.prune_row([1, 2, 5, 9, 12], [.3, .1, .2, .05, .4], dele, 4)
    assert s.tolist() == [1, 5, 12] and over and not tie                         # overflow: both tombstones leave, nothing else has to
    s, d, over, tie = R.prune_row([1, 3, 5, 7, 12, 15], [.3, .5, .2, .5, .4, .5], dele, 4)
    assert s.tolist() == [1, 3, 5, 12] and d.tolist() == np.float32([.3, .5, .2, .4]).tolist() and over and tie   # 3, 7, 15 tie: the lowest slot stays
    assert R.del_bits(np.r_[np.zeros(33, np.uint8), 1]).tolist() == [0, 2]
