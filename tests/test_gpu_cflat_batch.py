"""The multi-vector scan for a batch of requests (coltt_cflat_search_batch), the bulk upsert behind ChangedVertex and GetVertex, on the GPU.
Every comparison is exact (count, ids, order, f32 score bits): against O.CFlat request by request and, where stated, against the
single-request call MultiVertexSearch on the same store."""
import os

import numpy as np
import pytest

from coltt_amd._lib import ColttError
from coltt_amd.cflat import K_MAX
from cflat_ref import CFlatRef
from oracle import oracle as O
from oracle import pyref as P
from util import assert_same_results, cflat_ratio_sets, cflat_scaled_rows

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cflat.npz")


def perm_ids(n):
    """a permutation of ids: id order differs from slot order (restated from test_gpu_cflat.py)"""
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(11)) % np.uint64(1 << 40)


def mixed_requests(nq, nf):
    """request i takes cflat_ratio_sets(nf)[i % 5]: all included, ratio 0, ratio 250, all excluded, one field only"""
    sets = cflat_ratio_sets(nf)
    r = np.array([sets[i % 5][0] for i in range(nq)], np.uint32).reshape(nq, nf)
    inc = np.array([sets[i % 5][1] for i in range(nq)], np.uint8).reshape(nq, nf)
    return r, inc


def check_batch(gc, oc, Q, R, INC, k, want_count=None, single=True, msg="", want=None):
    """the batch call against the oracle (and the single-request call) for every request; `want` caches the oracle's answers"""
    gi, gs, gcnt = gc.MultiVertexSearchBatch(k, Q, R, INC)
    for i in range(len(Q)):
        m = f"{msg} request {i} r{R[i].tolist()} inc{INC[i].tolist()} k{k}"
        if want_count is not None:
            assert gcnt[i] == want_count, f"{m}: count {gcnt[i]} != {want_count}"
        key = (i, k)
        if want is None or key not in want:
            w = oc.search(Q[i], R[i], INC[i], k)
            if want is not None:
                want[key] = w
        else:
            w = want[key]
        assert_same_results(gi[i, :gcnt[i]], gs[i, :gcnt[i]], w[0], w[1], m + " vs oracle")
        if single:
            si, ss, sc = gc.MultiVertexSearch(k, Q[i], R[i], INC[i])
            assert_same_results(gi[i, :gcnt[i]], gs[i, :gcnt[i]], si[0, :sc[0]], ss[0, :sc[0]], m + " vs single call")
    return gi, gs, gcnt


# ---- a. group tails and mixed masks: one group, a partial last group and several groups for any group width up to 16; one group mixes
# all-included, ratio 0, ratio 250, all-excluded and single-field requests
@pytest.mark.parametrize("nf,dim", [(1, 4), (2, 20), (3, 36), (8, 64), (3, 768)])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_batch_group_tails_and_mixed_masks(gpu, metric, nf, dim):
    n = 700
    X = O.fill_normal(8000 + 10 * nf + dim, (n, nf, dim)); ids = perm_ids(n)
    if metric == O.L2:
        X = cflat_scaled_rows(X)
    Q = O.fill_normal(8600 + 10 * nf + dim, (17, nf, dim)); R, INC = mixed_requests(17, nf)
    oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(dim, nf, metric); gc.ChangedVertex(ids, X)
    assert gc.Len() == n
    if metric == O.L2:   # the clamp of scoreHelper fires for some rows only
        _, ws = oc.search(Q[4], R[4], INC[4], n)
        assert (ws == 0).sum() > 0 and (ws > 0).sum() > 0
    want = {}
    for nq in (17, 9, 7, 2, 1):      # request i is the same in every batch: the oracle answers once, the single call is made once
        for k in (1, 10, 700, 900):
            check_batch(gc, oc, Q[:nq], R[:nq], INC[:nq], k, want_count=min(k, n), single=(nq == 17), msg=f"nf{nf} dim{dim} nq{nq}", want=want)
    gc.close()


# ---- b. what an excluded field holds never reaches the score
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_batch_poison_in_excluded_fields(gpu, metric):
    n, nf, dim = 700, 3, 36
    X = O.fill_normal(8700, (n, nf, dim)); ids = perm_ids(n)
    if metric == O.L2:
        X = cflat_scaled_rows(X)
    oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(dim, nf, metric); gc.ChangedVertex(ids, X)
    nq = 17
    Q = O.fill_normal(8701, (nq, nf, dim)); R, INC = mixed_requests(nq, nf)
    poisoned = 0
    for i in range(nq):
        for f in range(nf):
            if not INC[i, f]:
                Q[i, f, :] = np.nan; Q[i, f, (i + f) % dim] = np.inf; poisoned += 1
    assert poisoned > 0
    for k in (10, 700):
        gi, gs, gcnt = check_batch(gc, oc, Q, R, INC, k, want_count=k, msg="poison")
        assert np.isfinite(gs).all()
    # every request all-excluded: every row ties at +0, the winners are the k largest ids, descending
    k = 10
    R0 = np.tile(np.array(cflat_ratio_sets(nf)[3][0], np.uint32), (5, 1)); INC0 = np.zeros((5, nf), np.uint8)
    Q0 = np.full((5, nf, dim), np.nan, np.float32); Q0[:, :, 3] = np.inf
    gi, gs, gcnt = gc.MultiVertexSearchBatch(k, Q0, R0, INC0)
    for i in range(5):
        assert gcnt[i] == k
        assert_same_results(gi[i], gs[i], np.sort(ids)[::-1][:k], np.zeros(k, np.float32), f"all excluded {i}")
        assert not gs[i].view(np.uint32).any()
    gc.close()


# ---- c. partial row groups and tiny stores
@pytest.mark.parametrize("n", [0, 1, 31, 33])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_batch_tiny_stores(gpu, metric, n):
    nf, dim, nq, k = 3, 36, 5, 10
    X = O.fill_normal(8800 + n, (max(n, 1), nf, dim))[:n]; ids = perm_ids(max(n, 1))[:n]
    Q = O.fill_normal(8810 + n, (nq, nf, dim)); R, INC = mixed_requests(nq, nf)
    oc = O.CFlat(dim, nf, metric); gc = gpu.MultiVectorSpace(dim, nf, metric)
    if n:
        oc.upsert(ids, X); gc.ChangedVertex(ids, X)
    assert gc.Len() == n
    check_batch(gc, oc, Q, R, INC, k, want_count=min(k, n), single=n > 0, msg=f"n{n}")
    gc.close()


# ---- d. tile budget edges: the largest query tile that still shares a pass over the rows, the next size up, and the 128 KiB request
# that must go through the single-request kernel inside the batch call
@pytest.mark.parametrize("nf,dim", [(8, 1024), (8, 2048), (8, 4096)])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_batch_tile_budget_edges(gpu, metric, nf, dim):
    n, nq, k = 96, 3, 10
    X = O.fill_normal(8900 + dim, (n, nf, dim)); ids = perm_ids(n); Q = O.fill_normal(8901 + dim, (nq, nf, dim))
    sets = cflat_ratio_sets(nf)
    R = np.array([sets[0][0], sets[2][0], sets[1][0]], np.uint32); INC = np.ones((nq, nf), np.uint8)
    oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(dim, nf, metric); gc.ChangedVertex(ids, X)
    gi, gs, gcnt = gc.MultiVertexSearchBatch(k, Q, R, INC)     # raises ColttError when a launch is refused
    assert (gcnt == k).all() and (gs > 0).all(), "an answer of zeros: the scan did not run"
    check_batch(gc, oc, Q, R, INC, k, want_count=k, msg=f"tile {nf}x{dim}")
    gc.close()


# ---- e. the segment chain with different winners in one group: n = 65 600 rows is one more segment than cap - min(k, cap / 2)
SEG_N = 65600


def seg_len(k):
    cap = max(65536, 8 * k)
    return cap - min(k, cap // 2)


@pytest.fixture(scope="module")
def ray(gpu):
    """the ray store of test_gpu_cflat.py's `chain` fixture, rebuilt here: L2, one field, dim 8, row of slot i = scale_i * (base + 3e-5 *
    jitter_i) with scale_i growing from 1 to 3 with the slot; a query picks WHERE along the slots its winners are"""
    n, dim = SEG_N, 8
    base = O.fill_normal(9001, (dim,))
    scale = (1.0 + 2.0 * np.arange(n, dtype=np.float64) / (n - 1)).astype(np.float32)
    X = (scale[:, None] * (base[None, :] + np.float32(3e-5) * O.fill_normal(9002, (n, dim)))).astype(np.float32).reshape(n, 1, dim)
    ids = perm_ids(n)
    assert len(np.unique(ids)) == n and not np.array_equal(np.argsort(ids), np.arange(n))
    oc = O.CFlat(dim, 1, O.L2); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(dim, 1, O.L2); gc.ChangedVertex(ids, X)
    assert gc.Len() == n
    slot_of = {int(v): i for i, v in enumerate(ids)}
    yield dict(gc=gc, oc=oc, ids=ids, base=base, scale=scale, slot_of=slot_of)
    gc.close()


@pytest.mark.parametrize("k", [10, 2048])
def test_batch_chain_different_winners_in_one_group(ray, k):
    """one group: winners in the first slots, in the last slots, on both sides of the segment boundary, and an all-tie; each request
    carries its OWN threshold over the boundary"""
    gc, oc, base, scale, slot_of = ray["gc"], ray["oc"], ray["base"], ray["scale"], ray["slot_of"]
    b = seg_len(k)
    assert 0 < b < SEG_N < 2 * b
    g = O.fill_normal(9010 + k, (8,)); g = g - (np.dot(g, base) / np.dot(base, base)) * base      # across the ray
    Q = np.stack([np.zeros(8, np.float32), np.float32(3) * base,
                  (scale[b - 1] + scale[b]) / np.float32(2) * base + np.float32(1e-4) * g, np.full(8, 1e3, np.float32)]).astype(np.float32).reshape(4, 1, 8)
    R = np.full((4, 1), 100, np.uint32); INC = np.ones((4, 1), np.uint8)
    gi, gs, gcnt = check_batch(gc, oc, Q, R, INC, k, want_count=k, single=False, msg=f"chain k{k}")
    slots = [np.array([slot_of[int(v)] for v in gi[i]]) for i in range(4)]
    # origin: the score falls with the slot, the first segment holds every winner
    assert slots[0].max() < b
    # 3 * base: every row of the second segment beats the threshold the first one hands over
    wi, ws = oc.search(Q[1], R[1], INC[1], SEG_N)
    sc = np.empty(SEG_N, np.float32); sc[[slot_of[int(v)] for v in wi]] = ws
    assert sc[b:].min() > np.sort(sc[:b])[-k], "the case is not what it claims"
    assert (slots[1] >= b).sum() == min(k, SEG_N - b)
    # the midpoint: winners on both sides, and the second segment also holds losers
    assert (slots[2] < b).sum() > 0 and (slots[2] >= b).sum() > 0, "the case is empty: every winner is in one segment"
    assert (slots[2] >= b).sum() < SEG_N - b
    # 1e3 * ones: all 65 600 rows tie at +0; the winners are the k largest ids, descending
    wi, ws = oc.search(Q[3], R[3], INC[3], SEG_N)
    assert len(ws) == SEG_N and not ws.view(np.uint32).any(), "the case is not what it claims: some score is not +0"
    assert_same_results(gi[3], gs[3], np.sort(ray["ids"])[::-1][:k], np.zeros(k, np.float32), f"all tie k{k}")
    assert not gs[3].view(np.uint32).any()
    # the same requests one at a time: the single-request chain agrees
    for i in range(4):
        si, ss, sc_ = gc.MultiVertexSearch(k, Q[i], R[i], INC[i])
        assert_same_results(gi[i], gs[i], si[0, :sc_[0]], ss[0, :sc_[0]], f"chain k{k} request {i} vs single call")


# ---- f. bulk upsert and read-back
def test_bulk_upsert_and_get_vertex(gpu):
    nf, dim, k = 2, 16, 25
    oc = O.CFlat(dim, nf, O.COSINE); ref = CFlatRef(dim, nf, O.COSINE); gc = gpu.MultiVectorSpace(dim, nf, O.COSINE)
    pool = perm_ids(3000)
    old = pool[:200]; V0 = O.fill_normal(9300, (200, nf, dim))
    for s in (oc, ref):
        s.upsert(old, V0)
    gc.ChangedVertex(old, V0)
    # one call of 3 000 rows: 2 650 new ids, the 200 stored ones, and 150 repeats (5 %) of ids of this call at later positions, each
    # occurrence with vectors of its own
    rng = np.random.default_rng(9301)
    first = np.concatenate([pool[200:2850], old])
    rep = rng.choice(first, 150, replace=False)
    call = np.concatenate([first, rep])[rng.permutation(3000)]     # the repeats lie anywhere, before and after their twins
    assert len(call) == 3000 and len(np.unique(call)) == 2850
    V = O.fill_normal(9302, (3000, nf, dim))
    for s in (oc, ref):
        s.upsert(call, V)
    gc.ChangedVertex(call, V)                                        # 200 -> 2 850 rows: past the capacity steps 1 024, 1 536 and 2 304
    assert gc.Len() == len(ref) == 2850
    lastpos = {int(v): i for i, v in enumerate(call)}
    for id_, fields in ref.v.items():
        got = gc.GetVertex(id_)
        assert np.array_equal(got.view(np.uint32), np.stack(fields).view(np.uint32)), id_
    for id_ in (int(call[0]), int(rep[0]), int(rep[77]), int(old[3])):      # the last occurrence is what is stored, as pyref.normalize bits
        want = np.stack([P.normalize(V[lastpos[id_], f].copy()) for f in range(nf)])
        assert np.array_equal(gc.GetVertex(id_).view(np.uint32), want.view(np.uint32))
    with pytest.raises(ColttError):
        gc.GetVertex(2**50 + 1)
    rm = np.concatenate([call[5:400:3], np.array([2**50 + 1], np.uint64)])
    for s in (oc, ref):
        s.remove(rm)
    gc.RemoveVertex(rm)
    assert gc.Len() == len(ref)
    with pytest.raises(ColttError):
        gc.GetVertex(int(rm[0]))
    nq = 9
    Q = O.fill_normal(9303, (nq, nf, dim)); R, INC = mixed_requests(nq, nf)
    check_batch(gc, oc, Q, R, INC, k, want_count=k, msg="after bulk upsert and removes")
    gc.close()


# ---- g. the committed record, made from the pure-Python restatement alone, through the batch call
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_batch_equals_golden(gpu, metric):
    g = np.load(GOLD)
    X = g["x_bits"].view(np.float32); Q = g["q_bits"].view(np.float32); k = int(g["k"][0])
    S = len(g["ratios"])
    gc = gpu.MultiVectorSpace(X.shape[2], X.shape[1], metric); gc.ChangedVertex(g["ids"], X)
    nreq = S * len(Q)                                  # request i: set i % S, query i // S
    BQ = np.stack([Q[i // S] for i in range(nreq)]); R = np.stack([g["ratios"][i % S] for i in range(nreq)]); INC = np.stack([g["include"][i % S] for i in range(nreq)])
    gi, gs, gcnt = gc.MultiVertexSearchBatch(k, BQ, R, INC)
    for i in range(nreq):
        si, qi = i % S, i // S
        assert gcnt[i] == k
        assert_same_results(gi[i], gs[i], g[f"ids_{metric}_{si}"][qi], g[f"scores_{metric}_{si}"][qi].view(np.float32), f"metric {metric} set {si} q{qi}")
    gc.close()


# ---- h. what the wrapper and the library refuse
def test_batch_validation(gpu):
    nf, dim = 3, 8
    gc = gpu.MultiVectorSpace(dim, nf, O.COSINE)
    ids = np.arange(4, dtype=np.uint64); X = O.fill_normal(9400, (4, nf, dim)); q = O.fill_normal(9401, (2, nf, dim))
    gc.ChangedVertex(ids, X)
    good = [[50, 30, 20], [10, 20, 30]]
    for ratios, inc in (([50, 30, 20], None), ([[50, 30], [10, 20]], None), ([[50, 30, 20]], None), (good + [[1, 2, 3]], None),
                        (good, [1, 1, 1]), (good, [[1, 1], [1, 1]]), (good, [[1, 1, 1]]), ([], None)):
        with pytest.raises(ValueError):
            gc.MultiVertexSearchBatch(2, q, ratios, inc)
    for k in (0, K_MAX + 1):
        with pytest.raises(ColttError):
            gc.MultiVertexSearchBatch(k, q, good)
    gi, gs, gcnt = gc.MultiVertexSearchBatch(K_MAX, q, good)
    assert (gcnt == 4).all()
    gi, gs, gcnt = gc.MultiVertexSearchBatch(5, np.zeros((0, nf, dim), np.float32), np.zeros((0, nf), np.uint32))
    assert gi.shape == (0, 5) and gs.shape == (0, 5) and gcnt.shape == (0,)
    gc.close()
