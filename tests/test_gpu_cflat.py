"""experimental CFLAT (multi-vector weighted FLAT scan) on the GPU vs the oracle restatement: bit-exact ids, ranks, scores."""
import numpy as np
import pytest

from oracle import oracle as O
from util import assert_same_results

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_cflat_search_parity(gpu, metric):
    n, d, nf = 1500, 64, 3
    X = O.fill_normal(51, (n, nf, d)); ids = np.arange(n, dtype=np.uint64) * np.uint64(7) + np.uint64(2)
    oc = O.CFlat(d, nf, metric); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(d, nf, metric); gc.ChangedVertex(ids, X)
    assert gc.Len() == n
    Q = O.fill_normal(52, (6, nf, d))
    for ratios, inc in (([50, 30, 20], [1, 1, 1]), ([100, 0, 40], [1, 0, 1]), ([33, 33, 34], [0, 1, 0])):
        for k in (1, 10, 50):
            gi, gs, gcnt = gc.MultiVertexSearch(k, Q, ratios, inc)
            for qi in range(len(Q)):
                wi, ws = oc.search(Q[qi], ratios, inc, k)
                assert_same_results(gi[qi, :gcnt[qi]], gs[qi, :gcnt[qi]], wi, ws, f"q{qi} r{ratios} k{k}")
    # overwrite + remove keep matching
    up = O.fill_normal(53, (40, nf, d)); oc.upsert(ids[100:140], up); gc.ChangedVertex(ids[100:140], up)
    rm = np.concatenate([ids[300:360], np.array([10**9], np.uint64)]); oc.remove(rm); gc.RemoveVertex(rm)
    assert gc.Len() == n - 60
    gi, gs, gcnt = gc.MultiVertexSearch(20, Q, [60, 25, 15])
    for qi in range(len(Q)):
        wi, ws = oc.search(Q[qi], [60, 25, 15], [1, 1, 1], 20)
        assert_same_results(gi[qi, :gcnt[qi]], gs[qi, :gcnt[qi]], wi, ws)
    e = gpu.MultiVectorSpace(d, nf, metric)
    assert e.MultiVertexSearch(5, Q[:1], [1, 1, 1])[2][0] == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# Everything below compares with O.CFlat exactly (ids, order, f32 score bits).  O.CFlat itself is held against an independent pure-Python
# restatement and a committed record on the CPU (tests/test_cflat_ref.py).
# ------------------------------------------------------------------------------------------------------------------------------------
import os

from coltt_amd._lib import ColttError
from coltt_amd.cflat import K_MAX
from util import cflat_ratio_sets, cflat_scaled_rows

GOLD = os.path.join(os.path.dirname(__file__), "golden", "cflat.npz")


def perm_ids(n):
    """a permutation of ids: id order differs from slot order"""
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(11)) % np.uint64(1 << 40)


def check_search(gc, oc, Q, ratios, inc, k, want_count=None, msg=""):
    gi, gs, gcnt = gc.MultiVertexSearch(k, Q, ratios, inc)
    for qi in range(len(Q)):
        wi, ws = oc.search(Q[qi], ratios, inc, k)
        if want_count is not None:
            assert gcnt[qi] == want_count, f"{msg} q{qi}: count {gcnt[qi]} != {want_count}"
        assert_same_results(gi[qi, :gcnt[qi]], gs[qi, :gcnt[qi]], wi, ws, f"{msg} q{qi} r{ratios} inc{inc} k{k}")


# ---- a. widths and field counts: dim 4 is the scalar tail alone, dims = 4 (mod 8) run it in both lanes of a pair, 1 and 8 fields are
# the ends of the allowed range; n = 700 > 512 takes the radix path of the selection, k >= n returns everything
@pytest.mark.parametrize("nf,dim", [(1, 4), (1, 12), (2, 20), (3, 36), (8, 64), (3, 768)])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_cflat_widths_and_fields(gpu, metric, nf, dim):
    n = 700
    X = O.fill_normal(8000 + 10 * nf + dim, (n, nf, dim)); ids = perm_ids(n)
    if metric == O.L2:
        X = cflat_scaled_rows(X)      # distances below, around and far above 100: the clamp of scoreHelper and its exact zeros
    Q = O.fill_normal(8500 + 10 * nf + dim, (5, nf, dim))
    oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(dim, nf, metric); gc.ChangedVertex(ids, X)
    assert gc.Len() == n
    if metric == O.L2:   # the case is what it claims: for a single included field some rows clamp to +0 and some do not
        ratios, inc = cflat_ratio_sets(nf)[4]
        _, ws = oc.search(Q[0], ratios, inc, n)
        assert (ws == 0).sum() > 0 and (ws > 0).sum() > 0
    for ratios, inc in cflat_ratio_sets(nf):
        for k in (1, 10, 700, 900):
            check_search(gc, oc, Q, ratios, inc, k, want_count=min(k, n), msg=f"nf{nf} dim{dim}")
    gc.close()


# ---- b. query tiles above 48 KiB of LDS (64 KiB and 128 KiB): the kernel attribute must take effect; a refused launch is an error
@pytest.mark.parametrize("nf,dim", [(8, 2048), (8, 4096)])
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_cflat_large_query_tile(gpu, metric, nf, dim):
    n, k = 96, 10
    X = O.fill_normal(8800 + dim, (n, nf, dim)); ids = perm_ids(n); Q = O.fill_normal(8801 + dim, (2, nf, dim))
    oc = O.CFlat(dim, nf, metric); oc.upsert(ids, X)
    gc = gpu.MultiVectorSpace(dim, nf, metric); gc.ChangedVertex(ids, X)
    ratios, inc = cflat_ratio_sets(nf)[0]
    gi, gs, gcnt = gc.MultiVertexSearch(k, Q, ratios, inc)    # raises ColttError when the launch is refused
    assert (gcnt == k).all() and (gs > 0).all(), "an answer of zeros: the scan did not run"
    check_search(gc, oc, Q, ratios, inc, k, want_count=k, msg=f"tile {nf}x{dim}")
    gc.close()


# ---- c. the segment chain: n = 65 600 rows is one more segment than cap - min(k, cap / 2) = 65 526 (k = 10) or 63 488 (k = 2048) rows
SEG_N = 65600


def seg_len(k):
    cap = max(65536, 8 * k)
    return cap - min(k, cap // 2)


@pytest.fixture(scope="module")
def chain(gpu):
    """ONE store for every segment-chain case (the upsert path is one vertex and one stream sync per row: this build is most of the
    time spent here).  L2, one field, dim 8.  Row of slot i = scale_i * (base + jitter_i): base is one Gaussian direction, scale_i grows
    linearly from 1 to 3 with the slot, jitter_i is Gaussian at 3e-5 (about the step of the scale between neighbouring slots, so score
    order and slot order differ locally, and both differ from id order).  The rows lie along a ray, so a query picks WHERE along the
    slots its winners are:
      origin              distance = scale_i * |base + jitter_i| grows with the slot: the winners are the first slots
      3 * base            distance ~ (3 - scale_i) * |base| falls with the slot: the winners are the last slots
      scale_b * base + g  winners on both sides of slot b
      1e3 * ones          every distance is above 100: every score is +0
    Independent Gaussian rows could not do this: no query makes all of the last 74 of them beat the best 10 of the 65 526 before."""
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

    def oracle_scores_by_slot(q):
        wi, ws = oc.search(q, [100], [1], n)
        out = np.empty(n, np.float32); out[[slot_of[int(v)] for v in wi]] = ws
        return out
    yield dict(gc=gc, oc=oc, ids=ids, base=base, scale=scale, slot_of=slot_of, by_slot=oracle_scores_by_slot)
    gc.close()


def chain_check(chain, q, k):
    q = np.asarray(q, np.float32).reshape(1, 1, -1)
    check_search(chain["gc"], chain["oc"], q, [100], [1], k, want_count=k, msg=f"chain k{k}")
    wi, _ = chain["oc"].search(q[0], [100], [1], k)
    return np.array([chain["slot_of"][int(v)] for v in wi])      # slots of the winners


@pytest.mark.parametrize("k", [10, 2048])
def test_cflat_chain_winners_on_both_sides(chain, k):
    """query = scale_b * base + a small Gaussian across the ray, b the first slot of the second segment: the second segment holds rows better AND worse than the
    carried threshold, and the answer mixes survivors of the first segment with new rows; plus a plain Gaussian query"""
    b = seg_len(k)
    assert 0 < b < SEG_N < 2 * b
    base = chain["base"]; g = O.fill_normal(9010 + k, (8,))
    g = g - (np.dot(g, base) / np.dot(base, base)) * base        # across the ray: it moves no winner along the slots
    slots = chain_check(chain, (chain["scale"][b - 1] + chain["scale"][b]) / np.float32(2) * base + np.float32(1e-4) * g, k)
    assert (slots < b).sum() > 0 and (slots >= b).sum() > 0, "the case is empty: every winner is in one segment"
    assert (slots >= b).sum() < SEG_N - b, "the second segment must also hold losers"
    chain_check(chain, O.fill_normal(9020 + k, (8,)), k)


@pytest.mark.parametrize("k", [10, 2048])
def test_cflat_chain_first_segment_wins(chain, k):
    """query at the origin: the score falls with the slot, the first segment holds every winner and the second must add nothing"""
    slots = chain_check(chain, np.zeros(8, np.float32), k)
    assert slots.max() < seg_len(k)


@pytest.mark.parametrize("k", [10, 2048])
def test_cflat_chain_second_segment_beats_threshold(chain, k):
    """query = 3 * base: the best rows are the LAST slots; every row of the second segment beats the threshold the first one hands over"""
    q = np.float32(3) * chain["base"]
    b = seg_len(k)
    sc = chain["by_slot"](q)
    carried = np.sort(sc[:b])[-k]                       # the k-th best score of the first segment
    assert sc[b:].min() > carried, "the case is not what it claims"
    slots = chain_check(chain, q, k)
    assert (slots >= b).sum() == min(k, SEG_N - b)


@pytest.mark.parametrize("k", [10, 2048])
def test_cflat_chain_all_tie(chain, k):
    """query = 1e3 * ones: every distance is above 100, every score is exactly +0 and all 65 600 rows tie with the carried threshold; the
    winners are the k largest ids, descending — the id radix-select across a segment boundary"""
    q = np.full(8, 1e3, np.float32)
    wi, ws = chain["oc"].search(q, [100], [1], SEG_N)
    assert len(ws) == SEG_N and not ws.view(np.uint32).any(), "the case is not what it claims: some score is not +0"
    gi, gs, gcnt = chain["gc"].MultiVertexSearch(k, q.reshape(1, 1, 8), [100], [1])
    assert gcnt[0] == k
    assert_same_results(gi[0], gs[0], np.sort(chain["ids"])[::-1][:k], np.zeros(k, np.float32), f"all tie k{k}")
    chain_check(chain, q, k)


# ---- d. store bookkeeping against a Python dict and an oracle kept in step
def test_cflat_bookkeeping(gpu):
    nf, dim, k = 2, 16, 25
    Q = O.fill_normal(9100, (4, nf, dim)); ratios, inc = [70, 30], [1, 1]
    oc = O.CFlat(dim, nf, O.COSINE); gc = gpu.MultiVectorSpace(dim, nf, O.COSINE)
    model = {}
    seed = [9101]

    def upsert(ids):
        ids = np.asarray(ids, np.uint64); seed[0] += 1
        V = O.fill_normal(seed[0], (len(ids), nf, dim))
        gc.ChangedVertex(ids, V); oc.upsert(ids, V)
        for i, v in zip(ids.tolist(), V):
            model[i] = v                                   # the last of a repeated id wins

    def remove(ids):
        ids = np.asarray(ids, np.uint64)
        gc.RemoveVertex(ids); oc.remove(ids)
        for i in ids.tolist():
            model.pop(i, None)

    def check(step):
        assert gc.Len() == len(model), step
        check_search(gc, oc, Q, ratios, inc, k, want_count=min(k, len(model)), msg=step)
        if model:   # the oracle was kept in step: its best answer is a vertex of the model
            wi, _ = oc.search(Q[0], ratios, inc, 1)
            assert int(wi[0]) in model, step

    ids = perm_ids(2400)
    for a, b in ((0, 1100), (1100, 1700), (1700, 2400)):      # the capacity grows 1024 -> 1536 -> 2304 -> 3456 with the rows kept
        upsert(ids[a:b]); check(f"insert {a}:{b}")
    assert len(model) == 2400
    new = np.uint64(2**41 + 5)
    upsert([ids[7], ids[900], ids[7], new, ids[7], new]); check("repeated ids in one call")
    assert len(model) == 2401
    # `new` sits in the last slot; ids[5] is listed twice; 2**42 was never stored
    remove([new, ids[5], ids[5], np.uint64(2**42)]); check("remove last slot, an id twice, an unknown id")
    assert len(model) == 2399
    remove(ids[2390:2400]); remove(ids[100:130]); check("more removes")          # swap-removes free slots in the middle
    upsert(np.concatenate([[new, ids[5]], ids[100:130], ids[2390:2400]])); check("re-insert removed ids")
    assert len(model) == 2401
    remove(np.fromiter(model.keys(), np.uint64))
    assert len(model) == 0 and gc.Len() == 0
    gi, gs, gcnt = gc.MultiVertexSearch(k, Q, ratios, inc)
    assert (gcnt == 0).all()
    upsert(ids[40:50]); check("ten rows into the emptied store")
    gc.close()


# ---- e. the committed record, made from the pure-Python restatement alone
@pytest.mark.parametrize("metric", [O.COSINE, O.L2])
def test_cflat_equals_golden(gpu, metric):
    g = np.load(GOLD)
    X = g["x_bits"].view(np.float32); Q = g["q_bits"].view(np.float32); k = int(g["k"][0])
    gc = gpu.MultiVectorSpace(X.shape[2], X.shape[1], metric); gc.ChangedVertex(g["ids"], X)
    for si in range(len(g["ratios"])):
        gi, gs, gcnt = gc.MultiVertexSearch(k, Q, g["ratios"][si], g["include"][si])
        for qi in range(len(Q)):
            assert gcnt[qi] == k
            assert_same_results(gi[qi], gs[qi], g[f"ids_{metric}_{si}"][qi], g[f"scores_{metric}_{si}"][qi].view(np.float32), f"metric {metric} set {si} q{qi}")
    gc.close()


# ---- f. what the wrapper and the library refuse
def test_cflat_validation(gpu):
    nf, dim = 3, 8
    gc = gpu.MultiVectorSpace(dim, nf, O.COSINE)
    ids = np.arange(4, dtype=np.uint64); X = O.fill_normal(9200, (4, nf, dim)); q = O.fill_normal(9201, (1, nf, dim))
    gc.ChangedVertex(ids, X)
    for ratios, inc in (([50, 50], [1, 1, 1]), ([50, 30, 20, 10], [1, 1, 1]), ([50, 30, 20], [1, 1]), ([50, 30, 20], [1, 1, 1, 1]), ([], None)):
        with pytest.raises(ValueError):
            gc.MultiVertexSearch(2, q, ratios, inc)
    for bad in (X[:3], X[:, :2], X[:, :, :4], np.zeros((4, nf, dim + 4), np.float32), np.zeros(0, np.float32)):
        with pytest.raises(ValueError):
            gc.ChangedVertex(ids, bad)
    assert gc.Len() == 4
    for k in (0, K_MAX + 1):
        with pytest.raises(ColttError):
            gc.MultiVertexSearch(k, q, [50, 30, 20])
    assert gc.MultiVertexSearch(K_MAX, q, [50, 30, 20])[2][0] == 4
    for d_, nf_, metric in ((6, 3, O.COSINE), (0, 3, O.COSINE), (8, 0, O.COSINE), (8, 9, O.COSINE), (8, 3, 2), (8, 3, -1)):
        with pytest.raises(ColttError):
            gpu.MultiVectorSpace(d_, nf_, metric)
    gc.close()
