"""The greedy descent of the 8-bit row-filter walks through the certified filter (COLTT_ROW_FILTER_UPPER; coltt_amd/csrc/hnsw_walk2.hpp:
greedy_level8_filtered) changes what the descent READS, never where it ends.  With the knob on, ids, score bits, counts, n_dist / n_exp / n_hops and the
three level-0 filter counters equal those with the knob off, those of COLTT_ROW_FILTER=0 and the oracle's canonical search over the arrays copied out of
HBM — bit equality — for both 8-bit kinds, both visited tables, both load hints (and the descent's own, COLTT_DESCENT_NT) and ef 32 / 128.  The descent's
own counters (RowFilterStats()["upper_*"]) show that the filter acted; its shares are printed, not asserted."""
import numpy as np
import pytest

import descent_filter_ref as D
import test_gpu_row_filter8 as T8
from oracle import oracle as O
from util import assert_same_results, bits

pytestmark = pytest.mark.gpu

KNOBS = T8.KNOBS + ("COLTT_ROW_FILTER_UPPER", "COLTT_DESCENT_NT", "COLTT_VIS16", "COLTT_ROWS_NT")
L0 = ("rejected", "f32_rows", "shadow_rows", "launches")
UP = ("upper_shadow_rows", "upper_rejected", "upper_f32_rows", "upper_launches")


@pytest.fixture(autouse=True)
def _throughput_kernels(monkeypatch):
    monkeypatch.setenv("COLTT_MW_MAX_NQ", "0")   # batches of any size on the one-wave-per-query kernels (the latency kernel is not filtered)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _run(gh, Q, k, ef, env):
    """one Search under `env`: (ids, scores, counts, traversal counters), the row filter's counter deltas, the visited table's kind"""
    with pytest.MonkeyPatch.context() as mp:
        for kk, v in env.items():
            mp.setenv(kk, v)
        a = gh.RowFilterStats()
        res = gh.Search(Q, k, ef=ef, with_stats=True)
        b = gh.RowFilterStats()
        kind = gh.VisitedStats()["kind"]
    return res, {kk: b[kk] - a[kk] for kk in L0 + UP}, kind


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def _check(gh, Q, efs, k=10, del_bits=None, deleted=None, gaussian=True):
    d = gh.dim
    g = gh.ExportRaw(); rows = gh.FetchRows()
    # evaluations above level 0, from the exact replay of the descent over the exported arrays
    upper_evals = 0; events = {}
    for q in Q:
        tr, ev, _ = D.descend(_Rows(rows), g["upper_off"], g["adjU"], g["entry"], g["entry_level"], O.normalize(q), deleted)
        upper_evals += tr[-1][3] - 1
        for kk, v in ev.items():
            events[kk] = events.get(kk, 0) + v
    for ef in efs:
        sl, sc, cn, ost, _ = O.csr_search(rows, O.Q_NONE, g["adj0"], g["upper_off"], g["adjU"], d, O.COSINE, g["entry"], g["entry_level"],
                                          Q, k, ef, del_bits=del_bits, threads=4)
        base, f0, _ = _run(gh, Q, k, ef, {"COLTT_ROW_FILTER": "0"})
        assert all(f0[kk] == 0 for kk in L0 + UP), "COLTT_ROW_FILTER=0 took a filtered launch"
        for qi in range(len(Q)):
            assert_same_results(base[0][qi, :base[2][qi]], base[1][qi, :base[2][qi]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], f"filter off, q{qi} ef{ef}")
        assert {k_: base[3][k_] for k_ in ost} == ost, (ef, base[3], ost)
        for nt in ("0", "1"):
            for kind in ("8", "8i"):
                for v16 in ("0", "1"):
                    env = {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": kind, "COLTT_ROWS_NT": nt, "COLTT_VIS16": v16}
                    off, foff, vk = _run(gh, Q, k, ef, dict(env, COLTT_ROW_FILTER_UPPER="0"))
                    tag = f"d{d} ef{ef} kind {kind} nt{nt} vis16={v16} (visited table {vk})"
                    assert foff["launches"] == 1 and all(foff[kk] == 0 for kk in UP), tag
                    assert _same(off, base), f"{tag}: knob off != filter off"
                    for dnt in (("1",) if nt == "0" else ("1", "0")):   # the descent's own hint matters to the non-temporal twins only
                        on, fon, vk2 = _run(gh, Q, k, ef, dict(env, COLTT_ROW_FILTER_UPPER="1", COLTT_DESCENT_NT=dnt))
                        assert vk2 == vk
                        assert _same(on, off), f"{tag} descent nt{dnt}: knob on != knob off"
                        assert {kk: fon[kk] for kk in L0} == {kk: foff[kk] for kk in L0}, (tag, fon, foff)
                        s, r, f = fon["upper_shadow_rows"], fon["upper_rejected"], fon["upper_f32_rows"]
                        assert fon["upper_launches"] == 1 and r + f == s, (tag, fon)
                        assert s == upper_evals, f"{tag}: {s} shadow rows above level 0, the exact replay counts {upper_evals} evaluations there"
                        if gaussian:
                            assert s > 0 and r > 0 and f < upper_evals, (tag, fon)
                    if nt == "0" and v16 == "1":
                        print(f"{tag}: {upper_evals} evaluations above level 0 ({upper_evals / len(Q):.1f} per query): rejected {r} ({100.0 * r / max(s, 1):.1f} %), f32 rows {f}")
    return events


class _Rows:
    """descent_filter_ref.descend needs .rows alone for the exact replay"""
    def __init__(self, rows):
        self.rows = rows


CASES = [(m, d) for m in (4, 16) for d in (256, 512, 768, 1536)]


@pytest.mark.parametrize("m,d", CASES, ids=[f"M{m}-d{d}" for m, d in CASES])
def test_knob_on_equals_knob_off_filter_off_and_the_oracle(gpu, m, d):
    """6 000 Gaussian rows, 48 queries, levels passed to the batched insert; M = 4: five or six levels (long descents), M = 16: wide hops; the four
    widths are the four forms of phase A (one burst of 2 lines | stream of bursts of 2 | one burst of 6 | stream of bursts of 6)"""
    n = 6000
    X = O.fill_normal(8600 + d + m, (n, d)); lv = O.levels(8601 + d + m, n, m=m)
    gh = T8._gpu_build(gpu, X, lv, gpu.HnswCfg.default(m=m, ef_construction=40), batch=512)
    assert 8 in gh.RowFilterStats()["shadow_bits"]
    assert gh.ExportRaw()["entry_level"] >= (4 if m == 4 else 2)
    Q = O.fill_normal(8602 + d + m, (48, d))
    _check(gh, Q, (32, 128))


def _nudge_to(qe, base, want_bits, rng, tries=12):
    """a nudged copy of the raw row `base` whose STORED form (Normalize) lies at exactly the distance want_bits from qe"""
    dim = base.size
    for _ in range(tries):
        C = np.tile(base, (1024, 1))
        j = rng.integers(0, dim, 1024); k = rng.integers(-4096, 4097, 1024)
        C[np.arange(1024), j] = (C[np.arange(1024), j].view(np.int32) + k.astype(np.int32)).view(np.float32)
        S = np.stack([O.normalize(c) for c in C])
        hit = np.flatnonzero(D.exact_distances(qe, S).view(np.uint32) == np.uint32(want_bits))
        if len(hit):
            return C[hit[0]].copy()
    raise AssertionError("no nudged copy of the row lands on the wanted distance")


def test_constructed_cases(gpu):
    """A few hundred rows with chosen levels.  Groups (A one level above its B's, the query near A): the descent arrives ON A and the first hop of the
    level below meets B at curd exactly (a duplicate: no move), one ulp below it (move), or two different rows at the same distance below it (the lower
    adjacency index wins).  A zero row and a row with a non-finite element sit among the neighbours on that level (no verdict: the exact path);
    fillers are tombstoned (skipped, not counted).  The exact replay over the exported arrays shows that the cases were met"""
    d = 256; seed = 8700
    rng = np.random.default_rng(seed)
    n_fill = 300
    unit = lambda X: np.stack([O.normalize(x) for x in np.ascontiguousarray(X, np.float32)])
    fill = unit(O.fill_normal(seed, (n_fill, d))); lvf = np.minimum(O.levels(seed + 1, n_fill, m=4), 2)
    As, Bs, Q = [], [], []
    for gi in range(5):
        A = unit(O.fill_normal(seed + 10 + gi, (1, d)))[0]
        q = A + O.fill_normal(seed + 40 + gi, (d,)) * np.float32(2.8 / np.sqrt(d))   # cos(q, A) about 0.34: d in (0.5, 1), where 1 - cos reaches EVERY f32
        qe = O.normalize(q)
        dA = D.exact_distances(qe, O.normalize(A)[None, :])[0]
        assert 0.5 < dA < 1.0
        if gi in (0, 3):
            B = [A.copy()]
        elif gi in (1, 4):
            B = [_nudge_to(qe, A, D.f32bits(dA) - 1, rng)]
        else:
            lo = D.f32bits(dA) - 3
            B = [_nudge_to(qe, A, lo, rng), _nudge_to(qe, A, lo, rng)]
            assert not np.array_equal(B[0], B[1])
        As.append(A); Bs += B; Q.append(q)
    bad = unit(O.fill_normal(seed + 90, (1, d))); bad[0, 5] = np.float32(np.inf)
    # the batched insert links a batch against the graph BEFORE it: the A's go in a hundred rows ahead of their B's
    rows = [fill[:200], np.stack(As), fill[200:], np.stack(Bs), np.zeros((1, d), np.float32), bad, unit(O.fill_normal(seed + 95, (1, d)))]
    lv = [lvf[:200], np.full(len(As), 4), lvf[200:], np.full(len(Bs), 3), np.array([3]), np.array([3]), np.array([5])]
    X = np.ascontiguousarray(np.concatenate(rows), np.float32); lv = np.concatenate(lv).astype(np.int32)
    is_fill = np.ones(len(X), bool); is_fill[200:200 + len(As)] = False; is_fill[n_fill + len(As):] = False
    gh = T8._gpu_build(gpu, X, lv, gpu.HnswCfg.default(m=16, ef_construction=40), batch=32)
    dead = rng.choice(np.flatnonzero(is_fill), 60, replace=False)
    for i in dead:
        gh.Remove(int(i))
    db = np.zeros((len(X) + 31) // 32, np.uint32); deleted = np.zeros(len(X), bool)
    for i in dead:
        db[i >> 5] |= np.uint32(1 << (i & 31)); deleted[i] = True
    g = gh.ExportRaw()
    assert g["entry"] == len(X) - 1 and g["entry_level"] == 5
    Q = np.ascontiguousarray(np.concatenate([np.stack(Q), O.fill_normal(seed + 96, (11, d))]), np.float32)
    ev = _check(gh, Q, (32,), del_bits=db, deleted=deleted, gaussian=False)
    print(f"constructed cases met by the exact replay: {ev}")
    assert ev["equal_no_move"] > 0 and ev["ulp_below_move"] > 0 and ev["tie_of_survivors"] > 0 and ev["tombstone"] > 0
    stored = gh.FetchRows()
    special = np.flatnonzero(~np.isfinite(stored).all(axis=1) | ~stored.any(axis=1))
    assert len(special) == 2, "a zero row and a row with a non-finite element are stored"
    listed = g["adjU"][np.concatenate([np.arange(int(g["upper_off"][v]), int(g["upper_off"][v]) + int(lv[v])) for v in np.flatnonzero(lv >= 3)])]
    assert np.isin(special, listed).all(), "the rows without a verdict are listed on the upper levels"


@pytest.mark.parametrize("shape", ["entry-level-0", "lone-upper-vertex"])
def test_nothing_to_descend_through(gpu, shape):
    """entry_level == 0 (every vertex on level 0: the prologue evaluates the entrypoint and walks), and an index whose only upper vertex is the
    entrypoint (one hop per level over an empty adjacency row)"""
    d, n = 256, 400
    X = O.fill_normal(8800, (n, d)); lv = np.zeros(n, np.int32)
    if shape == "lone-upper-vertex":
        lv[37] = 3
    gh = T8._gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=40), batch=32)
    g = gh.ExportRaw()
    assert g["entry_level"] == (0 if shape == "entry-level-0" else 3)
    _check(gh, O.fill_normal(8801, (16, d)), (32,), gaussian=False)
