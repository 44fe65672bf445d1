"""Filter expressions on the GPU (coltt_hnsw_filter_eval / _eval_batch / _ids / _info; include/coltt_gpu.h, "Filter expressions") against
the definition in numpy (tests/filter_expr_ref.py): the result of a programme over resident leaves is indistinguishable from
coltt_hnsw_filter_create over the set the definition computes — allowed count, id list, and every filtered search (ids, score bits, counts,
paths, stats).  Every comparison is exact.

Slot counts 1, 31, 32, 33, 1 000 and 70 001: one workgroup of the evaluate and compact kernels covers 1 024 bitmap words = 32 768 slots
(filter_expr.hpp: FEX_TILE_WORDS), so 70 001 slots span three workgroups of both with a ragged last word (70 001 = 2 187 words + 17 bits);
the read-back kernel's workgroups cover 256 ids each."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import filter_expr_ref as R

pytestmark = pytest.mark.gpu

K, D = 10, 64
A_, O_, X_, N_, T_ = R.AND, R.OR, R.ANDNOT, R.NOT, R.ALL
# leaves 0, 1, 2 = A (built early), B, C (built at the final size)
PROGS = [
    ("A B AND", [0, 1, A_]), ("A B OR", [0, 1, O_]), ("A B ANDNOT", [0, 1, X_]), ("A NOT", [0, N_]), ("ALL", [T_]),
    ("A B AND C OR", [0, 1, A_, 2, O_]), ("A B OR C ANDNOT", [0, 1, O_, 2, X_]), ("ALL A ANDNOT", [T_, 0, X_]),
    ("depth 8", [0, 1, 2, T_, 1, 0, 2, 1, A_, O_, X_, O_, A_, O_, X_]),
    ("one leaf repeated", [1, 1, A_, 1, O_, 1, X_, 1, O_]),
    ("empty result", [0, 0, X_]), ("all live", [0, N_, 0, O_]), ("C NOT NOT", [2, N_, N_]),
]


def _insert(gh, X, lv, lo, hi, ids=None, batch=512):
    import torch
    d = X.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(X[lo:hi])).cuda(); torch.cuda.synchronize()
    i = lo
    while i < hi:
        b = int(min(hi - i, max(1, min(batch, i // 16))))
        gh.InsertBatchDevice(xd.data_ptr() + (i - lo) * d * 4, b, lv[i:i + b], batch=b, first_id=i, ids=None if ids is None else ids[i:i + b])
        i += b


class Case:
    """an index grown in two stages with leaves of different ages, then removals: what the definition needs (stored leaf bits, live)"""

    def __init__(self, gpu, n, d=D, metric=None, quant=None, ids=False, n_early=None, seed=500):
        metric = O.L2 if metric is None else metric
        quant = O.Q_NONE if quant is None else quant
        self.n, self.d = n, d
        self.X = O.fill_normal(seed + n, (n, d)); lv = O.levels(seed + n + 1, n)
        self.ids = (np.arange(n, dtype=np.uint64) * 7 + 1000) if ids else None
        self.gh = gh = gpu.Hnsw(d, metric, quantization=quant)
        rng = np.random.default_rng(seed + n)
        n_early = n // 3 if n_early is None else n_early
        _insert(gh, self.X, lv, 0, n_early, self.ids)
        self.masks = [rng.random(n_early) < 0.5, rng.random(n) < 0.3, rng.random(n) < 0.05]
        if n <= 33:
            self.masks[2] = rng.random(n) < 0.5
        self.leaves = [gh.Filter(self.to_ids(np.nonzero(self.masks[0])[0]))]          # A: the index had n_early slots
        _insert(gh, self.X, lv, n_early, n, self.ids)
        self.leaves += [gh.Filter(self.to_ids(np.nonzero(m)[0])) for m in self.masks[1:]]   # B, C: n slots
        for f, m in zip(self.leaves, self.masks):
            assert f.allowed == int(m.sum()) and f.info() == {"index": gh.h.value, "allowed": int(m.sum()), "slots": len(m)}
        # removed after the leaves were built: slots in A only, in B only, in both, in neither (as far as the index has them)
        self.live = np.ones(n, bool)
        a = np.zeros(n, bool); a[:n_early] = self.masks[0]; b = self.masks[1]
        if n >= 31:
            for sel in (a & ~b, b & ~a, a & b, ~a & ~b):
                for s in np.nonzero(sel)[0][1:4]:
                    gh.Remove(int(self.to_ids(np.array([s]))[0]))
                    self.live[s] = False
        assert gh.Len() == int(self.live.sum())
        self.Q = O.fill_normal(seed + 7, (8, d))

    def to_ids(self, slots):
        slots = np.asarray(slots, np.int64)
        return slots.astype(np.uint64) if self.ids is None else self.ids[slots]

    def want(self, prog):
        return np.nonzero(R.evaluate(prog, self.masks, self.live))[0]


_CACHE = {}
KINDS = {"n1": dict(n=1), "n31": dict(n=31), "n32": dict(n=32), "n33": dict(n=33), "n1000": dict(n=1000),
         "n70001": dict(n=70001, n_early=20000), "ids1000": dict(n=1000, ids=True, seed=900),
         "f16_768d_1800": dict(n=1800, d=768, metric=O.COSINE, quant=O.Q_F16)}


def _case(gpu, kind):
    if kind not in _CACHE:
        _CACHE[kind] = Case(gpu, **KINDS[kind])
    return _CACHE[kind]


def _same_search(gpu, gh, Q, f, twin, modes_efs, what):
    for mode, ef in modes_efs:
        a = gh.SearchFiltered(Q, K, f, ef=ef, mode=mode, with_stats=True)
        b = gh.SearchFiltered(Q, K, twin, ef=ef, mode=mode, with_stats=True)
        assert np.array_equal(a[2], b[2]), (what, mode, ef)
        for qi in range(len(Q)):
            c = a[2][qi]
            assert np.array_equal(a[0][qi, :c], b[0][qi, :c]) and np.array_equal(bits(a[1][qi, :c]), bits(b[1][qi, :c])), (what, mode, ef, qi)
        assert a[3] == b[3], (what, mode, ef, a[3], b[3])


@pytest.mark.parametrize("kind", list(KINDS))
def test_every_programme_equals_filter_create_over_the_defined_set(gpu, kind):
    cs = _case(gpu, kind)
    gh = cs.gh
    modes = ((gpu.FILTER_WALK, 64), (gpu.FILTER_WALK, 256), (gpu.FILTER_EXACT, 0))
    for name, prog in PROGS:
        assert R.validate(prog, 3)[0] == R.OK
        want = cs.want(prog)
        if name == "empty result":
            assert len(want) == 0
        if name in ("all live", "ALL"):
            assert np.array_equal(want, np.nonzero(cs.live)[0])
        f = gh.FilterEval(prog, cs.leaves)
        twin = gh.Filter(cs.to_ids(want))
        assert f.allowed == twin.allowed == len(want), (kind, name, f.allowed, len(want))
        assert f.info() == twin.info() == {"index": gh.h.value, "allowed": len(want), "slots": cs.n}, (kind, name)
        got = f.ids()
        assert np.array_equal(got, cs.to_ids(want)) and np.array_equal(twin.ids(), got), (kind, name)
        _same_search(gpu, gh, cs.Q, f, twin, modes, (kind, name))
        a = gh.SearchFilteredBatch(cs.Q, K, [f] * len(cs.Q), ef=64, mode=gpu.FILTER_AUTO, with_stats=True)
        b = gh.SearchFilteredBatch(cs.Q, K, [twin] * len(cs.Q), ef=64, mode=gpu.FILTER_AUTO, with_stats=True)
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]) and a[4] == b[4], (kind, name)
        for qi in range(len(cs.Q)):
            c = a[2][qi]
            assert np.array_equal(a[0][qi, :c], b[0][qi, :c]) and np.array_equal(bits(a[1][qi, :c]), bits(b[1][qi, :c])), (kind, name, qi)
        f.close(); twin.close()


def test_tuple_expressions_and_later_inserts(gpu):
    """NOT and ALL see vertices inserted after their operand was built, AND / OR / ANDNOT of plain leaves do not"""
    cs = _case(gpu, "n70001")
    gh = cs.gh
    n_early = len(cs.masks[0])
    with gh.FilterEval(("not", 0), cs.leaves) as f:
        assert np.array_equal(f.ids()[-5:], np.nonzero(cs.live)[0][-5:].astype(np.uint64)) and f.ids().max() >= n_early
    with gh.FilterEval(("or", 0, 0), cs.leaves) as f:
        assert f.ids().max() < n_early
    with gh.FilterEval(("and", 0, ("or", 1, 2)), cs.leaves) as f:
        assert np.array_equal(f.ids(), cs.want([0, 1, 2, O_, A_]).astype(np.uint64))
    # refresh without a mutable filter: old  create(added) OR  create(dropped) ANDNOT
    old = cs.leaves[1]
    added = np.nonzero(cs.live & ~cs.masks[1])[0][:100]; dropped = np.nonzero(cs.live & cs.masks[1])[0][:100]
    with gh.Filter(added) as fa, gh.Filter(dropped) as fd, gh.FilterEval([0, 1, O_, 2, X_], [old, fa, fd]) as f:
        m = cs.masks[1].copy(); m[added] = True; m[dropped] = False
        assert np.array_equal(f.ids(), np.nonzero(m & cs.live)[0].astype(np.uint64))


def test_pq_search_equals_the_twin(gpu):
    cs = _case(gpu, "n1000")
    gh = cs.gh
    pq = gpu.PQSpace(D, gpu.PQ_EUCLIDEAN, 16, 32)
    pq.Fit(cs.X, iterations=2)
    gh.PqAttach(pq)
    for name, prog in PROGS:
        want = cs.want(prog)
        with gh.FilterEval(prog, cs.leaves) as f, gh.Filter(cs.to_ids(want)) as twin:
            for mode in (gpu.FILTER_AUTO, gpu.FILTER_WALK, gpu.FILTER_EXACT):
                a = gh.PqSearchFiltered(cs.Q, K, f, ef=64, mode=mode, with_stats=True)
                b = gh.PqSearchFiltered(cs.Q, K, twin, ef=64, mode=mode, with_stats=True)
                assert np.array_equal(a[2], b[2]) and a[3] == b[3], (name, mode, a[3], b[3])
                for qi in range(len(cs.Q)):
                    c = a[2][qi]
                    assert np.array_equal(a[0][qi, :c], b[0][qi, :c]) and np.array_equal(bits(a[1][qi, :c]), bits(b[1][qi, :c])), (name, mode, qi)
            a = gh.PqSearchFilteredBatch(cs.Q, K, [f] * len(cs.Q), ef=64)
            b = gh.PqSearchFilteredBatch(cs.Q, K, [twin] * len(cs.Q), ef=64)
            assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]), name


def _random_prog(rng, n_leaves):
    import coltt_amd
    while True:
        prog = coltt_amd.filter_postfix(R.random_tree(rng, n_leaves, int(rng.integers(1, 6))))
        if R.validate(prog, n_leaves)[0] == R.OK:
            return prog


def test_batch_eval_300_programmes_over_12_leaves(gpu):
    cs = _case(gpu, "n70001")
    gh = cs.gh
    rng = np.random.default_rng(31)
    masks = list(cs.masks) + [rng.random(cs.n) < p for p in (0.9, 0.5, 0.5, 0.2, 0.1, 0.02, 0.001, 0.0, 1.0)]
    leaves = list(cs.leaves) + [gh.Filter(np.nonzero(m)[0]) for m in masks[3:]]
    assert len(leaves) == 12
    progs = [_random_prog(rng, 12) for _ in range(300)]
    progs[7] = [0, 0, X_]; progs[8] = [T_]; progs[9] = [10]     # an empty result, all live, an empty leaf
    outs = gh.FilterEvalBatch(progs, leaves)
    assert len(outs) == 300 and len(set(f.h.value for f in outs)) == 300
    singles = {}
    for i, (prog, f) in enumerate(zip(progs, outs)):
        want = np.nonzero(R.evaluate(prog, masks, cs.live))[0].astype(np.uint64)
        assert f.allowed == len(want), (i, prog)
        assert np.array_equal(f.ids(), want), (i, prog)
        if i % 10 == 0:
            s = gh.FilterEval(prog, leaves)
            assert s.allowed == f.allowed and s.info() == f.info() and np.array_equal(s.ids(), want), i
            singles[i] = s
    for lf in leaves[3:]:
        lf.close()                       # the outputs outlive the leaves they were computed from
    modes = ((gpu.FILTER_WALK, 64), (gpu.FILTER_EXACT, 0))
    order = rng.permutation(300)
    alive = set(range(300))
    for j, i in enumerate(order):
        outs[i].close(); alive.discard(int(i))
        if j % 40 == 39 or j == 298:
            for s in sorted(alive & set(singles))[:2]:
                _same_search(gpu, gh, cs.Q, outs[s], singles[s], modes, ("survivor", s))
            rest = sorted(alive)
            for s in rest[:2]:
                want = np.nonzero(R.evaluate(progs[s], masks, cs.live))[0].astype(np.uint64)
                assert np.array_equal(outs[s].ids(), want), ("survivor", s)
    for s in singles.values():
        s.close()
    # n_out == 0 is not an error; a bad programme creates nothing and is named
    assert gh.FilterEvalBatch([], cs.leaves) == []
    with pytest.raises(gpu.ColttError) as e:
        gh.FilterEvalBatch([[0, 1, A_], [0], [0, 1], [A_]], cs.leaves)
    assert e.value.code == R.E_INVALID and "programme 2" in str(e.value) and "position 2" in str(e.value)
    with pytest.raises(gpu.ColttError) as e:
        gh.FilterEvalBatch([[0], [0] * 9 + [A_] * 8], cs.leaves)
    assert e.value.code == R.E_UNSUPPORTED and "programme 1" in str(e.value)


def _raw_ids(gpu, f, cap, room):
    o = np.full(room, 0xABCDABCDABCDABCD, np.uint64); n = C.c_uint64(0)
    rc = gpu.lib().coltt_hnsw_filter_ids(f.h, o.ctypes.data_as(C.c_void_p), C.c_uint64(cap), C.byref(n))
    return rc, o, n.value


def test_lifecycle(gpu):
    n = 2000
    X = O.fill_normal(61, (n, D)); lv = O.levels(62, n)
    gh = gpu.Hnsw(D, O.L2); _insert(gh, X, lv, 0, n)
    other = gpu.Hnsw(D, O.L2); _insert(other, X, lv, 0, 500)
    Q = X[:8] + 0.01
    ma = np.arange(n) % 3 == 0; mb = np.arange(n) % 2 == 0
    fa, fb = gh.Filter(np.nonzero(ma)[0]), gh.Filter(np.nonzero(mb)[0])
    # a repeated leaf handle; cap 0 and cap below allowed write no more than cap
    f = gh.FilterEval([0, 1, A_, 2, O_], [fa, fb, fa])
    want = np.nonzero(ma)[0].astype(np.uint64)
    assert f.allowed == len(want) and np.array_equal(f.ids(), want)
    rc, o, cnt = _raw_ids(gpu, f, 0, 8)
    assert rc == 0 and cnt == len(want) and (o == 0xABCDABCDABCDABCD).all()
    rc, o, cnt = _raw_ids(gpu, f, 300, 308)
    assert rc == 0 and cnt == len(want) and np.array_equal(o[:300], want[:300]) and (o[300:] == 0xABCDABCDABCDABCD).all()
    rc, o, cnt = _raw_ids(gpu, f, len(want) + 50, len(want) + 58)
    assert rc == 0 and cnt == len(want) and np.array_equal(o[:len(want)], want) and (o[len(want):] == 0xABCDABCDABCDABCD).all()
    assert len(f.ids(cap=5)) == 5
    # a leaf of another index
    fo = other.Filter([1, 2, 3])
    with pytest.raises(gpu.ColttError) as e:
        gh.FilterEval([0, 1, A_], [fa, fo])
    assert e.value.code == R.E_INVALID and "leaf 1" in str(e.value)
    # a destroyed leaf: unknown handle
    dead = gh.Filter([1, 2, 3]); hv = dead.h.value; dead.close(); dead.h = C.c_uint64(hv)
    with pytest.raises(gpu.ColttError) as e:
        gh.FilterEval([0, 1, A_], [fa, dead])
    assert e.value.code == R.E_NOT_FOUND
    dead.h = None
    # bad programmes are refused before any launch, with the checker's codes
    for prog, code in (([], R.E_INVALID), ([0, A_], R.E_INVALID), ([0, 1], R.E_INVALID), ([2], R.E_INVALID), ([0, -9], R.E_INVALID),
                       ([0] * 9 + [A_] * 8, R.E_UNSUPPORTED), ([0] + [N_] * 4096, R.E_UNSUPPORTED)):
        with pytest.raises(gpu.ColttError) as e:
            gh.FilterEval(prog, [fa, fb])
        assert e.value.code == code, prog
    with gh.FilterEval([0] + [N_] * 4095, [fa]) as f4096:       # the longest programme: an odd number of NOTs
        assert np.array_equal(f4096.ids(), np.nonzero(~ma)[0].astype(np.uint64))
    # a result outlives its leaves
    res = gh.FilterEval([0, 1, X_], [fa, fb])
    fa.close(); fb.close()
    want = np.nonzero(ma & ~mb)[0]
    with gh.Filter(want) as twin:
        assert np.array_equal(res.ids(), want.astype(np.uint64))
        _same_search(gpu, gh, Q, res, twin, ((gpu.FILTER_WALK, 64), (gpu.FILTER_EXACT, 0), (gpu.FILTER_AUTO, 0)), "outlives")
    # a result is a leaf like any other
    with gh.FilterEval([0, N_], [res]) as inv:
        assert np.array_equal(inv.ids(), np.nonzero(~(ma & ~mb))[0].astype(np.uint64))
    # an empty index: the result allows nothing
    e_idx = gpu.Hnsw(D, O.L2)
    with e_idx.FilterEval([T_], []) as f0:
        assert f0.allowed == 0 and len(f0.ids()) == 0 and f0.info()["slots"] == 0
        _, _, gc = e_idx.SearchFiltered(Q, K, f0)
        assert (gc == 0).all()
    # Load renumbers the index: leaves and results built before it are stale
    gh.Load(other.Commit())
    with pytest.raises(gpu.ColttError) as e:
        gh.FilterEval([0, N_], [res])
    assert e.value.code == R.E_INVALID and "stale" in str(e.value)
    with pytest.raises(gpu.ColttError) as e:
        res.ids()
    assert e.value.code == R.E_INVALID
    with gh.Filter([1, 2, 3]) as fresh, gh.FilterEval([0, N_], [fresh]) as f2:
        assert f2.allowed == 500 - 3
    res.close(); f.close(); fo.close()


def test_beside_a_writer(gpu):
    n = 3000
    X = O.fill_normal(81, (n, D)); lv = O.levels(82, n)
    gh = gpu.Hnsw(D, O.L2); _insert(gh, X, lv, 0, n)
    ma = np.arange(n) % 3 == 0; mb = np.arange(n) % 5 < 2
    fa, fb = gh.Filter(np.nonzero(ma)[0]), gh.Filter(np.nonzero(mb)[0])
    w_and = np.nonzero(ma & mb)[0].astype(np.uint64); w_or = np.nonzero(ma | mb)[0].astype(np.uint64)
    errors = []

    def evaluator():
        try:
            for it in range(50):
                for prog, want in (([0, 1, A_], w_and), ([0, 1, O_], w_or)):
                    with gh.FilterEval(prog, [fa, fb]) as f:
                        if f.allowed != len(want) or not np.array_equal(f.ids(), want):
                            errors.append((it, prog, f.allowed))
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    def inserter():
        try:
            Y = O.fill_normal(84, (300, D))
            for j in range(300):
                gh.Insert(n + j, Y[j], 0)
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=evaluator), threading.Thread(target=inserter)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:5]
    assert gh.Len() == n + 300
    with gh.FilterEval([0, N_], [fa]) as f:       # NOT sees the writer's vertices
        assert f.allowed == n + 300 - int(ma.sum())
    fa.close(); fb.close()
