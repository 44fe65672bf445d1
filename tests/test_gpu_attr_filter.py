"""Attribute columns and comparison predicates on the GPU (coltt_hnsw_attr_* / coltt_hnsw_filter_eval_attr / _eval_attr_batch; include/coltt_gpu.h,
"Attribute columns and predicates") against the definition in numpy (tests/attr_filter_ref.py): the result of a programme over resident leaves
and predicates is indistinguishable from coltt_hnsw_filter_create over the set the definition computes — allowed count, id list, info and every
filtered search (ids, score bits, counts, stats).  Every comparison is exact.

Slot counts.  A bitmap word is 32 slots and one ballot of the evaluate kernel is 64 (attr_filter.hpp): 1, 31, 32, 33, 63, 64, 65.  A wave's pass
is 64 words = 2 048 slots: 2 049.  A workgroup's tile is 1 024 words = 32 768 slots: 32 769.  70 001 = three workgroups and a ragged last word.
Values.  Half of the set slots hold 500, a twentieth 77, the rest lie in [501, 1000); the F64 column holds half of each.  The operands below then
allow about 0, 5, 50 and 100 % of the set slots per op.  EQ and NE are complements over one column, so EQ gets 0, 5 and 50 % there and NE 50, 95 and
100 %; EQ at 100 % and NE at 0 % need a constant column: the 64-slot case holds 7 everywhere.
The edge values of tests/test_attr_filter_ref.py sit at the first slots of every case of 31 slots and more."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import oracle as O
from util import bits

import attr_filter_ref as A
import filter_expr_ref as R

pytestmark = pytest.mark.gpu

K, D = 10, 64
I64_MIN, I64_MAX = -2**63, 2**63 - 1
DENORM = float(np.nextafter(0.0, 1.0))
I64_EDGE = [I64_MIN, I64_MAX, 2**53, 2**53 + 1]
F64_EDGE = [-0.0, 0.0, -np.inf, np.inf, DENORM, -DENORM]
# (op, operand in the I64 column's scale; the F64 column holds value / 2 and is asked at operand / 2)
OPERANDS = [(A.EQ, -5), (A.EQ, 77), (A.EQ, 500), (A.EQ, 7), (A.NE, 7), (A.NE, 500), (A.NE, 77), (A.NE, -5),
            (A.LT, 0), (A.LT, 78), (A.LT, 501), (A.LT, 1000), (A.LE, -1), (A.LE, 77), (A.LE, 500), (A.LE, 999),
            (A.GT, 999), (A.GT, 950), (A.GT, 500), (A.GT, -1), (A.GE, 1000), (A.GE, 951), (A.GE, 501), (A.GE, 0), (A.SET, 0)]
EDGE_I64 = [(A.EQ, 2**53), (A.EQ, 2**53 + 1), (A.LT, 2**53 + 1), (A.GT, 2**53), (A.GE, I64_MAX), (A.LE, I64_MIN), (A.LT, I64_MIN), (A.GT, I64_MAX),
            (A.NE, I64_MIN)]
EDGE_F64 = [(A.EQ, 0.0), (A.EQ, -0.0), (A.LT, 0.0), (A.GT, 0.0), (A.LT, DENORM), (A.GE, DENORM), (A.LT, np.inf), (A.GE, np.inf), (A.LE, -np.inf),
            (A.GT, -np.inf), (A.NE, np.inf)]


def _insert(gh, X, lv, lo, hi, ids=None, batch=512):
    import torch
    if hi <= lo:
        return
    d = X.shape[1]
    xd = torch.from_numpy(np.ascontiguousarray(X[lo:hi])).cuda(); torch.cuda.synchronize()
    i = lo
    while i < hi:
        b = int(min(hi - i, max(1, min(batch, i // 16))))
        gh.InsertBatchDevice(xd.data_ptr() + (i - lo) * d * 4, b, lv[i:i + b], batch=b, first_id=i, ids=None if ids is None else ids[i:i + b])
        i += b


def _draw(rng, n, const):
    if const:
        return np.full(n, 7, np.int64)
    u = rng.random(n)
    return np.where(u < 0.5, 500, np.where(u < 0.55, 77, rng.integers(501, 1000, n))).astype(np.int64)


class Case:
    """An index grown in three stages with one I64 and one F64 column set in two: after n1 slots (coverage n1), then — the index has grown to
    n2 slots — again (coverage n2, some slots overwritten, some never set); a tail of vertices follows the last set; then removals."""

    def __init__(self, gpu, n, d=D, metric=None, quant=None, ids=False, const=False, seed=1500):
        metric = O.L2 if metric is None else metric
        quant = O.Q_NONE if quant is None else quant
        self.n, self.d = n, d
        self.X = O.fill_normal(seed + n, (n, d)); lv = O.levels(seed + n + 1, n)
        self.ids = (np.arange(n, dtype=np.uint64) * 7 + 1000) if ids else None
        self.gh = gh = gpu.Hnsw(d, metric, quantization=quant)
        rng = np.random.default_rng(seed + n)
        tail = 0 if n < 31 else 3
        n1 = max(1, n // 2); n2 = max(n1, n - tail)
        self.n1, self.n2 = n1, n2
        self.vi = np.zeros(n, np.int64); self.vf = np.zeros(n, np.float64); self.set = np.zeros(n, bool)
        _insert(gh, self.X, lv, 0, n1, self.ids)
        self.ci, self.cf = gh.AttrColumn(gpu.ATTR_I64), gh.AttrColumn(gpu.ATTR_F64)
        assert self.ci.info() == {"index": gh.h.value, "type": gpu.ATTR_I64, "slots": 0, "set": 0}
        # stage 1: about 70 % of the first n1 slots; the edge values at the first slots
        s1 = np.nonzero(rng.random(n1) < 0.7)[0] if n1 > 1 else np.array([0])
        v1 = _draw(rng, len(s1), const)
        self._apply(s1, v1, v1 / 2.0)
        if n >= 31:
            self._apply(np.arange(len(I64_EDGE)), np.array(I64_EDGE, np.int64), None)
            self._apply(np.arange(len(F64_EDGE)), None, np.array(F64_EDGE, np.float64))
        self.covered = n1
        assert self.ci.info()["slots"] == n1 and self.ci.info()["set"] == int(self.set[:n1].sum()) and self.cf.info()["slots"] == n1
        _insert(gh, self.X, lv, n1, n2, self.ids)
        self.stage1 = (self.vi.copy(), self.vf.copy(), self.set.copy(), n1)   # what an evaluation between the stages sees: coverage below n_slots
        self.mid = None
        if n2 > n1:
            with gh.FilterEvalAttr([0, R.NOT], [], [(self.ci, gpu.CMP_SET, 0)]) as f:
                self.mid = f.ids()
        # stage 2: about 70 % of the slots past a few kept edge slots, over the grown index: overwrites and new slots
        s2 = np.nonzero(rng.random(n2) < 0.7)[0]
        s2 = s2[s2 >= 8] if n >= 31 else s2
        v2 = _draw(rng, len(s2), const)
        self._apply(s2, v2, v2 / 2.0)
        self.covered = n2
        self.leaf_mask = rng.random(n2) < 0.3
        self.leaf = gh.Filter(self.to_ids(np.nonzero(self.leaf_mask)[0]))
        _insert(gh, self.X, lv, n2, n, self.ids)
        self.live = np.ones(n, bool)
        if n >= 31:   # removals after the set: set and unset slots, a tail vertex
            rm = list(np.nonzero(self.set)[0][5:8]) + list(np.nonzero(~self.set[:n2])[0][:2]) + [n - 1]
            for s in rm:
                gh.Remove(int(self.to_ids(np.array([s]))[0]))
                self.live[s] = False
        assert gh.Len() == int(self.live.sum())
        self.Q = O.fill_normal(seed + 7, (8, d))

    def _apply(self, slots, vi, vf):
        ids = self.to_ids(slots)
        if vi is not None:
            assert self.ci.set(ids, vi) == len(slots)
            self.vi[slots] = vi
        if vf is not None:
            assert self.cf.set(ids, vf) == len(slots)
            self.vf[slots] = vf
        if vi is not None and vf is not None:
            self.set[slots] = True
        else:   # an edge value in one column: the other column holds the slot's value of stage 1 or, if it had none, 0
            for s in slots:
                if not self.set[s]:
                    self.set[s] = True
                    (self.cf if vi is not None else self.ci).set(self.to_ids(np.array([s])), [0])

    def to_ids(self, slots):
        slots = np.asarray(slots, np.int64)
        return slots.astype(np.uint64) if self.ids is None else self.ids[slots]

    def columns(self):
        return [(self.vi, self.set, self.covered), (self.vf, self.set, self.covered)]

    def want(self, prog, preds, leaves=None):
        """preds: (0 = I64 / 1 = F64, op, operand)"""
        return np.nonzero(A.evaluate(prog, [self.leaf_mask] if leaves is None else leaves, self.columns(), preds, self.live))[0]

    def gpu_preds(self, preds):
        return [((self.ci, self.cf)[c], op, operand) for c, op, operand in preds]


_CACHE = {}
KINDS = {"n1": dict(n=1), "n31": dict(n=31), "n32": dict(n=32), "n33": dict(n=33), "n63": dict(n=63), "n64": dict(n=64, const=True), "n65": dict(n=65),
         "n1000": dict(n=1000), "n2049": dict(n=2049), "n32769": dict(n=32769), "n70001": dict(n=70001), "ids1000": dict(n=1000, ids=True, seed=1900),
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


def _same_filter(cs, f, want, what):
    """f is indistinguishable from coltt_hnsw_filter_create over the ids of `want` (slots ascending)"""
    with cs.gh.Filter(cs.to_ids(want)) as twin:
        assert f.allowed == twin.allowed == len(want), (what, f.allowed, twin.allowed, len(want))
        assert f.info() == twin.info() == {"index": cs.gh.h.value, "allowed": len(want), "slots": cs.n}, what
        got = f.ids()
        assert np.array_equal(got, cs.to_ids(want)) and np.array_equal(twin.ids(), got), what


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "f16_768d_1800"])
def test_every_op_and_type_equals_filter_create_over_the_defined_set(gpu, kind):
    cs = _case(gpu, kind)
    gh = cs.gh
    if cs.mid is not None:   # between the stages: the coverage (n1) was below the index's slots (n2)
        vi, vf, st, cov = cs.stage1
        live_mid = np.ones(cs.n2, bool)
        want = np.nonzero(A.evaluate([0, R.NOT], [], [(vi[:cs.n2], st[:cs.n2], cov)], [(0, A.SET, 0)], live_mid))[0]
        assert np.array_equal(cs.mid, cs.to_ids(want)) and (want >= cov).sum() == cs.n2 - cov, kind
    assert cs.ci.info() == {"index": gh.h.value, "type": gpu.ATTR_I64, "slots": cs.n2, "set": int(cs.set.sum())}
    assert cs.cf.info() == {"index": gh.h.value, "type": gpu.ATTR_F64, "slots": cs.n2, "set": int(cs.set.sum())}
    n_set_live = int((cs.set & cs.live).sum())
    fractions = {}
    for c, table in ((0, OPERANDS + EDGE_I64), (1, [(op, o / 2.0) for op, o in OPERANDS] + EDGE_F64)):
        for i, (op, operand) in enumerate(table):
            preds = [(c, op, operand)]
            want = cs.want([1], preds)
            with gh.FilterEvalAttr([1], [cs.leaf], cs.gpu_preds(preds)) as f:
                _same_filter(cs, f, want, (kind, c, op, operand))
            if i < len(OPERANDS):
                fractions.setdefault((c, op), []).append(len(want) / max(1, n_set_live))
    if kind in ("n1000", "n70001"):       # the operands do allow about 0, 5, 50 and 100 % of the set slots (the few edge slots aside)
        bins = {0: (0.0, 0.01), 5: (0.02, 0.09), 50: (0.4, 0.6), 95: (0.9, 0.97), 100: (0.99, 1.0)}
        for (c, op), fr in fractions.items():
            for b in {A.EQ: (0, 5, 50), A.NE: (50, 95, 100), A.SET: (100,)}.get(op, (0, 5, 50, 100)):
                assert any(bins[b][0] <= x <= bins[b][1] for x in fr), (kind, c, op, b, fr)
    if kind == "n64":                     # the constant columns: EQ at about 100 %, NE at about 0 % (the edge slots and their fill-ins aside)
        assert len(cs.want([1], [(0, A.EQ, 7)])) >= n_set_live - 6 and len(cs.want([1], [(0, A.NE, 7)])) <= 6
        assert len(cs.want([1], [(1, A.EQ, 3.5)])) >= n_set_live - 6 and len(cs.want([1], [(1, A.NE, 3.5)])) <= 6


def _mixed(cs):
    """leaf 0; predicates 1 .. 4 = p0 (I64 < 501), p1 (F64 >= 250.5), SET of the I64 column, I64 == 77"""
    preds = [(0, A.LT, 501), (1, A.GE, 250.5), (0, A.SET, 0), (0, A.EQ, 77)]
    progs = [("p0 p1 AND", [1, 2, R.AND]), ("leaf p0 ANDNOT", [0, 1, R.ANDNOT]), ("p0 NOT", [1, R.NOT]), ("p0 SET ANDNOT", [1, 3, R.ANDNOT]),
             ("SET p0 ANDNOT", [3, 1, R.ANDNOT]), ("leaf p1 OR p3 ANDNOT", [0, 2, R.OR, 4, R.ANDNOT]), ("SET NOT", [3, R.NOT]),
             ("depth 8", [0, 1, 2, R.ALL, 3, 1, 4, 0, R.AND, R.OR, R.ANDNOT, R.OR, R.AND, R.OR, R.ANDNOT])]
    return preds, progs


@pytest.mark.parametrize("kind", ["n33", "n1000", "ids1000", "n2049", "n70001", "f16_768d_1800"])
def test_mixed_programmes_of_leaves_and_predicates(gpu, kind):
    cs = _case(gpu, kind)
    gh = cs.gh
    preds, progs = _mixed(cs)
    searches = kind in ("n1000", "f16_768d_1800")
    modes = ((gpu.FILTER_WALK, 64), (gpu.FILTER_EXACT, 0), (gpu.FILTER_AUTO, 0))
    for name, prog in progs:
        assert R.validate(prog, 1 + len(preds))[0] == R.OK
        if name == "depth 8":
            assert R.validate(prog, 1 + len(preds))[1] == 8
        want = cs.want(prog, preds)
        if name == "p0 SET ANDNOT":
            assert len(want) == 0
        if name == "SET NOT":      # NOT sees the unset slots and the vertices inserted after the last set; the bare predicate does not
            assert (want >= cs.n2).sum() == int(cs.live[cs.n2:].sum()) and len(cs.want([3], preds)) == int((cs.set & cs.live).sum())
        with gh.FilterEvalAttr(prog, [cs.leaf], cs.gpu_preds(preds)) as f:
            _same_filter(cs, f, want, (kind, name))
            if searches:
                with gh.Filter(cs.to_ids(want)) as twin:
                    _same_search(gpu, gh, cs.Q, f, twin, modes, (kind, name))


def test_batch_of_48_programmes_over_a_shared_predicate_table(gpu):
    cs = _case(gpu, "n70001")
    gh = cs.gh
    rng = np.random.default_rng(77)
    preds = [(int(rng.integers(0, 2)), int(op), int(rng.integers(400, 1000))) for op in rng.integers(0, 7, 14)]
    preds = [(c, op, o / 2.0 if c else o) for c, op, o in preds] + [(0, A.EQ, 77), (0, A.EQ, 77)]     # a repeated predicate
    gp = cs.gpu_preds(preds)
    nl = 1 + len(preds)
    import coltt_amd
    progs = []
    while len(progs) < 48:
        prog = coltt_amd.filter_postfix(R.random_tree(rng, nl, int(rng.integers(1, 5))))
        if R.validate(prog, nl)[0] == R.OK:
            progs.append(prog)
    progs[3] = [1, 1, R.ANDNOT]; progs[4] = [R.ALL]; progs[5] = [nl - 1]
    outs = gh.FilterEvalAttrBatch(progs, [cs.leaf], gp)
    assert len(outs) == 48 and len(set(f.h.value for f in outs)) == 48
    for i, (prog, f) in enumerate(zip(progs, outs)):
        want = cs.to_ids(cs.want(prog, preds))
        with gh.FilterEvalAttr(prog, [cs.leaf], gp) as s:
            assert f.allowed == s.allowed == len(want) and f.info() == s.info(), (i, prog)
            assert np.array_equal(f.ids(), want) and np.array_equal(s.ids(), want), (i, prog)
    for f in outs:
        f.close()
    # n_preds == 0: the call equals coltt_hnsw_filter_eval_batch
    plain = [[0], [0, R.NOT], [R.ALL, 0, R.ANDNOT], [0, 0, R.AND]]
    a = gh.FilterEvalAttrBatch(plain, [cs.leaf], []); b = gh.FilterEvalBatch(plain, [cs.leaf])
    for fa, fb in zip(a, b):
        assert fa.allowed == fb.allowed and fa.info() == fb.info() and np.array_equal(fa.ids(), fb.ids())
        fa.close(); fb.close()
    with gh.FilterEvalAttr([0, R.NOT], [cs.leaf], []) as fa, gh.FilterEval([0, R.NOT], [cs.leaf]) as fb:
        assert fa.allowed == fb.allowed and np.array_equal(fa.ids(), fb.ids())
    assert gh.FilterEvalAttrBatch([], [cs.leaf], gp) == []


def _small(gpu, n=300, ids=False):
    X = O.fill_normal(2100 + n, (n, D)); lv = O.levels(2101 + n, n)
    idv = (np.arange(n, dtype=np.uint64) * 3 + 50) if ids else None
    gh = gpu.Hnsw(D, O.L2)
    _insert(gh, X, lv, 0, n, idv)
    return gh, X, lv, (np.arange(n, dtype=np.uint64) if idv is None else idv)


@pytest.mark.parametrize("ids", [False, True])
def test_get_returns_what_was_set_and_set_ignores_unknown_and_removed_ids(gpu, ids):
    n = 300
    gh, X, lv, idv = _small(gpu, n, ids)
    gh.Remove(int(idv[10])); gh.Remove(int(idv[11]))
    ci, cf = gh.AttrColumn(gpu.ATTR_I64), gh.AttrColumn(gpu.ATTR_F64)
    v, s = ci.get(idv[:5])
    assert not s.any() and (v == 0).all()                                  # nothing was ever set
    # duplicates: the last value wins; ids 10 and 11 are removed, 10**9 is unknown
    call_ids = np.array([idv[3], idv[10], idv[4], idv[3], 10**9, idv[5], idv[3], idv[11], idv[4]], np.uint64)
    vals = np.array([1, 2, 3, 4, 5, 6, I64_MIN, 8, I64_MAX], np.int64)
    assert ci.set(call_ids, vals) == 3
    assert ci.info() == {"index": gh.h.value, "type": gpu.ATTR_I64, "slots": n, "set": 3}
    v, s = ci.get(np.array([idv[3], idv[4], idv[5], idv[6], idv[10], 10**9], np.uint64))
    assert list(s) == [True, True, True, False, False, False] and list(v) == [I64_MIN, I64_MAX, 6, 0, 0, 0]
    assert ci.set(np.array([idv[5]], np.uint64), [7]) == 1 and ci.info()["set"] == 3     # an overwrite sets no new slot
    assert list(ci.get([idv[5]])[0]) == [7]
    fv = np.array([-0.0, np.inf, DENORM, -1.5], np.float64)
    assert cf.set(idv[20:24], fv) == 4
    v, s = cf.get(idv[19:25])
    assert list(s) == [False, True, True, True, True, False] and np.array_equal(v[1:5].view(np.uint64), fv.view(np.uint64))
    # a NaN refuses the whole call before anything is written
    with pytest.raises(gpu.ColttError) as e:
        cf.set(idv[30:33], [1.0, float("nan"), 2.0])
    assert e.value.code == R.E_INVALID and "NaN" in str(e.value)
    assert not cf.get(idv[30:33])[1].any() and cf.info()["set"] == 4
    # a vertex removed after it was set keeps nothing a comparison can see, and get no longer finds it
    gh.Remove(int(idv[4]))
    with gh.FilterEvalAttr([0], [], [(ci, gpu.CMP_SET, 0)]) as f:
        assert np.array_equal(f.ids(), np.array([idv[3], idv[5]], np.uint64))
    assert list(ci.get([idv[4]])[1]) == [False]
    # Update in place = Remove + Insert under the same id: the new slot is unset until it is set again
    if ids:
        gh.Remove(int(idv[3])); gh.Insert(int(idv[3]), X[3], 0)
        assert list(ci.get([idv[3]])[1]) == [False]
        assert ci.set([idv[3]], [99]) == 1 and list(ci.get([idv[3]])[0]) == [99] and ci.info()["slots"] == n + 1
    ci.close(); cf.close()


def _raw_eval(gpu, gh, prog, leaves, pa, n_preds):
    p = np.asarray(prog, np.int32); lh = np.array([f.h.value for f in leaves], np.uint64)
    out = C.c_uint64(0xABCD); al = C.c_uint64(0xABCD)
    rc = gpu.lib().coltt_hnsw_filter_eval_attr(gh.h, p.ctypes.data_as(C.c_void_p), C.c_size_t(p.size), lh.ctypes.data_as(C.c_void_p) if lh.size else None,
                                               C.c_size_t(lh.size), pa, C.c_size_t(n_preds), C.byref(al), C.byref(out))
    return rc, out.value, gpu.lib().coltt_last_error().decode()


def test_errors_create_nothing(gpu):
    gh, X, lv, idv = _small(gpu, 200)
    other, _, _, _ = _small(gpu, 100)
    ci, cf, co = gh.AttrColumn(gpu.ATTR_I64), gh.AttrColumn(gpu.ATTR_F64), other.AttrColumn(gpu.ATTR_I64)
    ci.set(idv, np.arange(200)); cf.set(idv, np.arange(200) / 2.0); co.set(idv[:100], np.arange(100))
    leaf = gh.Filter(idv[::2])
    dead = gh.AttrColumn(gpu.ATTR_I64); dead_h = dead.h.value; dead.close()
    gone = gh.Filter([1]); gone_h = gone.h.value; gone.close()

    def pred(col_h, op, reserved=0, i64=None, f64=None):
        p = gpu.AttrPred(); p.column = col_h; p.op = op; p.reserved = reserved
        if f64 is not None:
            p.value.f64 = f64
        else:
            p.value.i64 = 0 if i64 is None else i64
        return p

    ok = pred(ci.h.value, gpu.CMP_LT, i64=50)
    cases = [("unknown column", [ok, pred(dead_h, gpu.CMP_LT)], R.E_NOT_FOUND, "predicate 1"),
             ("another index", [pred(co.h.value, gpu.CMP_LT)], R.E_INVALID, "predicate 0"),
             ("unknown op", [ok, ok, pred(ci.h.value, 7)], R.E_INVALID, "predicate 2"),
             ("negative op", [pred(ci.h.value, -1)], R.E_INVALID, "predicate 0"),
             ("reserved", [ok, pred(ci.h.value, gpu.CMP_EQ, reserved=1)], R.E_INVALID, "predicate 1"),
             ("NaN operand", [ok, pred(cf.h.value, gpu.CMP_GE, f64=float("nan"))], R.E_INVALID, "predicate 1")]
    before = gh.Filter([]); h0 = before.h.value; before.close()
    for name, plist, code, where in cases:
        pa = (gpu.AttrPred * len(plist))(*plist)
        rc, out, msg = _raw_eval(gpu, gh, [1 + len(plist) - 1], [leaf], pa, len(plist))
        assert rc == code and where in msg and out == 0xABCD, (name, rc, msg)
    rc, out, msg = _raw_eval(gpu, gh, [1], [leaf], None, 1)                                   # NULL preds with n_preds > 0
    assert rc == R.E_INVALID and out == 0xABCD, msg
    pa = (gpu.AttrPred * 1)(ok)
    for prog, code, where in (([2], R.E_INVALID, "position 0"), ([0, 1], R.E_INVALID, "position 2"), ([1, R.AND], R.E_INVALID, "position 1"),
                              ([], R.E_INVALID, ""), ([1] * 9 + [R.AND] * 8, R.E_UNSUPPORTED, "position 8")):
        rc, out, msg = _raw_eval(gpu, gh, prog, [leaf], pa, 1)
        assert rc == code and where in msg and out == 0xABCD, (prog, rc, msg)
    # an unknown leaf beside good predicates; a batch names the bad programme
    gone.h = C.c_uint64(gone_h)
    rc, out, msg = _raw_eval(gpu, gh, [1], [gone], pa, 1)
    gone.h = None
    assert rc == R.E_NOT_FOUND and out == 0xABCD, msg
    with pytest.raises(gpu.ColttError) as e:
        gh.FilterEvalAttrBatch([[0, 1, R.AND], [1], [0, 1]], [leaf], [(ci, gpu.CMP_LT, 50)])
    assert e.value.code == R.E_INVALID and "programme 2" in str(e.value) and "position 2" in str(e.value)
    # nothing was created by any of them: handles are handed out in sequence, and the next one follows the one before the failures
    after = gh.Filter([]); assert after.h.value == h0 + 1, (h0, after.h.value); after.close()
    # a NaN operand is ignored by SET; an unknown type is refused at create
    with gh.FilterEvalAttr([0], [], [(cf, gpu.CMP_SET, float("nan"))]) as f:
        assert f.allowed == 200
    with pytest.raises(gpu.ColttError) as e:
        gh.AttrColumn(2)
    assert e.value.code == R.E_INVALID
    # an empty index, a column never set, an empty result
    e_idx = gpu.Hnsw(D, O.L2)
    with e_idx.AttrColumn(gpu.ATTR_F64) as c0, e_idx.FilterEvalAttr([0, R.NOT], [], [(c0, gpu.CMP_LT, 1.0)]) as f0:
        assert f0.allowed == 0 and f0.info()["slots"] == 0 and c0.set([1, 2], [1.0, 2.0]) == 0
    with gh.AttrColumn(gpu.ATTR_I64) as c1, gh.FilterEvalAttr([0], [], [(c1, gpu.CMP_NE, 5)]) as f1, gh.FilterEvalAttr([0, R.NOT], [], [(c1, gpu.CMP_SET, 0)]) as f2:
        assert f1.allowed == 0 and len(f1.ids()) == 0 and f2.allowed == 200
    for o in (ci, cf, co, leaf):
        o.close()


def test_stale_after_a_renumbering_compact_and_bulk_load_valid_after_a_noop_compact(gpu):
    gh, X, lv, idv = _small(gpu, 400)
    ci = gh.AttrColumn(gpu.ATTR_I64)
    ci.set(idv, np.arange(400))
    st = gh.Compact()                                   # nothing was removed: no slot moves, the column stays valid
    assert st["slots_before"] == st["slots_after"] == 400
    with gh.FilterEvalAttr([0], [], [(ci, gpu.CMP_LT, 100)]) as f:
        assert f.allowed == 100
    assert ci.set(idv[:1], [5]) == 1 and list(ci.get(idv[:1])[0]) == [5]
    gh.Remove(7); gh.Remove(8)
    st = gh.Compact()
    assert st["slots_after"] == 398
    for call in (lambda: gh.FilterEvalAttr([0], [], [(ci, gpu.CMP_LT, 100)]), lambda: ci.set(idv[:1], [5]), lambda: ci.get(idv[:1])):
        with pytest.raises(gpu.ColttError) as e:
            call()
        assert e.value.code == R.E_INVALID and "stale" in str(e.value)
    assert ci.info()["slots"] == 400                    # info and destroy still serve a stale column
    live_ids = np.array([i for i in range(400) if i not in (7, 8)], np.uint64)
    with gh.AttrColumn(gpu.ATTR_I64) as c2:             # rebuilt by ids
        assert c2.set(np.arange(400, dtype=np.uint64), np.arange(400)) == 398
        with gh.FilterEvalAttr([0], [], [(c2, gpu.CMP_LT, 100)]) as f:
            assert np.array_equal(f.ids(), live_ids[live_ids < 100])
        # bulk_load renumbers as well
        oh = O.Hnsw(D, O.L2); Y = O.fill_normal(2300, (120, D)); oh.insert_many(np.arange(120, dtype=np.uint64), Y, O.levels(2301, 120))
        gh.BulkLoad(oh.export(with_vectors=False), Y)
        with pytest.raises(gpu.ColttError) as e:
            gh.FilterEvalAttr([0], [], [(c2, gpu.CMP_LT, 100)])
        assert e.value.code == R.E_INVALID and "stale" in str(e.value)
    with gh.AttrColumn(gpu.ATTR_F64) as c3:
        assert c3.set(np.arange(120, dtype=np.uint64), np.arange(120) / 4.0) == 120
        with gh.FilterEvalAttr([0], [], [(c3, gpu.CMP_GE, 10.0)]) as f:
            assert f.allowed == 80
    ci.close()


def test_one_thread_setting_beside_four_evaluating(gpu):
    n = 5000
    gh, X, lv, idv = _small(gpu, n)
    ci = gh.AttrColumn(gpu.ATTR_I64)
    state = [np.arange(n, dtype=np.int64) % 10, 9 - np.arange(n, dtype=np.int64) % 10]    # the writer flips every value between the two
    ci.set(idv, state[0])
    wants = [np.nonzero(s < 3)[0].astype(np.uint64) for s in state]
    assert not np.array_equal(wants[0], wants[1]) and len(np.intersect1d(wants[0], wants[1])) == 0
    errors, seen = [], [0, 0]
    done = threading.Event()

    def evaluator():
        try:
            for it in range(40):
                with gh.FilterEvalAttr([0], [], [(ci, gpu.CMP_LT, 3)]) as f:
                    got = f.ids()
                which = [i for i in (0, 1) if np.array_equal(got, wants[i])]
                if len(which) != 1 or f.allowed != len(got):
                    errors.append((it, f.allowed, len(got)))      # a mixture of the two states
                else:
                    seen[which[0]] += 1
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))

    def writer():
        try:
            for it in range(30):
                ci.set(idv, state[(it + 1) % 2])
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))
        done.set()

    ts = [threading.Thread(target=writer)] + [threading.Thread(target=evaluator) for _ in range(4)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors[:5]
    assert sum(seen) == 160 and done.is_set()
    with gh.FilterEvalAttr([0], [], [(ci, gpu.CMP_LT, 3)]) as f:      # the writer made 30 sets: the column ends in state 0
        assert np.array_equal(f.ids(), wants[0])
    ci.close()
