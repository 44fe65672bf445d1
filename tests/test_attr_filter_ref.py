"""Attribute predicates without a device: the numpy definition (tests/attr_filter_ref.py) against a plain Python loop, and coltt_attr_cmp_host —
the comparison the kernel compiles — against numpy for every op and both types at the edge values."""
import itertools

import numpy as np
import pytest

import coltt_amd
import attr_filter_ref as A
import filter_expr_ref as R

I64_MIN, I64_MAX = -2**63, 2**63 - 1
I64_EDGE = [I64_MIN, I64_MIN + 1, -1, 0, 1, 2**53, 2**53 + 1, I64_MAX - 1, I64_MAX]
DENORM = float(np.nextafter(0.0, 1.0))
F64_EDGE = [-np.inf, -1.5, -DENORM, -0.0, 0.0, DENORM, 1.5, float(2**53), float(2**53 + 2), np.inf]


def test_numpy_definition_equals_the_python_loop():
    rng = np.random.default_rng(5)
    for n in (1, 7, 40):
        live = rng.random(n) < 0.8
        leaves = [rng.random(max(1, n // 2)) < 0.5, rng.random(n) < 0.3]
        ci = (rng.integers(-3, 4, n).astype(np.int64), rng.random(n) < 0.7, max(0, n - 2))
        cf = (rng.integers(-3, 4, n).astype(np.float64) / 2, rng.random(n) < 0.7, n)
        cols = [ci, cf]
        preds = [(c, op, operand) for c in (0, 1) for op in A.OPS for operand in (-1, 0, 2)]
        for i in range(len(preds)):
            prog = [2 + i]
            assert np.array_equal(A.evaluate(prog, leaves, cols, preds, live), A.evaluate_loop(prog, leaves, cols, preds, live)), (n, preds[i])
        for prog in ([2, 3, R.AND], [0, 2 + 7, R.ANDNOT], [2 + 4, R.NOT], [2 + 3, 2 + 6, R.ANDNOT], [1, 2 + 30, R.OR, R.ALL, R.AND, 2 + 12, R.ANDNOT]):
            assert R.validate(prog, 2 + len(preds))[0] == R.OK
            assert np.array_equal(A.evaluate(prog, leaves, cols, preds, live), A.evaluate_loop(prog, leaves, cols, preds, live)), (n, prog)


def test_unset_and_uncovered_slots_satisfy_nothing_and_not_sees_them():
    live = np.ones(6, bool); live[5] = False
    col = (np.arange(6, dtype=np.int64), np.array([1, 1, 0, 1, 1, 1], bool), 4)   # slot 2 never set, slots 4 and 5 past the coverage
    for op in A.OPS:
        m = A.evaluate([0], [], [col], [(0, op, 100 if op in (A.LT, A.LE, A.NE) else -1)], live)
        assert not m[2] and not m[4] and not m[5], op
    assert np.array_equal(np.nonzero(A.evaluate([0], [], [col], [(0, A.SET, 0)], live))[0], [0, 1, 3])
    assert np.array_equal(np.nonzero(A.evaluate([0, R.NOT], [], [col], [(0, A.SET, 0)], live))[0], [2, 4])


@pytest.mark.parametrize("op", A.OPS)
def test_cmp_host_i64_equals_numpy(op):
    for operand, value in itertools.product(I64_EDGE, I64_EDGE):
        want = bool(A.compare(op, np.array([value], np.int64), operand)[0])
        assert coltt_amd.attr_cmp_host(A.I64, op, operand, value) == want, (op, operand, value)
        assert coltt_amd.attr_cmp_host(A.I64, op, operand, value, is_set=False) is False


def test_cmp_host_i64_never_goes_through_a_double():
    a, b = 2**53, 2**53 + 1
    assert float(a) == float(b)                                   # the trap: equal as doubles
    assert coltt_amd.attr_cmp_host(A.I64, A.EQ, b, a) is False and coltt_amd.attr_cmp_host(A.I64, A.EQ, a, b) is False
    assert coltt_amd.attr_cmp_host(A.I64, A.LT, b, a) is True and coltt_amd.attr_cmp_host(A.I64, A.LT, a, b) is False
    assert coltt_amd.attr_cmp_host(A.I64, A.LT, I64_MAX, I64_MIN) is True and coltt_amd.attr_cmp_host(A.I64, A.GT, I64_MIN, I64_MAX) is True


@pytest.mark.parametrize("op", A.OPS)
def test_cmp_host_f64_equals_numpy(op):
    for operand, value in itertools.product(F64_EDGE, F64_EDGE):
        want = bool(A.compare(op, np.array([value], np.float64), operand)[0])
        assert coltt_amd.attr_cmp_host(A.F64, op, operand, value) == want, (op, operand, value)
        assert coltt_amd.attr_cmp_host(A.F64, op, operand, value, is_set=False) is False
    assert coltt_amd.attr_cmp_host(A.F64, A.EQ, 0.0, -0.0) is True and coltt_amd.attr_cmp_host(A.F64, A.LT, 0.0, -0.0) is False
    assert coltt_amd.attr_cmp_host(A.F64, A.GT, 0.0, DENORM) is True and coltt_amd.attr_cmp_host(A.F64, A.LT, np.inf, 1e308) is True


def test_cmp_host_refuses_nan_and_unknown_op_or_type():
    for op in (A.EQ, A.NE, A.GT, A.GE, A.LT, A.LE):
        with pytest.raises(coltt_amd.ColttError) as e:
            coltt_amd.attr_cmp_host(A.F64, op, float("nan"), 1.0)
        assert e.value.code == R.E_INVALID and "NaN" in str(e.value)
    assert coltt_amd.attr_cmp_host(A.F64, A.SET, float("nan"), 1.0) is True     # the operand of SET is ignored
    for type_, op in ((2, A.EQ), (-1, A.EQ), (A.I64, 7), (A.I64, -1), (A.F64, 7)):
        with pytest.raises(coltt_amd.ColttError) as e:
            coltt_amd.attr_cmp_host(type_, op, 0, 0)
        assert e.value.code == R.E_INVALID, (type_, op)
