"""Filter expressions without a device: the numpy definition (tests/filter_expr_ref.py) against Python set algebra, the library's programme
checker (coltt_hnsw_filter_prog_check_host — the code coltt_hnsw_filter_eval itself calls) against the definition's validator on every
malformed shape and on the depth and length boundaries, the tuple -> postfix helper, and the entry points' errors that need no device."""
import ctypes as C

import numpy as np
import pytest

import coltt_amd
import filter_expr_ref as R

SYMS = ("coltt_hnsw_filter_eval", "coltt_hnsw_filter_eval_batch", "coltt_hnsw_filter_ids", "coltt_hnsw_filter_info",
        "coltt_hnsw_filter_prog_check_host")


def check(prog, n_leaves):
    L = coltt_amd.lib()
    p = np.ascontiguousarray(prog, np.int32)
    d = C.c_uint32(0xDEAD)
    rc = L.coltt_hnsw_filter_prog_check_host(p.ctypes.data_as(C.c_void_p), C.c_size_t(p.size), C.c_size_t(n_leaves), C.byref(d))
    return rc, d.value


def test_symbols_are_declared_and_exported():
    L = coltt_amd.lib()
    syms = coltt_amd.declared_symbols()
    for s in SYMS:
        assert s in syms and hasattr(L, s), s
    assert (coltt_amd.FOP_AND, coltt_amd.FOP_OR, coltt_amd.FOP_ANDNOT, coltt_amd.FOP_NOT, coltt_amd.FOP_ALL) == (R.AND, R.OR, R.ANDNOT, R.NOT, R.ALL)
    hdr = open(coltt_amd.__path__[0] + "/../include/coltt_gpu.h").read()
    for name, v in (("AND", R.AND), ("OR", R.OR), ("ANDNOT", R.ANDNOT), ("NOT", R.NOT), ("ALL", R.ALL)):
        assert f"#define COLTT_FOP_{name}" in hdr and f"({v})" in hdr.split(f"#define COLTT_FOP_{name}")[1].split("\n")[0]


def test_reference_evaluator_agrees_with_set_algebra_on_200_random_trees():
    rng = np.random.default_rng(2024)
    for it in range(200):
        n = int(rng.integers(1, 200))
        n_leaves = int(rng.integers(1, 6))
        live = rng.random(n) < 0.85
        leaves = []
        for _ in range(n_leaves):
            m = int(rng.integers(0, n + 1))          # built when the index had m slots
            leaves.append(rng.random(m) < rng.random())
        tree = R.random_tree(rng, n_leaves, int(rng.integers(0, 7)))
        prog = coltt_amd.filter_postfix(tree)
        got = R.evaluate(prog, leaves, live)
        live_set = set(np.nonzero(live)[0].tolist())
        want = R.tree_sets(tree, [set(np.nonzero(a)[0].tolist()) for a in leaves], live_set) & live_set
        assert set(np.nonzero(got)[0].tolist()) == want, (it, tree)
        assert len(got) == n


A, O_, N, X, T = R.AND, R.OR, R.NOT, R.ANDNOT, R.ALL
MALFORMED = [
    ("empty", [], 3),
    ("underflow: operator first", [A], 3),
    ("underflow: binary on one value", [0, A], 3),
    ("underflow: NOT on nothing", [N], 3),
    ("underflow: second operator", [0, 1, O_, X], 3),
    ("two values left", [0, 1], 3),
    ("three values left", [0, 1, 2, A], 3),
    ("ALL leaves two", [0, T], 3),
    ("leaf index == n_leaves", [0, 3, A], 3),
    ("leaf index far past", [2 ** 31 - 1], 3),
    ("no leaves at all", [0], 0),
    ("unknown operator -6", [0, 1, -6], 3),
    ("unknown operator INT_MIN", [0, -2 ** 31], 3),
]


@pytest.mark.parametrize("name,prog,n_leaves", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_checker_refuses_every_malformed_shape(name, prog, n_leaves):
    want, _ = R.validate(prog, n_leaves)
    assert want == R.E_INVALID
    rc, _ = check(prog, n_leaves)
    assert rc == want, (name, rc)
    assert b"position" in coltt_amd.lib().coltt_last_error()


def _nest(depth):
    """`depth` pushes, then depth - 1 ANDs: the stack reaches exactly `depth`"""
    return [0] * depth + [A] * (depth - 1)


def test_depth_boundary():
    assert R.validate(_nest(8), 1) == (R.OK, 8) and check(_nest(8), 1) == (R.OK, 8)
    assert R.validate(_nest(9), 1)[0] == R.E_UNSUPPORTED and check(_nest(9), 1)[0] == R.E_UNSUPPORTED
    assert check([T] * 9 + [O_] * 8, 0)[0] == R.E_UNSUPPORTED      # ALL counts as a push
    for d in range(1, 9):
        assert check(_nest(d), 1) == (R.OK, d) == R.validate(_nest(d), 1)


def test_length_boundary():
    chain = lambda n: [0] + [N] * (n - 1)    # noqa: E731  one value, n - 1 NOTs: n entries, depth 1
    assert len(chain(4096)) == 4096
    assert R.validate(chain(4096), 1) == (R.OK, 1) and check(chain(4096), 1) == (R.OK, 1)
    assert R.validate(chain(4097), 1)[0] == R.E_UNSUPPORTED and check(chain(4097), 1)[0] == R.E_UNSUPPORTED
    wide = [0, 1, A] + [2, O_] * 2046 + [N]  # 4096 entries, depth 2
    assert len(wide) == 4096 and check(wide, 3) == (R.OK, 2) == R.validate(wide, 3)


def test_checker_agrees_with_the_validator_on_random_programmes():
    rng = np.random.default_rng(7)
    seen = set()
    for _ in range(3000):
        n_leaves = int(rng.integers(0, 4))
        prog = rng.integers(-7, 4, int(rng.integers(0, 12))).tolist()
        want = R.validate(prog, n_leaves)
        rc, d = check(prog, n_leaves)
        assert rc == want[0], (prog, n_leaves, rc, want)
        if rc == R.OK:
            assert d == want[1], (prog, d, want)
        seen.add(rc)
    assert {R.OK, R.E_INVALID} <= seen
    for _ in range(300):                      # deep ones: pushes dominate
        prog = rng.choice([0, 0, 0, T, A, O_, N], int(rng.integers(8, 40))).tolist()
        assert check(prog, 1)[0] == R.validate(prog, 1)[0], prog


def test_tuple_to_postfix_round_trips():
    P, Tr = coltt_amd.filter_postfix, coltt_amd.filter_tree
    assert P(("and", 0, ("or", 1, 2))) == [0, 1, 2, O_, A]
    assert P(("or", ("and", 0, 1), 2)) == [0, 1, A, 2, O_]
    assert P(("andnot", ("or", 0, 1), 2)) == [0, 1, O_, 2, X]
    assert P(("not", 0)) == [0, N] and P(("andnot", "all", 0)) == [T, 0, X] and P("all") == [T] and P(3) == [3]
    assert P(("and", 0, 1, 2, 3)) == [0, 1, A, 2, A, 3, A]          # n-ary folds from the left: the stack stays at 2
    assert P(("AND", 0, ("Or", 1, 2))) == P(("and", 0, ("or", 1, 2)))
    rng = np.random.default_rng(11)
    for _ in range(200):
        tree = R.random_tree(rng, 5, int(rng.integers(0, 7)))
        prog = P(tree)
        assert R.validate(prog, 5)[0] in (R.OK, R.E_UNSUPPORTED)
        assert Tr(prog) == tree and P(Tr(prog)) == prog
        if R.validate(prog, 5)[0] == R.OK:
            assert coltt_amd.filter_prog_check(prog, 5) == R.validate(prog, 5)[1]
    for bad in (("and", 0), ("not", 0, 1), ("andnot", 0), ("xor", 0, 1), -1, ("all", 0), (), None, 1.5):
        with pytest.raises(ValueError):
            P(bad)
    with pytest.raises(coltt_amd.ColttError) as e:
        coltt_amd.filter_prog_check([0, 0], 1)
    assert e.value.code == R.E_INVALID


def test_entry_point_errors_that_need_no_device():
    L = coltt_amd.lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    prog = np.array([0, 1, A], np.int32); lv = np.array([11, 12], np.uint64); h = C.c_uint64(0); n = C.c_uint64(0)
    # unknown index handle
    assert L.coltt_hnsw_filter_eval(C.c_uint64(987654321), vp(prog), C.c_size_t(3), vp(lv), C.c_size_t(2), C.byref(n), C.byref(h)) == R.E_NOT_FOUND
    off = np.array([0, 3], np.uint64)
    assert L.coltt_hnsw_filter_eval_batch(C.c_uint64(987654321), vp(prog), vp(off), C.c_size_t(1), vp(lv), C.c_size_t(2), None, C.byref(h)) == R.E_NOT_FOUND
    # NULL out
    assert L.coltt_hnsw_filter_eval(C.c_uint64(987654321), vp(prog), C.c_size_t(3), vp(lv), C.c_size_t(2), C.byref(n), None) == R.E_INVALID
    # unknown filter handles
    assert L.coltt_hnsw_filter_ids(C.c_uint64(987654321), None, C.c_uint64(0), C.byref(n)) == R.E_NOT_FOUND
    assert L.coltt_hnsw_filter_info(C.c_uint64(987654321), None, None, None) == R.E_NOT_FOUND
