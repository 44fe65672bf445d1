"""The definition of coltt_hnsw_filter_eval (include/coltt_gpu.h, "Filter expressions") in numpy: a validator for postfix programmes and an
evaluator over boolean arrays of different lengths (leaves built at different ages of the index) plus the `live` array of the index now.
Shared by the CPU tests (tests/test_filter_expr_host.py) and the GPU tests (tests/test_gpu_hnsw_filter_expr.py)."""
import numpy as np

AND, OR, ANDNOT, NOT, ALL = -1, -2, -3, -4, -5
OK, E_INVALID, E_NOT_FOUND, E_UNSUPPORTED = 0, -1, -3, -4
MAX_DEPTH, MAX_PROG = 8, 4096


def validate(prog, n_leaves):
    """(code, deepest stack) by the rules of the header, in the order a left-to-right reader meets them"""
    prog = [int(v) for v in prog]
    if len(prog) == 0:
        return E_INVALID, 0
    if len(prog) > MAX_PROG:
        return E_UNSUPPORTED, 0
    depth = top = 0
    for v in prog:
        if v >= 0:
            if v >= n_leaves:
                return E_INVALID, top
            depth += 1
        elif v == ALL:
            depth += 1
        elif v == NOT:
            if depth < 1:
                return E_INVALID, top
        elif v in (AND, OR, ANDNOT):
            if depth < 2:
                return E_INVALID, top
            depth -= 1
        else:
            return E_INVALID, top
        if depth > MAX_DEPTH:
            return E_UNSUPPORTED, top
        top = max(top, depth)
    if depth != 1:
        return E_INVALID, top
    return OK, top


def evaluate(prog, leaves, live):
    """the allowed slots of a well-formed programme: a boolean array as long as `live`.  leaves[i]: a boolean array no longer than `live`
    (bit s past its end reads 0)."""
    live = np.asarray(live, bool)
    n = len(live)

    def wide(a):
        a = np.asarray(a, bool)
        assert len(a) <= n
        o = np.zeros(n, bool)
        o[:len(a)] = a
        return o

    st = []
    for v in prog:
        v = int(v)
        if v >= 0:
            st.append(wide(leaves[v]))
        elif v == ALL:
            st.append(live.copy())
        elif v == NOT:
            st.append(live & ~st.pop())
        else:
            b = st.pop(); a = st.pop()
            st.append(a & b if v == AND else a | b if v == OR else a & ~b)
    assert len(st) == 1
    return st[0] & live


def random_tree(rng, n_leaves, depth):
    """a random nested expression in the form coltt_amd.filter_postfix takes (binary nodes)"""
    if depth == 0 or rng.random() < 0.25:
        return "all" if rng.random() < 0.1 else int(rng.integers(0, n_leaves))
    op = ("and", "or", "andnot", "not")[int(rng.integers(0, 4))]
    if op == "not":
        return (op, random_tree(rng, n_leaves, depth - 1))
    return (op, random_tree(rng, n_leaves, depth - 1), random_tree(rng, n_leaves, depth - 1))


def tree_sets(tree, leaf_sets, live_set):
    """the same expression in Python set algebra (an independent statement of the semantics)"""
    if tree == "all" or tree == ("all",):
        return set(live_set)
    if isinstance(tree, int):
        return set(leaf_sets[tree])
    op = tree[0]
    if op == "not":
        return live_set - tree_sets(tree[1], leaf_sets, live_set)
    a = tree_sets(tree[1], leaf_sets, live_set); b = tree_sets(tree[2], leaf_sets, live_set)
    return a & b if op == "and" else a | b if op == "or" else a - b
