"""The definition of coltt_hnsw_filter_eval_attr (include/coltt_gpu.h, "Attribute columns and predicates") in numpy: filter_expr_ref.evaluate
with predicate leaves.  A column is (values, set_mask, covered): values an int64 or float64 array, set_mask a boolean array of the same length,
covered the slots the column covers (slots at or past it hold no value).  A predicate is (column index, op, operand).
Shared by tests/test_attr_filter_ref.py (CPU) and tests/test_gpu_attr_filter.py (GPU)."""
import numpy as np

import filter_expr_ref as R

I64, F64 = 0, 1
EQ, NE, GT, GE, LT, LE, SET = range(7)
OPS = (EQ, NE, GT, GE, LT, LE, SET)
DTYPE = {I64: np.int64, F64: np.float64}


def compare(op, values, operand):
    """values OP operand elementwise in the array's own dtype (int64 stays int64: nothing goes through a double)"""
    values = np.asarray(values)
    if op == SET:
        return np.ones(len(values), bool)
    o = values.dtype.type(operand)
    return {EQ: values == o, NE: values != o, GT: values > o, GE: values >= o, LT: values < o, LE: values <= o}[op]


def pred_mask(column, op, operand, n):
    """the predicate's bits over n slots: set and cmp below the coverage, 0 at and past it"""
    values, set_mask, covered = column
    covered = min(int(covered), n, len(values))
    o = np.zeros(n, bool)
    o[:covered] = np.asarray(set_mask[:covered], bool) & compare(op, np.asarray(values)[:covered], operand)
    return o


def evaluate(prog, leaves, columns, preds, live):
    """filter_expr_ref.evaluate over the leaf table extended by the predicates' masks: a value v >= len(leaves) is predicate v - len(leaves)"""
    n = len(live)
    table = list(leaves) + [pred_mask(columns[c], op, operand, n) for c, op, operand in preds]
    return R.evaluate(prog, table, live)


def evaluate_loop(prog, leaves, columns, preds, live):
    """the same, slot by slot in plain Python (an independent statement of the semantics, for tiny inputs)"""
    n = len(live)
    out = []
    for s in range(n):
        st = []
        for v in prog:
            v = int(v)
            if v >= 0 and v < len(leaves):
                st.append(bool(leaves[v][s]) if s < len(leaves[v]) else False)
            elif v >= 0:
                c, op, operand = preds[v - len(leaves)]
                values, set_mask, covered = columns[c]
                if s >= covered or s >= len(values) or not set_mask[s]:
                    st.append(False)
                elif op == SET:
                    st.append(True)
                else:
                    a = values[s].item(); b = np.asarray(values).dtype.type(operand).item()
                    st.append({EQ: a == b, NE: a != b, GT: a > b, GE: a >= b, LT: a < b, LE: a <= b}[op])
            elif v == R.ALL:
                st.append(bool(live[s]))
            elif v == R.NOT:
                a = st.pop()
                st.append(bool(live[s]) and not a)
            else:
                b = st.pop(); a = st.pop()
                st.append((a and b) if v == R.AND else (a or b) if v == R.OR else (a and not b))
        assert len(st) == 1
        out.append(st[0] and bool(live[s]))
    return np.array(out, bool)
