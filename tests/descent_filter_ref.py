"""The greedy descent of the 8-bit row-filter walks (coltt_amd/csrc/hnsw_walk2.hpp: greedy_level8 / greedy_level8_filtered), replayed on the host over
the index's HBM-layout arrays (upper_off, adjU): once with the exact distances of every listed neighbour, once through the certified filter — the
headers' own bound (row_filter8.hpp / row_filter8i.hpp compiled with g++) against curd, the exact distance for what it cannot reject.  Both replays
record (level, cur, curd bits, n_dist, n_hops) after every hop; test_descent_filter_host.py asserts the two records equal, test_gpu_descent_filter.py
uses the exact replay to show that a fixture meets the cases it was built for."""
import numpy as np

import row_filter8i_ref as R8
import row_filter_probe_ref as R
from oracle import oracle as O
from row_filter8_ref import quantise

NONE = 0xFFFFFFFF


def f32bits(x):
    return int(np.float32(x).view(np.uint32))


class Shadow:
    """what the index keeps per slot for the 8-bit filter: codes, (scale, error norm), the squared norm the exact kernel divides by"""

    def __init__(self, rows):
        self.rows = np.ascontiguousarray(rows, np.float32)
        q = [quantise(r) for r in self.rows]
        self.codes = np.stack([c for c, _, _ in q]); self.s = np.array([s for _, s, _ in q], np.float32); self.e = np.array([e for _, _, e in q], np.float32)
        with np.errstate(all="ignore"):
            self.rn = np.array([O.cosine_parts(r, r)[1] for r in self.rows], np.float32)


def exact_distances(qe, rows):
    with np.errstate(all="ignore"):
        return np.asarray(O.dist_rows(O.COSINE, qe, np.ascontiguousarray(rows, np.float32)), np.float32)


class Bound:
    """d_lo of one (normalised) query against chosen slots, by the header of `kind` ("8": f32 query, "8i": quantised query)"""

    def __init__(self, kind, libs, sh, qe):
        self.kind, self.sh, self.qe = kind, sh, np.ascontiguousarray(qe, np.float32)
        self.L8, self.L8i = libs
        with np.errstate(all="ignore"):
            self.qn = np.float32(O.cosine_parts(self.qe, self.qe)[1])
        if kind == "8i":
            self.t, self.qh, _, _, self.eq = R8.quantise_query(self.qe)

    def d_lo(self, slots):
        sh = self.sh; slots = np.asarray(slots, np.int64); dim = sh.rows.shape[1]
        if self.kind == "8i":
            I = R8.int_dot(self.qh, sh.codes[slots])
            return R8.dlo8i(self.L8i, I, self.t, self.eq, sh.s[slots], sh.e[slots], dim, self.qn, sh.rn[slots])
        G = np.array([R.fused_kernel_order_sum(self.L8, self.qe, sh.codes[j].astype(np.float32)) for j in slots], np.float32)
        return R.dlo8(self.L8, G, sh.s[slots], sh.e[slots], dim, self.qn, sh.rn[slots])

    def rejects(self, d_lo, curd):
        return bool(self.L8.rf_rejects(float(d_lo), float(curd)))   # row_filter_rejects: no verdict on anything non-finite


def descend(sh, upper_off, adjU, entry, entry_level, qe, deleted=None, bound=None):
    """greedy_level8 (bound None) or greedy_level8_filtered over the arrays.  Returns (trace, events, counters): trace = [(level, cur, curd bits,
    n_dist, n_hops)] after every hop; events counts what the exact distances of the hop's neighbours were relative to curd (from the exact values,
    whichever way the hop was decided); counters = (shadow rows, rejected, f32 rows) of the filtered replay"""
    rows = sh.rows
    cur = int(entry)
    curd = exact_distances(qe, rows[cur:cur + 1])[0]
    n_dist, n_hops = 1, 0
    trace = [(int(entry_level) + 1, cur, f32bits(curd), n_dist, n_hops)]
    ev = {"equal_no_move": 0, "ulp_below_move": 0, "tie_of_survivors": 0, "no_verdict": 0, "tombstone": 0, "hops": 0}
    n_sh = n_rej = n_f32 = 0
    for level in range(int(entry_level), 0, -1):
        while True:
            row = adjU[int(upper_off[cur]) + level - 1]
            idx = [i for i, nb in enumerate(row) if nb != NONE]
            dead = [i for i in idx if deleted is not None and deleted[int(row[i])]]
            ev["tombstone"] += len(dead)
            idx = [i for i in idx if i not in dead]
            n_dist += len(idx); n_hops += 1; ev["hops"] += 1
            best = None
            if idx:
                nbs = np.array([int(row[i]) for i in idx], np.int64)
                d = exact_distances(qe, rows[nbs])
                used = d.copy()
                if bound is not None:
                    dl = bound.d_lo(nbs)
                    rej = np.array([bound.rejects(x, curd) for x in dl])
                    used[rej] = dl[rej]
                    n_sh += len(idx); n_rej += int(rej.sum()); n_f32 += int((~rej).sum())
                    ev["no_verdict"] += int(np.count_nonzero(~np.isfinite(dl)))
                    assert np.all(dl[rej] <= d[rej]) and np.all(dl[rej] >= curd), "a rejected neighbour's bound lies in [curd, d]"
                keys = [(f32bits(u) << 32) | i for u, i in zip(used, idx)]
                k = int(np.argmin(np.array(keys, np.uint64)))
                best = (np.float32(used[k]), int(nbs[k]))
                below = d < curd
                if np.any(d == curd) and not np.any(below):
                    ev["equal_no_move"] += 1
                if np.any(below) and f32bits(d[below].min()) == f32bits(curd) - 1:
                    ev["ulp_below_move"] += 1
                if np.any(below) and np.count_nonzero(d == d[below].min()) > 1:
                    ev["tie_of_survivors"] += 1
            if best is not None and best[0] < curd:
                curd, cur = best
                trace.append((level, cur, f32bits(curd), n_dist, n_hops))
            else:
                trace.append((level, cur, f32bits(curd), n_dist, n_hops))
                break
    return trace, ev, (n_sh, n_rej, n_f32)
