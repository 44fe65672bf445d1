"""Filtered search over the product-quantised HNSW walk restated on the CPU (include/coltt_gpu.h, coltt_hnsw_pq_search_filtered).
TEST INFRASTRUCTURE ONLY.

Plain numpy over the GPU's HBM-layout arrays (ExportRaw / FetchRows / PqCodes / the codebooks) with a `deleted` mask:

  table_distances(...)  d(q, v) for ALL slots at once: the quantiser's table over the query the index's distance sees, scaled by the
                        power of two that keeps it in binary16 range, every entry rounded to binary16, summed as two half-row f32 sums in
                        j order (oracle/pyref.py: csr_search_pq states the same arithmetic one slot at a time)
  walk(...)             coltt_hnsw_pq_search's walk with tombstones: result set, the vertices it expanded, counters
  allowed_set(...)      C as the definition states it — a SET: the live allowed vertices among the level-0 entry point and the rows of
                        the expanded vertices — and R, its cap smallest by (d bits, slot)
  search(...)           WALK for one query: R re-ranked with the index's exact distance (oracle.dist_rows), the k smallest
"""
import numpy as np

from oracle import oracle as O

import filtered_ref as F

NONE = 0xFFFFFFFF
f32 = np.float32


def table_distances(codebooks, pq_metric, codes, q_seen):
    """f32 [n]: d(q, slot) = S_lo + S_hi for every slot.  q_seen: the query as the index's distance sees it (filtered_ref.prep_query)."""
    cb = np.asarray(codebooks, f32); m = cb.shape[0]
    lut32 = O.pq_lut(pq_metric, cb, q_seen)                      # [m][C] f32: distFn(q_j, centroid[j][c])
    pos = lut32[lut32 > 0]
    big = pos.max() if len(pos) else f32(0)
    sc = f32(1)
    if np.isfinite(big):
        while f32(big * sc) > f32(32768):                        # the table scale: a power of two, exact
            sc = f32(sc * f32(0.5))
    with np.errstate(over="ignore"):
        lut = (lut32 * sc).astype(f32).astype(np.float16).astype(f32)   # entries rounded to binary16 (nearest even)
    codes = np.asarray(codes, np.uint8)
    js = 16 * (((m + 15) // 16 + 1) // 2)                        # the first ceil(P / 2) of the row's P = ceil(m / 16) 16-byte pieces
    lo = np.zeros(len(codes), f32); hi = np.zeros(len(codes), f32)
    for j in range(min(m, js)):                                  # f32 adds in j order from +0.0, per half row
        lo = (lo + lut[j][codes[:, j]]).astype(f32)
    for j in range(js, m):
        hi = (hi + lut[j][codes[:, j]]).astype(f32)
    return (lo + hi).astype(f32)


def key(d, slot):
    return (int(f32(d).view(np.uint32)) << 32) | int(slot)


def walk(adj0, upper_off, adjU, entry, entry_level, dall, ef, deleted=None):
    """The walk of coltt_hnsw_pq_search at ef over table distances dall [n].  Returns (result set: keys ascending, expanded slots in pop
    order, level-0 entry point, {n_dist, n_exp, n_hops})."""
    n = adj0.shape[0]
    deleted = np.zeros(n, bool) if deleted is None else deleted
    st = {"n_dist": 0, "n_exp": 0, "n_hops": 0}
    if entry < 0:
        return [], [], -1, st

    def live_row(r):
        r = r[r != NONE]
        return r[~deleted[r]]                                    # tombstoned neighbours are skipped before anything else

    ep = int(entry); min_d = dall[ep]; st["n_dist"] += 1
    for lvl in range(int(entry_level), 0, -1):                   # greedyClosestNeighbor: the strict minimum, first position on ties
        while True:
            closest = -1
            for s in live_row(adjU[int(upper_off[ep]) + lvl - 1]):
                st["n_dist"] += 1
                if dall[s] < min_d:
                    min_d, closest = dall[s], int(s)
            st["n_hops"] += 1
            if closest < 0:
                break
            ep = closest
    st["n_dist"] += 1                                            # searchLevel re-evaluates the entry point
    res = [[key(dall[ep], ep), False]]
    visited = {ep}
    expanded = []
    while True:
        ci = next((i for i, e in enumerate(res) if not e[1]), -1)
        if ci < 0:
            break
        res[ci][1] = True
        lower_bound = np.uint32(res[-1][0] >> 32).view(f32)      # stale: sampled once per pop
        free = ef - len(res)
        full_at_pop = free == 0
        c = res[ci][0] & 0xFFFFFFFF
        expanded.append(int(c))
        st["n_exp"] += 1
        adm = []
        for s in live_row(adj0[c]):                              # canonical order: ascending slot
            s = int(s); d = dall[s]
            if full_at_pop:                                      # bounded visiting: the bound before the visited test
                if not d < lower_bound or s in visited:
                    continue
                visited.add(s); st["n_dist"] += 1
                adm.append([key(d, s), False])
                continue
            if s in visited:
                continue
            visited.add(s); st["n_dist"] += 1
            if free > 0:
                adm.append([key(d, s), False]); free -= 1
            elif d < lower_bound:
                adm.append([key(d, s), False])
        res = sorted(res + adm, key=lambda e: e[0])[:ef]
    return [e[0] for e in res], expanded, ep, st


def allowed_set(adj0, expanded, ep, dall, allow, deleted, cap):
    """(C, R): C = the set of live allowed vertices among the level-0 entry point and every listed neighbour of every expanded vertex —
    the union of whole rows, whether or not a neighbour was fresh, under the bound or admitted; R = its cap smallest keys, ascending."""
    if ep < 0:
        return set(), []
    n = adj0.shape[0]
    allow = np.asarray(allow, bool)
    allow = np.concatenate([allow, np.zeros(n - len(allow), bool)]) if len(allow) < n else allow   # slots past the filter's: not allowed
    deleted = np.zeros(n, bool) if deleted is None else deleted
    listed = adj0[np.array(expanded, np.int64)].ravel() if expanded else np.zeros(0, np.uint32)
    cand = np.unique(np.concatenate([listed[listed != NONE], np.array([ep], np.uint32)])).astype(np.int64)
    C = set(int(s) for s in cand[allow[cand] & ~deleted[cand]])
    R = sorted(key(dall[s], s) for s in C)[:cap]
    return C, R


def cap_of(ef_walk, k, rerank):
    return ef_walk if rerank == 0 else min(max(rerank, k), ef_walk)


def rerank_set(rows, metric, q_seen, R, k):
    """every member of R gets the index's exact distance; the k smallest by (exact score bits, slot)"""
    slots = np.array([x & 0xFFFFFFFF for x in R], np.int64)
    if len(slots) == 0:
        return slots, np.zeros(0, f32)
    d = O.dist_rows(metric, q_seen, rows[slots])
    order = np.lexsort((slots, d.view(np.uint32)))[:k]
    return slots[order], d[order]


class Walked:
    """one (query, ef, filter) walk; every `rerank` is derived from it (the walk does not depend on rerank)"""

    def __init__(self, rows, g, metric, codebooks, pq_metric, codes, q_seen, ef_walk, allow, deleted=None):
        self.rows, self.metric, self.q, self.ef = rows, metric, q_seen, ef_walk
        self.dall = table_distances(codebooks, pq_metric, codes, q_seen)
        self.res, self.expanded, self.ep, self.stats = walk(g["adj0"], g["upper_off"], g["adjU"], g["entry"], g["entry_level"], self.dall, ef_walk, deleted)
        self.C, self.R = allowed_set(g["adj0"], self.expanded, self.ep, self.dall, allow, deleted, ef_walk)   # the largest cap; smaller ones are prefixes

    def answer(self, k, rerank):
        """(slots, exact scores, |R|) of the WALK answer"""
        R = self.R[:cap_of(self.ef, k, rerank)]
        s, v = rerank_set(self.rows, self.metric, self.q, R, k)
        return s, v, len(R)


def search(rows, g, metric, quant, codebooks, pq_metric, codes, query, k, ef_walk, rerank, allow, deleted=None):
    w = Walked(rows, g, metric, codebooks, pq_metric, codes, F.prep_query(metric, quant, query), ef_walk, allow, deleted)
    return w.answer(k, rerank) + (w.stats,)


# ---- the inputs the CPU suite (tests/test_filtered_pq_ref.py) and the GPU suite (tests/test_gpu_hnsw_pq_filter.py) share ----------------
# (metric, rows, d, sub-vectors, centroids, quantiser metric): run-time pieces with 32-entry rows | LS 5 / NP 4, bias form |
# LS 8 / NP 2, add-per-lookup form | the fully run-time form
CASES = [("l2", "f32", 64, 16, 17, O.PQ_EUCLIDEAN), ("cos", "f16", 128, 64, 32, O.PQ_COSINE), ("cos", "f32", 64, 32, 256, O.PQ_EUCLIDEAN),
         ("l2", "f16", 96, 32, 64, O.PQ_EUCLIDEAN)]
WIDE = ("l2", "f32", 64, 16, 32, O.PQ_EUCLIDEAN)   # graph m = 32: level-0 rows of 64, two chunks per expansion
N, N_WIDE, K, NQ = 3000, 1500, 10, 6
GRAPH = dict(m=8, ef=32, ef_construction=40)
GRAPH_WIDE = dict(m=32, ef=32, ef_construction=40)
WALK_FRACS, WALK_EFS, WALK_RERANKS = (0.5, 0.1, 0.01), (48, 300), (0, 12, 3, 1000)
PROP_FRACS, PROP_EF = (0.3, 0.1, 0.01), 64


def case_seed(d, m):
    return 7000 + d + m


def case_data(case, n):
    """(X, levels, queries) of a case"""
    seed = case_seed(case[2], case[3])
    return O.fill_normal(seed, (n, case[2])), O.levels(seed + 1, n), O.fill_normal(seed + 7, (NQ, case[2]))


def allow_mask(case, n, frac):
    return np.random.default_rng(case_seed(case[2], case[3]) * 1000 + int(frac * 1000)).random(n) < frac
