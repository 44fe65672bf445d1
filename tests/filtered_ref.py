"""Filtered HNSW search restated on the CPU (include/coltt_gpu.h, "Filtered HNSW search").  TEST INFRASTRUCTURE ONLY.

Built on the oracle's pieces: the canonical walk of csr_search (oracle/coltt_oracle.cpp: search_level_canon over the GPU's HBM-layout
arrays — ExportRaw / FetchRows), its distance (oracle.dist_rows, AVX order) and the query preparation (normalize / lower).

  walk(...)       WALK: the canonical Hnsw.Search at ef, plus the allowed set R (the k smallest live allowed vertices whose distance the
                  level-0 walk holds: the level-0 entry point and every neighbour it evaluates)
  exact(...)      EXACT: the k nearest live allowed vertices, ascending by (score bits, slot)
  auto_path(...)  AUTO: which path serves a call, at which walk breadth
"""
import numpy as np

from oracle import oracle as O

AUTO, WALK, EXACT = 0, 1, 2
EF_MAX = 4096
ROWS_PER_EF = 32
NONE = 0xFFFFFFFF


def auto_path(allowed, n_live, ef, mode=AUTO):
    """(path, ef_walk) for a call at walk breadth ef = max(ef_override or cfg.ef, k); ef_walk is 0 when EXACT serves it"""
    if mode == WALK:
        return WALK, ef
    if mode == EXACT or allowed == 0:
        return EXACT, 0
    ef_need = -(-ef * n_live // allowed)
    ef_walk = min(EF_MAX, max(ef, ef_need))
    if ef_need > EF_MAX or allowed <= ROWS_PER_EF * ef_walk:
        return EXACT, 0
    return WALK, ef_walk


def decode(quant, rows):
    """stored rows (FetchRows) -> the f32 values the distance sees"""
    if quant == O.Q_NONE:
        return np.ascontiguousarray(rows, np.float32)
    if quant == O.Q_F8:
        return O.f8_decode(rows)
    return O.f16_decode(rows)   # "f16" and "bf16": the reference codes both as binary16 (oracle: lower / raise)


def prep_query(metric, quant, q):
    """the query as the index's distance sees it: cosine normalises it, a quantised index lowers it (as Search does)"""
    q = np.ascontiguousarray(q, np.float32).reshape(-1)
    if metric == O.COSINE:
        q = O.normalize(q)
    if quant != O.Q_NONE:
        q = decode(quant, O.lower(quant, q))
    return q


def csr_from_export(g, m_max0, m_max):
    """oracle.Hnsw.export() -> the HBM layout (adj0 [n][m_max0] ascending slot, upper_off [n], adjU [rows][m_max], NONE-padded)"""
    lv = g["levels"]; off = g["row_offsets"]; nb = g["nbr"]; n = len(lv)
    adj0 = np.full((n, m_max0), NONE, np.uint32); uo = np.zeros(n, np.uint32)
    adjU = np.full((max(int(lv.sum()), 1), m_max), NONE, np.uint32)
    row = 0; urow = 0
    for s in range(n):
        uo[s] = urow
        for lvl in range(int(lv[s]) + 1):
            e = np.sort(nb[off[row]:off[row + 1]].astype(np.uint32))
            if lvl == 0:
                adj0[s, :len(e)] = e
            else:
                adjU[urow, :len(e)] = e; urow += 1
            row += 1
    return adj0, uo, adjU


def key(d, slot):
    return (int(np.float32(d).view(np.uint32)) << 32) | int(slot)


def walk(rows, adj0, upper_off, adjU, metric, entry, entry_level, q, k, ef, allow, deleted=None):
    """WALK for one prepared query.  rows: f32 [n][dim] (decoded); allow, deleted: bool [n].
    Returns (slots, scores, {n_dist, n_exp, n_hops})."""
    n = rows.shape[0]
    deleted = np.zeros(n, bool) if deleted is None else deleted
    st = {"n_dist": 0, "n_exp": 0, "n_hops": 0}
    if entry < 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32), st

    def D(slots):
        st["n_dist"] += len(slots)
        return O.dist_rows(metric, q, rows[slots])

    ep = int(entry); min_d = D([ep])[0]
    for lvl in range(entry_level, 0, -1):   # greedyClosestNeighbor: move to the strict minimum until nothing improves
        while True:
            r = adjU[int(upper_off[ep]) + lvl - 1]
            r = r[r != NONE]; r = r[~deleted[r]]
            st["n_hops"] += 1
            closest = -1
            if len(r):
                for s, d in zip(r, D(r)):
                    if d < min_d:
                        min_d, closest = d, int(s)
            if closest < 0:
                break
            ep = closest
    d0 = D([ep])[0]                          # searchLevel re-evaluates the entry point
    res = [[key(d0, ep), False]]             # the result set, ascending by (d bits, slot), with an `expanded` flag
    visited = {ep}
    R = [key(d0, ep)] if allow[ep] and not deleted[ep] else []
    while True:
        ci = next((i for i, e in enumerate(res) if not e[1]), -1)
        if ci < 0:
            break
        res[ci][1] = True
        lower_bound = np.uint32(res[-1][0] >> 32).view(np.float32)
        free = ef - len(res)
        c = res[ci][0] & 0xFFFFFFFF
        st["n_exp"] += 1
        r = adj0[c]; r = r[r != NONE]
        fresh = [int(s) for s in r if not deleted[s] and s not in visited]
        visited.update(fresh)
        if not fresh:
            continue
        ds = D(np.array(fresh, np.int64))
        adm = []
        for s, d in zip(fresh, ds):
            if free > 0:
                adm.append(key(d, s)); free -= 1
            elif d < lower_bound:
                adm.append(key(d, s))
            if allow[s]:
                R.append(key(d, s))
        res = sorted(res + [[a, False] for a in adm], key=lambda e: e[0])[:ef]
    R = sorted(R)[:k]
    return (np.array([x & 0xFFFFFFFF for x in R], np.int64),
            np.array([np.uint32(x >> 32) for x in R], np.uint32).view(np.float32), st)


def exact(rows, metric, q, k, allow, deleted=None):
    """EXACT for one prepared query: (slots, scores) of the k nearest live allowed rows by (score bits, slot)"""
    ok = allow.copy()
    if deleted is not None:
        ok &= ~deleted
    slots = np.nonzero(ok)[0]
    if len(slots) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    d = O.dist_rows(metric, q, rows[slots])
    order = np.lexsort((slots, d.view(np.uint32)))[:k]
    return slots[order].astype(np.int64), d[order]
