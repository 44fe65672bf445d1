"""Hnsw — GPU-backed stand-in for *vectorindex.Hnsw (core/vectorindex/hnsw.go:43-54)."""
import ctypes as C

import numpy as np

from . import _lib as L


class HnswCfg(C.Structure):
    """hnswConfig (core/vectorindex/hnsw_config.go:135-162); -1 = derive the default."""
    _fields_ = [("m", C.c_int32), ("m_max", C.c_int32), ("m_max0", C.c_int32), ("ef", C.c_int32),
                ("ef_construction", C.c_int32), ("algo", C.c_int32), ("level_multiplier", C.c_float),
                ("extend_candidates", C.c_int32), ("keep_pruned", C.c_int32)]

    @staticmethod
    def default(**kw):
        c = HnswCfg(16, -1, -1, 20, 200, 0, -1.0, 0, 1)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


class HnswStats(C.Structure):
    _fields_ = [("n_dist", C.c_uint64), ("n_exp", C.c_uint64), ("n_hops", C.c_uint64), ("n_visit_resets", C.c_uint64)]


FILTER_AUTO, FILTER_WALK, FILTER_EXACT = 0, 1, 2


class HnswFilterStats(C.Structure):
    _fields_ = [("n_dist", C.c_uint64), ("n_exp", C.c_uint64), ("n_hops", C.c_uint64), ("n_visit_resets", C.c_uint64),
                ("ef_walk", C.c_uint32), ("path", C.c_int32), ("n_exact_rows", C.c_uint64)]


# filter expressions (coltt_hnsw_filter_eval; include/coltt_gpu.h, "Filter expressions"): the operators of a postfix programme
FOP_AND, FOP_OR, FOP_ANDNOT, FOP_NOT, FOP_ALL = -1, -2, -3, -4, -5
_FOP_BY_NAME = {"and": FOP_AND, "or": FOP_OR, "andnot": FOP_ANDNOT, "not": FOP_NOT, "all": FOP_ALL}
_FOP_ARITY = {FOP_AND: 2, FOP_OR: 2, FOP_ANDNOT: 2, FOP_NOT: 1, FOP_ALL: 0}


def filter_postfix(tree):
    """A nested expression -> the postfix programme of coltt_hnsw_filter_eval.  A node is a leaf index (int >= 0), the string "all", or a
    tuple (op, operand, ...) with op one of "and", "or", "andnot", "not"; "and" / "or" take two or more operands and fold from the left
    (the shape of evaluateCompositeFilter, pkg/inverted/search.go:50-77), "andnot" takes two, "not" one."""
    out = []

    def walk(t):
        if isinstance(t, (int, np.integer)) and not isinstance(t, bool):
            if t < 0:
                raise ValueError(f"filter_postfix: leaf index {t}")
            out.append(int(t))
            return
        if isinstance(t, str):
            t = (t,)
        if not isinstance(t, tuple) or not t or not isinstance(t[0], str) or t[0].lower() not in _FOP_BY_NAME:
            raise ValueError(f"filter_postfix: not an expression: {t!r}")
        op = _FOP_BY_NAME[t[0].lower()]
        args = t[1:]
        ar = _FOP_ARITY[op]
        if (op in (FOP_AND, FOP_OR) and len(args) < 2) or (op not in (FOP_AND, FOP_OR) and len(args) != ar):
            raise ValueError(f"filter_postfix: {t[0]!r} with {len(args)} operands")
        if ar == 0:
            out.append(op)
            return
        walk(args[0])
        if ar == 1:
            out.append(op)
        for a in args[1:]:
            walk(a)
            out.append(op)

    walk(tree)
    return out


def filter_tree(prog):
    """The inverse of filter_postfix for a well-formed programme: nested binary tuples."""
    names = {v: k for k, v in _FOP_BY_NAME.items()}
    st = []
    for v in prog:
        v = int(v)
        if v >= 0:
            st.append(v)
        elif v == FOP_ALL:
            st.append("all")
        elif v == FOP_NOT:
            st.append(("not", st.pop()))
        elif v in names:
            b = st.pop(); a = st.pop()
            st.append((names[v], a, b))
        else:
            raise ValueError(f"filter_tree: unknown operator {v}")
    if len(st) != 1:
        raise ValueError("filter_tree: the programme does not leave exactly one value")
    return st[0]


def filter_prog_check(prog, n_leaves):
    """coltt_hnsw_filter_prog_check_host (no device): the deepest stack of a well-formed programme; raises ColttError otherwise."""
    p = np.ascontiguousarray(np.asarray(prog, dtype=np.int32).reshape(-1))
    d = C.c_uint32(0)
    L.check(L.lib().coltt_hnsw_filter_prog_check_host(L.vp(p), C.c_size_t(p.size), C.c_size_t(int(n_leaves)), C.byref(d)))
    return d.value


def _prog_array(prog):
    if isinstance(prog, (tuple, str)):
        prog = filter_postfix(prog)
    return np.ascontiguousarray(np.asarray(prog, dtype=np.int32).reshape(-1))


class HnswCompactStats(C.Structure):
    """coltt_hnsw_compact_stats (include/coltt_gpu.h, "HNSW compaction")"""
    _fields_ = [("slots_before", C.c_uint64), ("slots_after", C.c_uint64), ("upper_rows_before", C.c_uint64), ("upper_rows_after", C.c_uint64),
                ("edges_dropped", C.c_uint64), ("rows_moved", C.c_uint64), ("bytes_moved", C.c_uint64), ("ms", C.c_float)]


def compact_map_host(del_bits, n_slots, levels):
    """coltt_hnsw_compact_map_host (no device): the plan of Hnsw.Compact.  del_bits: uint32 words, bit s % 32 of word s // 32 = slot s is
    tombstoned (None = none is); levels [n_slots].  Returns (new_of_old [n_slots], 0xffffffff for a dead slot; new_upper_off [live], indexed by
    NEW slot, 0xffffffff for a vertex of level 0; live; upper_rows)."""
    n = int(n_slots)
    db = None if del_bits is None else np.ascontiguousarray(np.asarray(del_bits, dtype=np.uint32).reshape(-1))
    if db is not None and db.size * 32 < n:
        raise ValueError(f"compact_map_host: {db.size} bitmap words for {n} slots")
    lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32).reshape(-1))
    if lv.size < n:
        raise ValueError(f"compact_map_host: {lv.size} levels for {n} slots")
    new_of_old = np.empty(n, np.uint32); upper_off = np.empty(n, np.uint32)
    live = C.c_uint64(0); up = C.c_uint64(0)
    L.check(L.lib().coltt_hnsw_compact_map_host(L.vp(db), C.c_uint64(n), L.vp(lv), L.vp(new_of_old), L.vp(upper_off), C.byref(live), C.byref(up)))
    return new_of_old, upper_off[:live.value].copy(), live.value, up.value


class HnswCarryStats(C.Structure):
    """coltt_hnsw_carry_stats (include/coltt_gpu.h, "Carrying resident filters and attribute columns through a compaction")"""
    _fields_ = [("filters", C.c_uint64), ("columns", C.c_uint64), ("bitmap_words", C.c_uint64), ("list_entries", C.c_uint64),
                ("column_values", C.c_uint64), ("ms", C.c_float)]


def _carry_args(bits, del_bits, n_slots):
    n = int(n_slots)
    b = np.ascontiguousarray(np.asarray(bits, dtype=np.uint32))
    db = None if del_bits is None else np.ascontiguousarray(np.asarray(del_bits, dtype=np.uint32).reshape(-1))
    if db is not None and db.size * 32 < n:
        raise ValueError(f"carry_bits: {db.size} tombstone words for {n} slots")
    dead = 0
    if db is not None and n:
        w = db[:(n + 31) // 32].copy()
        if n & 31:
            w[-1] &= np.uint32((1 << (n & 31)) - 1)
        dead = int(np.unpackbits(w.view(np.uint8)).sum())
    return n, b, db, n - dead


def carry_bits_host(bits, del_bits, n_slots):
    """coltt_hnsw_carry_bits_host (no device): the definition of a bitmap carried through a compaction.  bits: uint32 words over the old slots
    (words it lacks read as 0); del_bits: the tombstones (None = none).  Returns (out_bits [ceil(live / 32)], allowed, live): bit new(s) of
    out_bits = bit s of bits for every live slot s."""
    n, b, db, live = _carry_args(bits, del_bits, n_slots)
    b = b.reshape(-1)
    out = np.zeros((live + 31) // 32, np.uint32)
    al = C.c_uint64(0); lv = C.c_uint64(0)
    L.check(L.lib().coltt_hnsw_carry_bits_host(L.vp(b), C.c_uint64(b.size), L.vp(db), C.c_uint64(n), L.vp(out), C.byref(al), C.byref(lv)))
    assert lv.value == live
    return out, al.value, lv.value


def carry_bits_device(bits, del_bits, n_slots, with_lists=False):
    """coltt_hnsw_carry_bits_device: the kernels of Hnsw.CompactCarry on bitmaps of the caller, no index.  bits: [n_bitmaps, n_words] uint32.
    Returns (out_bits [n_bitmaps, ceil(live / 32)], allowed [n_bitmaps]) and with with_lists=True also a list of n_bitmaps uint32 arrays: each
    bitmap's new slots, ascending."""
    n, b, db, live = _carry_args(bits, del_bits, n_slots)
    if b.ndim != 2:
        raise ValueError("carry_bits_device: bits must be [n_bitmaps, n_words]")
    nb, nw = b.shape
    out = np.zeros((nb, (live + 31) // 32), np.uint32)
    al = np.zeros(max(nb, 1), np.uint64)
    lists = off = None
    if with_lists:
        off = np.arange(nb, dtype=np.uint64) * np.uint64(max(live, 1))   # no list is longer than the live count
        lists = np.zeros(max(nb * max(live, 1), 1), np.uint32)
    L.check(L.lib().coltt_hnsw_carry_bits_device(L.vp(b), C.c_uint64(nb), C.c_uint64(nw), L.vp(db), C.c_uint64(n), L.vp(out), L.vp(al), L.vp(lists),
                                                 L.vp(off)))
    al = al[:nb]
    if with_lists:
        return out, al, [lists[int(off[p]):int(off[p]) + int(al[p])].copy() for p in range(nb)]
    return out, al


class PlanFactsC(C.Structure):
    """coltt_hnsw_plan_facts (include/coltt_gpu.h): what the search plan reads of an index"""
    _fields_ = [("dim", C.c_uint32), ("metric", C.c_int32), ("quant", C.c_int32), ("m_max0", C.c_uint32), ("stride", C.c_uint64), ("slots", C.c_uint64),
                ("r8", C.c_int32), ("shadow8", C.c_int32), ("shadow16", C.c_int32), ("vis_ready", C.c_int32), ("vis_regions", C.c_uint32)]


class SearchPlanC(C.Structure):
    """coltt_hnsw_search_plan (include/coltt_gpu.h): which kernel a search launches, and how"""
    _fields_ = [("family", C.c_int32), ("ef", C.c_uint32), ("ef_pad", C.c_uint32), ("hcap", C.c_uint32), ("lds", C.c_uint64), ("vis_kind", C.c_int32),
                ("w2", C.c_int32), ("bloom_words", C.c_uint32), ("r8", C.c_int32), ("ev8", C.c_int32), ("nt", C.c_int32), ("filter", C.c_int32),
                ("upper", C.c_uint32), ("v16_bits", C.c_uint32), ("v16_limit", C.c_uint32), ("per_cu", C.c_uint32), ("grid", C.c_uint32),
                ("rows8_launch", C.c_int32), ("lat_seq", C.c_int32), ("lat_helpers", C.c_int32)]


SEARCH_PLAN_DTYPE = np.dtype(SearchPlanC)   # an array of plans as numpy records
PLAN_LATENCY, PLAN_WALK2, PLAN_ONE_WAVE = 0, 1, 2   # SearchPlanC.family
ROWF_UPPER_FILTER, ROWF_UPPER_CACHED = 1, 2         # SearchPlanC.upper


def search_plan_host(facts, nq, k, ef, force=0):
    """coltt_hnsw_search_plan_host (no device): the plan of a search of nq queries for k answers at ef over an index with these facts (a PlanFactsC or a
    dict of its fields) under the knobs os.environ holds now — a dict of SearchPlanC's fields; raises ColttError where the search would"""
    f = facts if isinstance(facts, PlanFactsC) else PlanFactsC(**{n: int(v) for n, v in facts.items()})
    p = SearchPlanC()
    L.check(L.lib().coltt_hnsw_search_plan_host(C.byref(f), C.c_size_t(int(nq)), C.c_uint32(int(k)), C.c_uint32(int(ef)), C.c_int(int(force)), C.byref(p)))
    return {n: getattr(p, n) for n, _ in SearchPlanC._fields_}


class HnswFilter:
    """An allow-list of ids against one index (coltt_hnsw_filter_create; include/coltt_gpu.h, "Filtered HNSW search" — an extension the
    reference does not have).  `.allowed` = the live vertices it allows."""

    def __init__(self, index, ids):
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
        h = C.c_uint64(0); n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_filter_create(index.h, L.vp(a), C.c_size_t(a.size), C.byref(n), C.byref(h)))
        self.h, self.allowed = h, n.value

    @classmethod
    def _from_handle(cls, h, allowed):
        o = cls.__new__(cls)
        o.h, o.allowed = C.c_uint64(int(h)), int(allowed)
        return o

    def info(self):
        """coltt_hnsw_filter_info: the handle of the index it was built for, its allowed count, the slots it covers"""
        ix = C.c_uint64(0); a = C.c_uint64(0); s = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_filter_info(self.h, C.byref(ix), C.byref(a), C.byref(s)))
        return {"index": ix.value, "allowed": a.value, "slots": s.value}

    def ids(self, cap=None):
        """coltt_hnsw_filter_ids: the allowed ids in ascending slot order (the first `cap` of them), gathered on the device"""
        n = C.c_uint64(0)
        if cap is None:
            cap = self.allowed
        o = np.zeros(int(cap), np.uint64)
        L.check(L.lib().coltt_hnsw_filter_ids(self.h, L.vp(o), C.c_uint64(int(cap)), C.byref(n)))
        return o[:min(int(cap), n.value)]

    def close(self):
        if getattr(self, "h", None) is not None:
            L.lib().coltt_hnsw_filter_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# attribute columns and predicates (include/coltt_gpu.h, "Attribute columns and predicates")
ATTR_I64, ATTR_F64 = 0, 1
CMP_EQ, CMP_NE, CMP_GT, CMP_GE, CMP_LT, CMP_LE, CMP_SET = range(7)
_ATTR_DTYPE = {ATTR_I64: np.int64, ATTR_F64: np.float64}


class _AttrValue(C.Union):
    _fields_ = [("i64", C.c_int64), ("f64", C.c_double)]


class AttrPred(C.Structure):
    """coltt_attr_pred"""
    _fields_ = [("column", C.c_uint64), ("op", C.c_int32), ("reserved", C.c_int32), ("value", _AttrValue)]


def attr_cmp_host(type_, op, operand, value, is_set=True):
    """coltt_attr_cmp_host (no device): is_set and (value OP operand) in the column type's arithmetic; raises ColttError for an unknown type or
    op and for NaN."""
    dt = _ATTR_DTYPE.get(int(type_), np.int64)
    o = np.array([0 if operand is None else operand], dt); v = np.array([0 if value is None else value], dt)
    rc = L.lib().coltt_attr_cmp_host(C.c_int(int(type_)), C.c_int(int(op)), L.vp(o), L.vp(v), C.c_int(1 if is_set else 0))
    if rc < 0:
        L.check(rc)
    return bool(rc)


class HnswAttrColumn:
    """An attribute column beside one index (coltt_hnsw_attr_create): one int64 (ATTR_I64) or float64 (ATTR_F64) per slot and a set bitmap, on
    the index's device.  Predicates over it are (column, op, operand) tuples for Hnsw.FilterEvalAttr."""

    def __init__(self, index, type_):
        h = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_attr_create(index.h, C.c_int(int(type_)), C.byref(h)))
        self.h, self.type, self.dtype = h, int(type_), _ATTR_DTYPE[int(type_)]

    def set(self, ids, values):
        """coltt_hnsw_attr_set: ids -> values (the last value of a repeated id; unknown and removed ids are ignored).  Returns the vertices set."""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
        v = np.ascontiguousarray(np.asarray(values, dtype=self.dtype).reshape(-1))
        if a.size != v.size:
            raise ValueError(f"HnswAttrColumn.set: {a.size} ids, {v.size} values")
        n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_attr_set(self.h, L.vp(a), L.vp(v), C.c_size_t(a.size), C.byref(n)))
        return n.value

    def get(self, ids):
        """coltt_hnsw_attr_get: (values in the column's dtype, bool flags: the id's vertex holds a value)"""
        a = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
        v = np.zeros(a.size, self.dtype); f = np.zeros(a.size, np.uint8)
        L.check(L.lib().coltt_hnsw_attr_get(self.h, L.vp(a), C.c_size_t(a.size), L.vp(v), L.vp(f)))
        return v, f.astype(bool)

    def info(self):
        ix = C.c_uint64(0); t = C.c_int32(0); s = C.c_uint64(0); n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_attr_info(self.h, C.byref(ix), C.byref(t), C.byref(s), C.byref(n)))
        return {"index": ix.value, "type": t.value, "slots": s.value, "set": n.value}

    def close(self):
        if getattr(self, "h", None) is not None:
            L.lib().coltt_hnsw_attr_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pred_array(preds):
    """(column, op, operand) tuples (or AttrPred structures) -> a coltt_attr_pred array; the column's type picks the member of the union"""
    arr = (AttrPred * max(len(preds), 1))()
    for i, p in enumerate(preds):
        if isinstance(p, AttrPred):
            arr[i] = p
            continue
        col, op, operand = p
        arr[i].column = 0 if col.h is None else col.h.value
        arr[i].op = int(op); arr[i].reserved = 0
        if col.type == ATTR_F64:
            arr[i].value.f64 = float(0.0 if operand is None else operand)
        else:
            arr[i].value.i64 = int(0 if operand is None else operand)
    return arr


class Hnsw:
    def __init__(self, dim, distance=L.COSINE, cfg=None, quantization=L.Q_NONE):
        self.dim, self.distance, self.quantization = int(dim), distance, quantization
        cfg = cfg or HnswCfg.default()
        h = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_create(C.c_uint32(dim), distance, quantization, C.byref(cfg), C.byref(h)))
        self.h = h
        self.cfg = HnswCfg()
        L.check(L.lib().coltt_hnsw_get_cfg(self.h, C.byref(self.cfg)))

    @classmethod
    def from_handle(cls, h, dim, distance, quantization):
        """wrap a handle owned by someone else (a group member): close() will not destroy it"""
        o = cls.__new__(cls)
        o.h, o.dim, o.distance, o.quantization, o._borrowed = h, int(dim), distance, quantization, True
        o.cfg = HnswCfg()
        o.Config()
        return o

    def close(self):
        if getattr(self, "_borrowed", False):
            self.h = None
        if getattr(self, "h", None) is not None:
            L.lib().coltt_hnsw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Len(self):
        n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_len(self.h, C.byref(n)))
        return n.value

    def Dim(self):
        return self.dim

    def Config(self):
        """Hnsw.Config() (hnsw.go:92-94): the live configuration, re-read from the library."""
        L.check(L.lib().coltt_hnsw_get_cfg(self.h, C.byref(self.cfg)))
        return self.cfg

    def Get(self, id_):
        """Hnsw.Get(id) / GetVertex(id) (hnsw.go:169-189): (stored vector, level) of a live vertex."""
        dt = {L.Q_NONE: np.float32, L.Q_F8: np.uint8}.get(self.quantization, np.uint16)
        o = np.empty(self.dim, dt); lv = C.c_int32(0)
        L.check(L.lib().coltt_hnsw_get(self.h, C.c_uint64(int(id_)), L.vp(o), C.byref(lv)))
        return o, lv.value

    def RandomLevel(self, u):
        """Hnsw.RandomLevel() (hnsw.go:280-282) for a uniform draw u in (0,1) supplied by the caller."""
        lv = C.c_int32(0)
        L.check(L.lib().coltt_hnsw_random_level(self.h, C.c_float(u), C.byref(lv)))
        return lv.value

    # -- Hnsw.Load-shaped bulk import (graph dict in the oracle's export layout; raw vectors in slot order)
    def BulkLoad(self, g, raw_vectors):
        v = np.ascontiguousarray(raw_vectors, np.float32)
        ids = np.ascontiguousarray(g["ids"], np.uint64) if g.get("ids") is not None else None
        lv = np.ascontiguousarray(g["levels"], np.int32)
        dl = np.ascontiguousarray(g["deleted"], np.uint8) if g.get("deleted") is not None else None
        off = np.ascontiguousarray(g["row_offsets"], np.int64)
        nb = np.ascontiguousarray(g["nbr"], np.int32)
        nd = np.ascontiguousarray(g["nbr_dist"], np.float32) if g.get("nbr_dist") is not None else None
        L.check(L.lib().coltt_hnsw_bulk_load(self.h, C.c_uint64(len(lv)), L.vp(ids), L.vp(lv), L.vp(dl), L.vp(v), L.vp(off),
                                             L.vp(nb), L.vp(nd), C.c_int32(int(g["entry"]))))

    # -- Hnsw.Insert (hnsw.go:104-167)
    def Insert(self, id_, vector, level):
        v = np.ascontiguousarray(vector, np.float32).reshape(-1)
        L.check(L.lib().coltt_hnsw_insert(self.h, C.c_uint64(int(id_)), L.vp(v), C.c_int32(int(level))))

    def InsertBatchDevice(self, d_vecs, n, levels, batch, first_id=0, ids=None):
        lv = np.ascontiguousarray(levels, np.int32)
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.uint64)
        L.check(L.lib().coltt_hnsw_insert_batch_device(self.h, L.vp(ids), C.c_uint64(first_id), C.c_void_p(d_vecs), L.vp(lv),
                                                       C.c_size_t(n), C.c_uint32(batch)))

    # -- Hnsw.Remove (hnsw.go:191-241)
    def Remove(self, id_):
        L.check(L.lib().coltt_hnsw_remove(self.h, C.c_uint64(int(id_))))

    # -- reclaim the slots Remove left behind (an extension the reference does not have)
    def Compact(self, stage_bytes=0, with_map=False):
        """coltt_hnsw_compact: drop the tombstoned slots in place on the device — vertex s moves to slot new(s) = live slots below s, no answer of
        any search changes, filters built before are stale.  stage_bytes: the staging block (0 = 64 MiB).  Returns the stats dict, with
        with_map=True also new_of_old [slots before] (0xffffffff for a dropped slot)."""
        ns = C.c_uint64(0)
        m = None
        if with_map:
            L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), None, None, None, None, None, None))
            m = np.empty(ns.value, np.uint32)
        st = HnswCompactStats()
        L.check(L.lib().coltt_hnsw_compact(self.h, C.c_uint64(int(stage_bytes)), L.vp(m), C.c_uint64(ns.value), C.byref(st)))
        d = {k: getattr(st, k) for k, _ in HnswCompactStats._fields_}
        if with_map:
            return d, m[:d["slots_before"]]
        return d

    def CompactCarry(self, filters=(), columns=(), stage_bytes=0, with_map=False):
        """coltt_hnsw_compact_carry: Compact, after which the listed HnswFilter / HnswAttrColumn objects are valid at the new generation under the same
        handles — a filter allows what it allowed among the live vertices, a column holds at every live vertex what it held; objects that are not
        listed go stale.  Returns (stats, carry stats, allowed [len(filters)], set [len(columns)]), with with_map=True also new_of_old.  The
        `.allowed` of the listed filter objects is refreshed."""
        filters, columns = list(filters), list(columns)
        fh = np.array([0 if f.h is None else f.h.value for f in filters], np.uint64)
        ch = np.array([0 if c.h is None else c.h.value for c in columns], np.uint64)
        al = np.zeros(max(len(filters), 1), np.uint64); ns_ = np.zeros(max(len(columns), 1), np.uint64)
        ns = C.c_uint64(0)
        m = None
        if with_map:
            L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), None, None, None, None, None, None))
            m = np.empty(ns.value, np.uint32)
        st = HnswCompactStats(); cs = HnswCarryStats()
        L.check(L.lib().coltt_hnsw_compact_carry(self.h, C.c_uint64(int(stage_bytes)), L.vp(fh) if fh.size else None, C.c_size_t(fh.size), L.vp(al),
                                                 L.vp(ch) if ch.size else None, C.c_size_t(ch.size), L.vp(ns_), L.vp(m), C.c_uint64(ns.value),
                                                 C.byref(st), C.byref(cs)))
        d = {k: getattr(st, k) for k, _ in HnswCompactStats._fields_}
        c = {k: getattr(cs, k) for k, _ in HnswCarryStats._fields_}
        al = al[:len(filters)]; ns_ = ns_[:len(columns)]
        for f, a in zip(filters, al):
            f.allowed = int(a)
        if with_map:
            return d, c, al, ns_, m[:d["slots_before"]]
        return d, c, al, ns_

    # -- Hnsw.Search (hnsw.go:243-278) for a batch of queries
    def Search(self, queries, k, ef=0, with_stats=False):
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32)
        st = HnswStats()
        L.check(L.lib().coltt_hnsw_search(self.h, L.vp(q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), L.vp(ids), L.vp(sc),
                                          L.vp(cnt), C.byref(st)))
        if with_stats:
            return ids, sc, cnt, {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_visit_resets": st.n_visit_resets}
        return ids, sc, cnt

    # -- filtered search (an extension the reference does not have): the k nearest among the ids of `flt`
    def Filter(self, ids):
        return HnswFilter(self, ids)

    def FilterEval(self, prog, leaves):
        """coltt_hnsw_filter_eval: the filter of a postfix programme (a list of leaf indices / FOP_*; a nested tuple goes through
        filter_postfix) over resident filters `leaves`, evaluated on the device.  An ordinary HnswFilter."""
        p = _prog_array(prog)
        lh = np.array([0 if f.h is None else f.h.value for f in leaves], np.uint64)
        h = C.c_uint64(0); n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_filter_eval(self.h, L.vp(p), C.c_size_t(p.size), L.vp(lh) if lh.size else None, C.c_size_t(lh.size),
                                               C.byref(n), C.byref(h)))
        return HnswFilter._from_handle(h.value, n.value)

    def FilterEvalBatch(self, progs, leaves):
        """coltt_hnsw_filter_eval_batch: one filter per programme over the shared leaf table, under one index state, in two kernel
        launches whatever len(progs) is.  Returns a list of HnswFilter."""
        ps = [_prog_array(p) for p in progs]
        off = np.zeros(len(ps) + 1, np.uint64)
        if ps:
            off[1:] = np.cumsum([p.size for p in ps])
        flat = np.ascontiguousarray(np.concatenate(ps)) if ps else np.zeros(0, np.int32)
        lh = np.array([0 if f.h is None else f.h.value for f in leaves], np.uint64)
        out = np.zeros(max(len(ps), 1), np.uint64); al = np.zeros(max(len(ps), 1), np.uint64)
        L.check(L.lib().coltt_hnsw_filter_eval_batch(self.h, L.vp(flat), L.vp(off), C.c_size_t(len(ps)), L.vp(lh) if lh.size else None,
                                                     C.c_size_t(lh.size), L.vp(al), L.vp(out)))
        return [HnswFilter._from_handle(out[i], al[i]) for i in range(len(ps))]

    # -- attribute columns: comparison predicates as programme leaves (include/coltt_gpu.h, "Attribute columns and predicates")
    def AttrColumn(self, type_):
        return HnswAttrColumn(self, type_)

    def FilterEvalAttr(self, prog, leaves, preds):
        """coltt_hnsw_filter_eval_attr: a programme over resident filters `leaves` and predicates `preds` ((column, op, operand) tuples): a value
        v >= 0 pushes leaves[v] when v < len(leaves), predicate v - len(leaves) otherwise.  An ordinary HnswFilter."""
        p = _prog_array(prog)
        lh = np.array([0 if f.h is None else f.h.value for f in leaves], np.uint64)
        pa = _pred_array(preds)
        h = C.c_uint64(0); n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_filter_eval_attr(self.h, L.vp(p), C.c_size_t(p.size), L.vp(lh) if lh.size else None, C.c_size_t(lh.size),
                                                    C.byref(pa) if len(preds) else None, C.c_size_t(len(preds)), C.byref(n), C.byref(h)))
        return HnswFilter._from_handle(h.value, n.value)

    def FilterEvalAttrBatch(self, progs, leaves, preds):
        """coltt_hnsw_filter_eval_attr_batch: one filter per programme over the shared leaf and predicate tables, under one index state, in
        two kernel launches.  Returns a list of HnswFilter."""
        ps = [_prog_array(p) for p in progs]
        off = np.zeros(len(ps) + 1, np.uint64)
        if ps:
            off[1:] = np.cumsum([p.size for p in ps])
        flat = np.ascontiguousarray(np.concatenate(ps)) if ps else np.zeros(0, np.int32)
        lh = np.array([0 if f.h is None else f.h.value for f in leaves], np.uint64)
        pa = _pred_array(preds)
        out = np.zeros(max(len(ps), 1), np.uint64); al = np.zeros(max(len(ps), 1), np.uint64)
        L.check(L.lib().coltt_hnsw_filter_eval_attr_batch(self.h, L.vp(flat), L.vp(off), C.c_size_t(len(ps)), L.vp(lh) if lh.size else None,
                                                          C.c_size_t(lh.size), C.byref(pa) if len(preds) else None, C.c_size_t(len(preds)),
                                                          L.vp(al), L.vp(out)))
        return [HnswFilter._from_handle(out[i], al[i]) for i in range(len(ps))]

    def SearchFiltered(self, queries, k, flt, ef=0, mode=FILTER_AUTO, with_stats=False):
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32)
        st = HnswFilterStats()
        L.check(L.lib().coltt_hnsw_search_filtered(self.h, flt.h, L.vp(q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_int(int(mode)),
                                                   L.vp(ids), L.vp(sc), L.vp(cnt), C.byref(st)))
        if with_stats:
            return ids, sc, cnt, {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_visit_resets": st.n_visit_resets,
                                  "ef_walk": st.ef_walk, "path": st.path, "n_exact_rows": st.n_exact_rows}
        return ids, sc, cnt

    def SearchFilteredBatch(self, queries, k, filters, ef=0, mode=FILTER_AUTO, with_stats=False):
        """a filter per query (coltt_hnsw_search_filtered_batch): row i == SearchFiltered(queries[i], k, filters[i], ef, mode).
        `filters`: one HnswFilter per query row (repeats allowed).  Returns ids, scores, counts, paths (+ stats)."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        if len(filters) != nq:
            raise ValueError(f"SearchFilteredBatch: {len(filters)} filters for {nq} queries")
        fh = np.array([0 if f.h is None else f.h.value for f in filters], np.uint64)
        ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32)
        paths = np.zeros(nq, np.int32)
        st = HnswFilterStats()
        L.check(L.lib().coltt_hnsw_search_filtered_batch(self.h, L.vp(fh), L.vp(q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef),
                                                         C.c_int(int(mode)), L.vp(ids), L.vp(sc), L.vp(cnt), L.vp(paths), C.byref(st)))
        if with_stats:
            return ids, sc, cnt, paths, {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_visit_resets": st.n_visit_resets,
                                         "ef_walk": st.ef_walk, "path": st.path, "n_exact_rows": st.n_exact_rows}
        return ids, sc, cnt, paths

    def SearchDevice(self, d_q, nq, k, d_ids, d_scores, d_counts, ef=0):
        st = HnswStats()
        L.check(L.lib().coltt_hnsw_search_device(self.h, C.c_void_p(d_q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef),
                                                 C.c_void_p(d_ids), C.c_void_p(d_scores), C.c_void_p(d_counts), C.byref(st)))
        return {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_visit_resets": st.n_visit_resets}

    def Export(self):
        ns, nr, ne, ent = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        L.check(L.lib().coltt_hnsw_export(self.h, C.byref(ns), C.byref(nr), C.byref(ne), None, None, None, None, None, None, C.byref(ent)))
        ids = np.empty(ns.value, np.uint64); lv = np.empty(ns.value, np.int32); dl = np.empty(ns.value, np.uint8)
        off = np.empty(nr.value + 1, np.int64); nb = np.empty(ne.value, np.int32); nd = np.empty(ne.value, np.float32)
        L.check(L.lib().coltt_hnsw_export(self.h, C.byref(ns), C.byref(nr), C.byref(ne), L.vp(ids), L.vp(lv), L.vp(dl), L.vp(off),
                                          L.vp(nb), L.vp(nd), C.byref(ent)))
        return {"ids": ids, "levels": lv, "deleted": dl, "row_offsets": off, "nbr": nb, "nbr_dist": nd, "entry": ent.value}

    # -- Hnsw.Commit / Hnsw.Load (core/vectorindex/hnsw_commit.go:69-278)
    def Commit(self, header=True):
        n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_commit(self.h, int(header), None, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(n)))
        buf = np.empty(n.value, np.uint8)
        L.check(L.lib().coltt_hnsw_commit(self.h, int(header), None, None, C.c_uint64(0), L.vp(buf), C.c_uint64(n.value), C.byref(n)))
        return buf.tobytes()

    def Load(self, data, header=True):
        b = np.frombuffer(data, np.uint8)
        n = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_load(self.h, int(header), L.vp(b), C.c_uint64(len(b)), C.byref(n), None, None, None, C.c_uint64(0)))
        L.check(L.lib().coltt_hnsw_get_cfg(self.h, C.byref(self.cfg)))
        return n.value

    def ExportRaw(self):
        """adjacency in the HBM layout: adj0 [n, mMax0], upper_off [n], adjU [n_upper, mMax] (0xffffffff padded)."""
        ns, nu, ent, el = C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), C.byref(nu), C.byref(ent), C.byref(el), None, None, None))
        adj0 = np.empty((ns.value, self.cfg.m_max0), np.uint32); uo = np.empty(ns.value, np.uint32)
        adjU = np.empty((max(nu.value, 1), self.cfg.m_max), np.uint32)
        L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), C.byref(nu), C.byref(ent), C.byref(el), L.vp(adj0), L.vp(uo), L.vp(adjU)))
        return {"adj0": adj0, "upper_off": uo, "adjU": adjU, "entry": ent.value, "entry_level": el.value, "n": ns.value}

    def FetchRows(self, first=0, n=None, out=None):
        ns = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), None, None, None, None, None, None))
        n = ns.value - first if n is None else n
        dt = {L.Q_NONE: np.float32, L.Q_F8: np.uint8}.get(self.quantization, np.uint16)
        if out is None:
            out = np.empty((n, self.dim), dt)
        L.check(L.lib().coltt_hnsw_fetch_rows(self.h, C.c_uint64(first), C.c_uint64(n), L.vp(out)))
        return out

    def Reserve(self, n_slots, n_upper_rows=0):
        L.check(L.lib().coltt_hnsw_reserve(self.h, C.c_uint64(int(n_slots)), C.c_uint64(int(n_upper_rows))))

    def Rows8(self):
        """(search launches served by the eight-lanes-per-row core, whether the line-transposed row copy is complete)"""
        a, f = C.c_uint64(0), C.c_int32(0)
        L.check(L.lib().coltt_hnsw_rows8_searches(self.h, C.byref(a), C.byref(f)))
        return a.value, bool(f.value)

    def RowFilterStats(self):
        """the level-0 row filter (coltt_hnsw_row_filter_stats): cumulative evaluations it rejected, f32 rows and shadow rows the filtered
        launches read at level 0, filtered launches, whether the index keeps a shadow of its rows and of which kinds (8 / 16 bits); upper_*: the same
        counters of the filtered descent (levels above 0; COLTT_ROW_FILTER_UPPER) and the launches that ran it (coltt_hnsw_row_filter_stats_ex)"""
        r, e, s, n, f = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        L.check(L.lib().coltt_hnsw_row_filter_stats(self.h, C.byref(r), C.byref(e), C.byref(s), C.byref(n), C.byref(f)))
        us, ur, uf, un = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_row_filter_stats_ex(self.h, C.byref(us), C.byref(ur), C.byref(uf), C.byref(un)))
        return {"rejected": r.value, "f32_rows": e.value, "shadow_rows": s.value, "launches": n.value, "shadow": bool(f.value),
                "shadow_bits": tuple(b for b in (8, 16) if f.value & b),
                "upper_shadow_rows": us.value, "upper_rejected": ur.value, "upper_f32_rows": uf.value, "upper_launches": un.value}

    def VisitedStats(self):
        """the visited set of the last search launch (coltt_hnsw_visited_stats): its kind (0 HBM byte map, 32 LDS table of 32-bit slots, 16 the 16-bit LDS
        table), the traversals that launch kept resident per CU and its grid, launches on the 16-bit table so far, and — if that last launch ran on the
        16-bit table — the fullest stash and the most vertices one of its traversals visited"""
        k, w, g = C.c_int32(0), C.c_uint32(0), C.c_uint32(0)
        n, s, v = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_visited_stats(self.h, C.byref(k), C.byref(w), C.byref(g), C.byref(n), C.byref(s), C.byref(v)))
        return {"kind": k.value, "waves_per_cu": w.value, "grid": g.value, "launches16": n.value, "stash_max": s.value, "visited_max": v.value}

    def PlanFacts(self):
        """what the search plan reads of this index as it is now (coltt_hnsw_search_plan_facts).  vis_ready: the HBM visited workspace exists — the first
        search that wants it (ef > 128 by default) makes it"""
        f = PlanFactsC()
        L.check(L.lib().coltt_hnsw_search_plan_facts(self.h, C.byref(f)))
        return f

    def SearchPlan(self, nq, k, ef=0, force=0):
        """which kernel Search(queries[nq], k, ef) launches on this index as it is now, and how (search_plan_host over PlanFacts())"""
        return search_plan_host(self.PlanFacts(), nq, k, ef or self.cfg.ef, force)

    def FetchShadow8(self, first=0, n=None):
        """the 8-bit shadow of slots [first, first + n) (coltt_hnsw_fetch_shadow8): codes [n, dim] int8 in natural element order, (scale, error norm)
        [n, 2], and the pairs riding with the level-0 adjacency rows [n, m_max0, 2]"""
        ns = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), None, None, None, None, None, None))
        n = ns.value - first if n is None else n
        codes = np.empty((n, self.dim), np.int8); meta = np.empty((n, 2), np.float32); adj = np.empty((n, self.cfg.m_max0, 2), np.float32)
        L.check(L.lib().coltt_hnsw_fetch_shadow8(self.h, C.c_uint64(first), C.c_uint64(n), L.vp(codes), L.vp(meta), L.vp(adj)))
        return codes, meta, adj

    def RowFilterProbe(self, queries, slots, lower_bound, bits=8, nt=0, full_at_pop=1, sums=False):
        """the level-0 walk's chunk evaluation on chosen pairs (coltt_hnsw_row_filter_probe): slots [nq, 32] uint32 (L.NBR_NONE = not fresh),
        lower_bound a scalar or [nq].  bits: 8, 16 or "8i" (the 8-bit shadow against the quantised query, row_filter8i.hpp).
        Returns (r [nq, 32], qnorm [nq], rnorm [nq, 32], counts [nq, 3] = rejected, f32 rows, shadow rows); with sums=True ("8i" only) also
        (isum [nq, 32] int64: the integer sums phase A formed, qte [nq, 2]: the queries' (scale, error norm))."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        s = np.ascontiguousarray(slots, np.uint32).reshape(nq, 32)
        lb = np.ascontiguousarray(np.broadcast_to(np.asarray(lower_bound, np.float32), (nq,)))
        r = np.zeros((nq, 32), np.float32); qn = np.zeros(nq, np.float32); rn = np.zeros((nq, 32), np.float32); cnt = np.zeros((nq, 3), np.uint32)
        if bits in ("8i", 80):
            isum = np.zeros((nq, 32), np.int64); qte = np.zeros((nq, 2), np.float32)
            L.check(L.lib().coltt_hnsw_row_filter_probe_ex(self.h, L.vp(q), C.c_size_t(nq), L.vp(s), L.vp(lb), C.c_int(80), C.c_int(int(nt)),
                                                           C.c_int(int(full_at_pop)), L.vp(r), L.vp(qn), L.vp(rn), L.vp(cnt), L.vp(isum), L.vp(qte)))
            return (r, qn, rn, cnt, isum, qte) if sums else (r, qn, rn, cnt)
        if sums:
            raise ValueError("RowFilterProbe: only the \"8i\" kind forms integer sums")
        L.check(L.lib().coltt_hnsw_row_filter_probe(self.h, L.vp(q), C.c_size_t(nq), L.vp(s), L.vp(lb), C.c_int(int(bits)), C.c_int(int(nt)),
                                                    C.c_int(int(full_at_pop)), L.vp(r), L.vp(qn), L.vp(rn), L.vp(cnt)))
        return r, qn, rn, cnt

    # -- product-quantised search (coltt_hnsw_pq_*; the reference's call shape: playground/hnswpq_verification.go:69-105)
    def PqAttach(self, pq):
        """snapshot the trained quantiser `pq` (a PQSpace) into the index and encode every stored row"""
        L.check(L.lib().coltt_hnsw_pq_attach(self.h, pq.h))

    def PqInfo(self):
        m, c, mt, n = C.c_uint32(0), C.c_uint32(0), C.c_int32(0), C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_pq_info(self.h, C.byref(m), C.byref(c), C.byref(mt), C.byref(n)))
        return {"m": m.value, "C": c.value, "metric": mt.value, "coded": n.value}

    def PqCodes(self, first=0, n=None):
        info = self.PqInfo()
        n = info["coded"] - first if n is None else n
        out = np.empty((n, info["m"]), np.uint8)
        L.check(L.lib().coltt_hnsw_pq_fetch_codes(self.h, C.c_uint64(first), C.c_uint64(n), L.vp(out)))
        return out

    def PqNbrStats(self):
        """the neighbourhood blocks of the product-quantised walk (coltt_hnsw_pq_nbr_stats): whole builds, mutating calls that patched, blocks they
        rewrote, state 0 = none (never built / off / not affordable) / 1 = current / 2 = stale"""
        b, p, r, s = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        L.check(L.lib().coltt_hnsw_pq_nbr_stats(self.h, C.byref(b), C.byref(p), C.byref(r), C.byref(s)))
        return {"builds": b.value, "patches": p.value, "patched_rows": r.value, "state": s.value}

    def PqFetchNbr(self, first=0, n=None):
        """the blocks of slots [first, first + n) as the walk reads them (coltt_hnsw_pq_fetch_nbr): uint8 [n, m_max0, code row rounded up to 16];
        raises unless the blocks are current (state 1)"""
        ns = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_export_raw(self.h, C.byref(ns), None, None, None, None, None, None))
        n = ns.value - first if n is None else n
        out = np.empty((n, self.cfg.m_max0, (self.PqInfo()["m"] + 15) & ~15), np.uint8)
        L.check(L.lib().coltt_hnsw_pq_fetch_nbr(self.h, C.c_uint64(first), C.c_uint64(n), L.vp(out)))
        return out

    def PqSearch(self, queries, k, ef=0, rerank=0, with_stats=False):
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32)
        st = HnswStats(); nx = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_pq_search(self.h, L.vp(q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_uint32(rerank), L.vp(ids), L.vp(sc),
                                             L.vp(cnt), C.byref(st), C.byref(nx)))
        if with_stats:
            return ids, sc, cnt, {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_exact": nx.value}
        return ids, sc, cnt

    def PqSearchFiltered(self, queries, k, flt, ef=0, rerank=0, mode=FILTER_AUTO, with_stats=False):
        """the k nearest among the ids of `flt` over the walk on the quantiser's codes (coltt_hnsw_pq_search_filtered); returns as SearchFiltered"""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32)
        st = HnswFilterStats()
        L.check(L.lib().coltt_hnsw_pq_search_filtered(self.h, flt.h, L.vp(q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_uint32(rerank),
                                                      C.c_int(int(mode)), L.vp(ids), L.vp(sc), L.vp(cnt), C.byref(st)))
        if with_stats:
            return ids, sc, cnt, {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_visit_resets": st.n_visit_resets,
                                  "ef_walk": st.ef_walk, "path": st.path, "n_exact_rows": st.n_exact_rows}
        return ids, sc, cnt

    def PqSearchFilteredBatch(self, queries, k, filters, ef=0, rerank=0, mode=FILTER_AUTO, with_stats=False):
        """a filter per query over the walk on the quantiser's codes (coltt_hnsw_pq_search_filtered_batch): row i ==
        PqSearchFiltered(queries[i], k, filters[i], ef, rerank, mode).  `filters`: one HnswFilter per query row (repeats allowed).
        Returns as SearchFilteredBatch: ids, scores, counts, paths (+ stats)."""
        q = np.ascontiguousarray(queries, np.float32).reshape(-1, self.dim)
        nq = q.shape[0]
        if len(filters) != nq:
            raise ValueError(f"PqSearchFilteredBatch: {len(filters)} filters for {nq} queries")
        fh = np.array([0 if f.h is None else f.h.value for f in filters], np.uint64)
        ids = np.zeros((nq, k), np.uint64); sc = np.zeros((nq, k), np.float32); cnt = np.zeros(nq, np.uint32)
        paths = np.zeros(nq, np.int32)
        st = HnswFilterStats()
        L.check(L.lib().coltt_hnsw_pq_search_filtered_batch(self.h, L.vp(fh), L.vp(q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_uint32(rerank),
                                                            C.c_int(int(mode)), L.vp(ids), L.vp(sc), L.vp(cnt), L.vp(paths), C.byref(st)))
        if with_stats:
            return ids, sc, cnt, paths, {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_visit_resets": st.n_visit_resets,
                                         "ef_walk": st.ef_walk, "path": st.path, "n_exact_rows": st.n_exact_rows}
        return ids, sc, cnt, paths

    def PqSearchDevice(self, d_q, nq, k, d_ids, d_scores, d_counts, ef=0, rerank=0):
        st = HnswStats(); nx = C.c_uint64(0)
        L.check(L.lib().coltt_hnsw_pq_search_device(self.h, C.c_void_p(d_q), C.c_size_t(nq), C.c_uint32(k), C.c_uint32(ef), C.c_uint32(rerank),
                                                    C.c_void_p(d_ids), C.c_void_p(d_scores), C.c_void_p(d_counts), C.byref(st), C.byref(nx)))
        return {"n_dist": st.n_dist, "n_exp": st.n_exp, "n_hops": st.n_hops, "n_exact": nx.value}

    def last_kernel_ms(self):
        ms = C.c_float(0)
        L.check(L.lib().coltt_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value
