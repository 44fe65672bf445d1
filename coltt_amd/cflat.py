"""MultiVectorSpace — GPU-backed stand-in for experimental.multiVectorVertex (experimental/multi_vector_vertex.go)."""
import ctypes as C

import numpy as np

from . import _lib as L

K_MAX = 2048   # largest topK the selection serves (csrc/select.hpp)


class MultiVectorSpace:
    def __init__(self, dim, n_fields, distance=L.COSINE):
        self.dim, self.nf = int(dim), int(n_fields)
        h = C.c_uint64(0)
        L.check(L.lib().coltt_cflat_create(C.c_uint32(dim), distance, C.c_uint32(n_fields), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) is not None:
            L.lib().coltt_cflat_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ChangedVertex (multi_vector_vertex.go:60-75)
    def ChangedVertex(self, ids, multi_vectors):
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        v = np.ascontiguousarray(multi_vectors, np.float32)
        if v.size != len(ids) * self.nf * self.dim:   # the library reads len(ids) x n_fields x dim floats, whatever it is handed
            raise ValueError(f"expect {len(ids)} x {self.nf} vectors of dimension [{self.dim}] ({len(ids) * self.nf * self.dim} values), but got {v.size}")
        v = v.reshape(len(ids), self.nf, self.dim)
        L.check(L.lib().coltt_cflat_upsert(self.h, L.vp(ids), L.vp(v), C.c_size_t(len(ids))))

    def RemoveVertex(self, ids):
        ids = np.ascontiguousarray(ids, np.uint64).reshape(-1)
        L.check(L.lib().coltt_cflat_remove(self.h, L.vp(ids), C.c_size_t(len(ids))))

    def Len(self):
        n = C.c_uint64(0); L.check(L.lib().coltt_cflat_len(self.h, C.byref(n))); return n.value

    def GetVertex(self, id_):
        """the stored (for cosine: normalised) fields of one vertex, [n_fields][dim] f32; ColttError for an unknown id"""
        o = np.zeros((self.nf, self.dim), np.float32)
        L.check(L.lib().coltt_cflat_get(self.h, C.c_uint64(int(id_)), L.vp(o)))
        return o

    # MultiVertexSearch (multi_vector_vertex.go:85-137)
    def MultiVertexSearch(self, topK, multi_vectors, ratios, include=None):
        q = np.ascontiguousarray(multi_vectors, np.float32).reshape(-1, self.nf, self.dim)
        r = np.ascontiguousarray(ratios, np.uint32); inc = np.ones(self.nf, np.uint8) if include is None else np.ascontiguousarray(include, np.uint8)
        if r.size != self.nf or inc.size != self.nf:   # the library reads n_fields entries of each
            raise ValueError(f"expect one ratio and one include flag per field ({self.nf}), but got {r.size} and {inc.size}")
        nq = q.shape[0]
        ids = np.zeros((nq, topK), np.uint64); sc = np.zeros((nq, topK), np.float32); cnt = np.zeros(nq, np.uint32)
        L.check(L.lib().coltt_cflat_search(self.h, L.vp(q), L.vp(r), L.vp(inc), C.c_size_t(nq), C.c_uint32(topK), L.vp(ids), L.vp(sc), L.vp(cnt)))
        return ids, sc, cnt

    def MultiVertexSearchBatch(self, topK, multi_vectors, ratios, include=None):
        """nq independent MultiVertexSearch requests in one call: ratios / include are [nq][n_fields] (include=None: every field of
        every request).  Row i equals MultiVertexSearch(topK, multi_vectors[i], ratios[i], include[i]): same count, ids, order, score bits."""
        q = np.ascontiguousarray(multi_vectors, np.float32).reshape(-1, self.nf, self.dim)
        nq = q.shape[0]
        r = np.ascontiguousarray(ratios, np.uint32); inc = np.ones((nq, self.nf), np.uint8) if include is None else np.ascontiguousarray(include, np.uint8)
        want = (nq, self.nf)
        if r.shape != want or inc.shape != want:   # the library reads nq x n_fields entries of each
            raise ValueError(f"expect one ratio and one include flag per request and field {want}, but got {r.shape} and {inc.shape}")
        ids = np.zeros((nq, topK), np.uint64); sc = np.zeros((nq, topK), np.float32); cnt = np.zeros(nq, np.uint32)
        L.check(L.lib().coltt_cflat_search_batch(self.h, L.vp(q), L.vp(r), L.vp(inc), C.c_size_t(nq), C.c_uint32(topK), L.vp(ids), L.vp(sc), L.vp(cnt)))
        return ids, sc, cnt
