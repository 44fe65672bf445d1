"""cflat_ref.py — SECOND, INDEPENDENT restatement of the experimental multi-vector weighted scan, in pure Python.  TEST INFRASTRUCTURE ONLY.

Written from the Go text (not from oracle/coltt_oracle.cpp and not from coltt_amd/csrc/cflat.hip), on top of oracle/pyref.py's normalize /
cosine / euclidean, so that a misreading in one restatement shows up as a disagreement between the two: tests/test_cflat_ref.py asserts
C++ oracle == this file, and tests/golden/cflat.npz (made by tests/golden/make_golden_cflat.py FROM THIS FILE ALONE) pins both and the GPU.

Followed line by line:
  experimental/multi_vector_vertex.go   ChangedVertex :61-75 (every field of a stored vertex is Normalize'd for cosine), RemoveVertex :77-83,
                                        MultiVertexSearch :85-137 (only INCLUDED query fields are Normalize'd :96-100; score := float32(0);
                                        score += scoreHelper(Distance(node[f], q[f])) * (float32(Ratio) / 100) over included fields, in
                                        the order of the request's field list :112-118)
  experimental/experimental_helper.go   scoreHelper :134-139: cosine ((2 - d) / 2) * 100 in f32; otherwise float32(math.Max(0, float64(100 - d)))
  experimental/constants.go             Normalize :48-64 (the same text as core/vectorindex/metadata.go:107-123 == pyref.normalize)
  experimental/multi_priority_queue.go  Add :54-63 (min-heap, pop-min when over capacity: keeps the K LARGEST scores), ToSlice :65-77
                                        (sort.Slice by Score DESCENDING)

Two things the Go text leaves open, and what is done here:
  * TIES.  The per-shard maps are walked in Go's random order, the heap breaks ties by arrival and sort.Slice is unstable: among equal
    scores neither WHICH vertices survive nor their order is specified.  This file returns the project's canonical order — the K largest
    (score, id) pairs, descending by score and, among equal scores, descending by id — as coltt_oracle.cpp and the GPU do.  It is a
    convention of this project, not reference behaviour.
  * `score += a * b` is evaluated as two f32 roundings (multiply, then add), which is what the Go compiler emits on amd64; the language
    would also allow a fused multiply-add.

Vertex ids are the uint64 the stores use (the reference's are strings); the field list of a request is fields 0 .. nf-1 in order."""
import numpy as np

from oracle import pyref as P

f32 = np.float32
COSINE, L2 = 0, 1


def score_helper(d, metric):
    """experimental_helper.go:134-139"""
    d = f32(d)
    if metric == COSINE:
        return f32(f32(f32(f32(2) - d) / f32(2)) * f32(100))
    x = float(f32(f32(100) - d))                 # float64(100 - score): the subtraction is f32
    if x != x:
        return f32(np.nan)                       # math.Max propagates NaN
    return f32(x if x > 0.0 else 0.0)            # math.Max(0, x); Max(0, -0) = +0


def weight(ratio):
    """float32(vectors.Ratio) / 100 — Ratio is a uint32, the constant converts to float32"""
    return f32(f32(int(ratio)) / f32(100))


def _key(score):
    """total order of f32 by value with -0 < +0 (the stores' score key)"""
    u = int(f32(score).view(np.uint32))
    return (~u & 0xFFFFFFFF) if (u & 0x80000000) else (u | 0x80000000)


class CFlatRef:
    def __init__(self, dim, n_fields, metric=COSINE):
        self.dim, self.nf, self.metric = int(dim), int(n_fields), int(metric)
        self.v = {}                              # id -> [nf] f32 vectors as stored

    def __len__(self):
        return len(self.v)

    # ChangedVertex :61-75 — one vertex per call; a later one of the same id replaces the earlier
    def upsert(self, ids, vecs):
        vecs = np.asarray(vecs, f32).reshape(len(ids), self.nf, self.dim)
        for i, id_ in enumerate(ids):
            fields = []
            for f in range(self.nf):
                vec = vecs[i, f].copy()
                if self.metric == COSINE:
                    vec = P.normalize(vec)
                fields.append(vec)
            self.v[int(id_)] = fields

    # RemoveVertex :77-83 — delete() of an absent key is a no-op
    def remove(self, ids):
        for id_ in ids:
            self.v.pop(int(id_), None)

    def distance(self, a, b):
        return P.cosine(a, b) if self.metric == COSINE else P.euclidean(a, b)

    def scores(self, q, ratios, include):
        """MultiVertexSearch :85-118: {id: score} of every stored vertex"""
        q = np.asarray(q, f32).reshape(self.nf, self.dim)
        qv = []
        for f in range(self.nf):
            vec = q[f].copy()
            if include[f] and self.metric == COSINE:
                vec = P.normalize(vec)
            qv.append(vec)
        out = {}
        for id_, node in self.v.items():
            score = f32(0)
            for f in range(self.nf):
                if include[f]:
                    sim = self.distance(node[f], qv[f])
                    score = f32(score + f32(score_helper(sim, self.metric) * weight(ratios[f])))
            out[id_] = score
        return out

    def rank(self, q, ratios, include):
        """every vertex, descending by (score, id): search(k) is its first k entries (the queue keeps the K largest, ToSlice sorts descending)"""
        sc = self.scores(q, ratios, include)
        order = sorted(sc.items(), key=lambda t: (_key(t[1]), t[0]), reverse=True)
        return np.array([t[0] for t in order], np.uint64), np.array([t[1] for t in order], np.float32)

    def search(self, q, ratios, include, k):
        ids, sc = self.rank(q, ratios, include)
        k = max(int(k), 0)
        return ids[:k], sc[:k]
