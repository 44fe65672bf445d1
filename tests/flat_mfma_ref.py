"""A float64 model of the candidate generation of the FLAT matrix-core search (coltt_amd/csrc/flat_mfma.hpp, flat.hip: search_group_mfma),
and the data sets that attack its margin.  No GPU.  Shared by tests/test_flat_mfma_margin_host.py and tests/test_gpu_flat_mfma_margin.py.

What the kernels do, and what is modelled:
  * flat_mfma3_kernel forms an approximate candidate value s~ per (row, query): cosine |1 - dot~ / sqrt(nq * nr)|, Euclidean
    nq + nr - 2 dot~ (a squared distance).  nq / nr are the f32 norms of the prepared query / the stored row; dot~ is taken over operands
    rounded to binary16: f32 rows and queries through a round-to-nearest cast (`astype(float16)`, denormals kept), 2-byte rows are their own
    codes (exact) and the query went through the same Lower.  The model takes dot~ EXACTLY (float64) over those operands: it leaves out the
    f32 accumulation order of the matrix cores, which the margins budget separately (D * 2^-24 * sum |a_i b_i|).
  * flat_pick_kernel keeps s~ <= s~_(k) + margin (nearest) or s~ >= s~_(k) - margin (farthest).  The margin is computed here as
    search_group_mfma / flat_pick_kernel compute it, from constants PARSED out of the sources: a drift fails the host test.
  * the survivors are re-scored exactly, so the answer is right iff the kept set holds every true top-k member: kept_superset()."""
import ctypes as C
import os
import re

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coltt_amd", "csrc")


# ------------------------------------------------------------------------------------------------ constants, parsed from the sources
def _const(text, name):
    m = re.search(r"constexpr\s+float\s+" + name + r"\s*=\s*([0-9.eE+-]+)f\s*;", text)
    assert m, f"constexpr float {name} not found"
    return np.float32(m.group(1))


def constants():
    """The margins of flat_mfma.hpp and the terms of flat.hip's l2_eps / l2_abs, as float32."""
    hpp = open(os.path.join(CSRC, "flat_mfma.hpp")).read()
    hip = open(os.path.join(CSRC, "flat.hip")).read()
    c = {"MF_MARGIN": _const(hpp, "MF_MARGIN"), "MF_MARGIN_F32": _const(hpp, "MF_MARGIN_F32"),
         "L2_ULP": _const(hip, "L2_ULP"), "L2_ACC_TERMS": _const(hip, "L2_ACC_TERMS"), "L2_ROUND_F16": _const(hip, "L2_ROUND_F16"),
         "L2_ABS_F16": _const(hip, "L2_ABS_F16")}
    # the functions really are built from those names, and from nothing else
    body = re.search(r"float l2_eps\(const Flat\* f\) \{(.*?)\n\}", hip, re.S).group(1)
    assert "L2_ULP" in body and "L2_ACC_TERMS" in body and "L2_ROUND_F16" in body and not re.search(r"\d\.\d*e-\d", body), body
    body = re.search(r"float l2_abs\(const Flat\* f\) \{(.*?)\n\}", hip, re.S).group(1)
    assert "L2_ABS_F16" in body and "sqrtf((float)f->dim)" in body and not re.search(r"\d\.\d*e-\d", body), body
    # flat_pick_kernel: the out-of-range clause and the shape of the Euclidean margin
    m = re.search(r"if \(qn_l2\) margin = qn_l2\[q\] <= ([0-9.e]+)f \? margin \* \(qn_l2\[q\] \+ max_row_norm\) \+ abs_l2 \* \(sqrtf\(qn_l2\[q\]\) \+ sqrtf\(max_row_norm\)\) : __builtin_inff\(\);", hpp)
    assert m, "flat_pick_kernel: the Euclidean margin is not the expression this model restates"
    c["QN_MAX"] = np.float32(m.group(1))
    # search_group_mfma: which margin goes with which store, and the factor 2
    assert "f->quant == COLTT_Q_NONE ? MF_MARGIN_F32 : MF_MARGIN, ovf)" in hip
    assert "2.0f * l2_eps(f), ovf, qn, f->max_norm(), 2.0f * l2_abs(f))" in hip
    return c


def margin(metric, quant, dim, qn, max_norm, consts=None):
    """The pick margin per query (float32 arithmetic, as on the device).  qn: [nq] f32 norms^2 of the prepared queries."""
    c = consts or constants()
    qn = np.asarray(qn, np.float32)
    if metric == O.COSINE:
        return np.full(qn.shape, c["MF_MARGIN_F32"] if quant == O.Q_NONE else c["MF_MARGIN"], np.float32)
    f = np.float32
    eps = c["L2_ACC_TERMS"] * (f(dim) * c["L2_ULP"]) + (c["L2_ROUND_F16"] if quant == O.Q_NONE else f(0))
    ab = c["L2_ABS_F16"] * np.sqrt(f(dim)) if quant == O.Q_NONE else f(0)
    mx = f(max_norm)
    with np.errstate(over="ignore", invalid="ignore"):
        m = (f(2) * eps) * (qn + mx) + (f(2) * ab) * (np.sqrt(qn) + np.sqrt(mx))
    return np.where(qn <= c["QN_MAX"], m, f(np.inf)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the store's view of rows and queries
def stored_rows(metric, quant, X):
    """What the store keeps for upserted rows X: Normalize (cosine) + Lower.  Returns (codes, values): the stored codes (f32 rows / u16
    codes) and their f32 values."""
    X = np.ascontiguousarray(X, np.float32)
    if metric == O.COSINE:
        X = O.normalize(X)
    return loaded_rows(quant, X)


def loaded_rows(quant, X):
    """Rows as a loaded stream leaves them: Lower only, no Normalize."""
    X = np.ascontiguousarray(X, np.float32)
    if quant == O.Q_NONE:
        return X, X
    assert quant in (O.Q_F16, O.Q_BF16)      # the reference's "BF16" codes are binary16 (bf16.go:233-317)
    codes = O.f16_encode(X)
    return codes, O.f16_decode(codes)


def prepared_queries(metric, quant, Q):
    """q_eff of prep_queries_kernel: Normalize (cosine), Lower, decode."""
    Q = np.ascontiguousarray(Q, np.float32)
    if metric == O.COSINE:
        Q = O.normalize(Q)
    return Q if quant == O.Q_NONE else O.f16_decode(O.f16_encode(Q))


def sqnorms(V):
    """||v||^2 as f32 (the device sums in f32 in the reference's order: a relative difference of ~1e-7, far below every margin)"""
    V = np.asarray(V, np.float64)
    return (V * V).sum(axis=1).astype(np.float32)


def fragment_operands(quant, values):
    """The binary16 operands the matrix cores multiply, as float64."""
    if quant == O.Q_NONE:
        with np.errstate(over="ignore"):
            return np.asarray(values, np.float32).astype(np.float16).astype(np.float64)
    v16 = np.asarray(values, np.float32).astype(np.float16)
    assert np.array_equal(v16.astype(np.float32), np.asarray(values, np.float32)), "2-byte rows must be exact in binary16"
    return v16.astype(np.float64)


def eligible(metric, quant, dim, min_norm, max_norm, f8_expanded=0):
    """coltt_flat_mfma_eligible_host: the decision search_prepared takes, with no device."""
    import coltt_amd
    L = coltt_amd.lib()
    L.coltt_flat_mfma_eligible_host.restype = C.c_int
    L.coltt_flat_mfma_eligible_host.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_int]
    return int(L.coltt_flat_mfma_eligible_host(int(metric), int(quant), int(dim), float(min_norm), float(max_norm), int(f8_expanded)))


class Scores:
    """Approximate candidate values and float64 exact scores of every (query, row) pair of one store + batch."""

    def __init__(self, metric, quant, values, q_eff):
        self.metric, self.quant, self.dim = metric, quant, values.shape[1]
        r64, q64 = np.asarray(values, np.float64), np.asarray(q_eff, np.float64)
        self.nr, self.nq = sqnorms(values), sqnorms(q_eff)
        self.min_norm, self.max_norm = self.nr.min(), self.nr.max()
        dot_t = fragment_operands(quant, q_eff) @ fragment_operands(quant, values).T
        nr64, nq64 = self.nr.astype(np.float64), self.nq.astype(np.float64)
        with np.errstate(all="ignore"):
            if metric == O.COSINE:
                self.approx = np.abs(1.0 - dot_t / np.sqrt(nq64[:, None] * nr64[None, :]))
                self.exact = np.abs(1.0 - (q64 @ r64.T) / np.sqrt((q64 * q64).sum(1)[:, None] * (r64 * r64).sum(1)[None, :]))
            else:
                self.approx = nq64[:, None] + nr64[None, :] - 2.0 * dot_t
                # the squared distance in difference form, float64 (monotone in the distance the exact scan returns)
                self.exact = np.stack([((r64 - q) ** 2).sum(axis=1) for q in q64])

    def kept_superset(self, k, nearest, margin_override=None, consts=None):
        """Per query: is every true top-k member (bottom-k for the farthest direction, ties at the k-th place included) inside
        s~ <= s~_(k) + margin?  Returns (ok [nq] bool, kept [nq] counts, missed [nq] counts)."""
        n = self.approx.shape[1]
        kk = min(k, n)
        sgn = 1.0 if nearest else -1.0
        a, e = sgn * self.approx, sgn * self.exact
        m = margin(self.metric, self.quant, self.dim, self.nq, self.max_norm, consts).astype(np.float64) if margin_override is None \
            else np.full(len(a), margin_override, np.float64)
        kth_a = np.partition(a, kk - 1, axis=1)[:, kk - 1]
        kth_e = np.partition(e, kk - 1, axis=1)[:, kk - 1]
        with np.errstate(invalid="ignore"):
            kept = a <= (kth_a + m)[:, None]
        member = e <= kth_e[:, None]
        missed = (member & ~kept).sum(axis=1)
        return missed == 0, kept.sum(axis=1), missed


# ------------------------------------------------------------------------------------------------ data sets
def _unit(V):
    return V / np.sqrt((V * V).sum(axis=1, keepdims=True))


def band_set(seed, d, nq, n_fill, base, width=4e-4, planted=200, scale=1.0):
    """Near ties at the k-th place for every k <= planted: per query `planted` rows whose cosine distance to it steps evenly through
    [base - width/2, base + width/2] (base 1.9: the FARTHEST rows), and n_fill random rows that stay outside the band for every query (a
    random row that would fall inside or beyond it is replaced by its component orthogonal to all queries: distance 1).  Rows and queries
    have norm `scale`, so the Euclidean distances have the same geometry: d^2 = 2 scale^2 (1 - cos).  All randomness is O.fill_normal;
    the rows are shuffled so that every segment of the scan meets planted rows.  Returns X [nq * planted + n_fill, d], Q [nq, d], f32."""
    assert d >= 2 * nq
    Qh = _unit(O.fill_normal(seed, (nq, d)).astype(np.float64))
    B, _ = np.linalg.qr(Qh.T)                                  # [d, nq] orthonormal basis of the queries' span
    ortho = lambda V: _unit(V - (V @ B) @ B.T)
    U = ortho(O.fill_normal(seed + 1, (nq * planted, d)).astype(np.float64))
    dist = base + width * (np.arange(planted) / (planted - 1) - 0.5)
    cosv = np.tile(1.0 - dist, nq)[:, None]
    P = cosv * np.repeat(Qh, planted, axis=0) + np.sqrt(1.0 - cosv * cosv) * U
    F = _unit(O.fill_normal(seed + 2, (n_fill, d)).astype(np.float64))
    cf = F @ Qh.T
    guard = 4 * width
    intrude = (cf > 1.0 - (base + width / 2 + guard)).any(axis=1) if base < 1.0 else (cf < 1.0 - (base - width / 2 - guard)).any(axis=1)
    F[intrude] = ortho(F[intrude])
    X = np.concatenate([P, F])
    perm = np.argsort(O.fill_normal(seed + 3, (len(X),)), kind="stable")
    return (X[perm] * scale).astype(np.float32), (Qh * scale).astype(np.float32)


def positive_set(seed, n, d, nq):
    """|Gaussian| rows and queries: sum |a_i b_i| is the dot product itself — no cancellation, the worst case the margins' derivations quote"""
    return np.abs(O.fill_normal(seed, (n, d))), np.abs(O.fill_normal(seed + 1, (nq, d)))


def scaled_set(seed, n, d, nq, s):
    """Gaussian rows and queries times s (s = 1e-5 puts the elements into binary16's subnormal range, 1e-7 next to its smallest step 2^-24)"""
    return (O.fill_normal(seed, (n, d)) * np.float32(s)).astype(np.float32), (O.fill_normal(seed + 1, (nq, d)) * np.float32(s)).astype(np.float32)


def mixed_set(seed, n, d, nq):
    """rows and queries of norm 1e-5, and ONE row of norm 1e3 (||row||^2 = 1e6): max_norm blows the Euclidean margin up to 'keep everything'"""
    X = _unit(O.fill_normal(seed, (n, d)).astype(np.float64)) * 1e-5
    X[n // 2] *= 1e8
    Q = _unit(O.fill_normal(seed + 1, (nq, d)).astype(np.float64)) * 1e-5
    return X.astype(np.float32), Q.astype(np.float32)


def f8_band_set(seed, d, nq, n_fill, planted=200):
    """Near ties for a cosine "f8" store, built in CODE space on values the codec keeps distinct.  The reference's Float8 decodes to the
    levels 0, 1, 2, 3 (x 2^-24) and, with the top bit of the code set, 1 + 2^-8, 2 + 2^-7, 3 + 2^-7 (codes 1, 2, 3, 129, 130, 131).  Per query:
    `planted` rows that follow the prepared query's own levels — except on 24 coordinates, so that the score responds in first order — and
    differ from each other only in WHICH coordinates carry the top bit: ~190 distinct scores inside 3e-4, half of MF_MARGIN.  n_fill rows of
    random codes lie >= 0.1 farther.  Returns (X, codes, Q): f32 inputs that Lower to exactly `codes` (an L2 store keeps them as they are;
    its stream loads into a cosine store), and the raw queries."""
    xs = O.fill_normal(seed, (200000,)); c = O.f8_encode(xs)
    inp = np.zeros(256, np.float32)
    for code in (0, 1, 2, 3, 129, 130, 131):
        inp[code] = xs[np.nonzero(c == code)[0][0]]
    Q = O.fill_normal(seed + 1, (nq, d))
    lv = np.rint(O.f8_decode(O.f8_encode(O.normalize(Q))).astype(np.float64) * 2.0 ** 24).astype(np.int64)     # levels 0..3 of the prepared queries
    rows = []
    for i in range(nq):
        b = lv[i].copy()
        b[b == 0] = 1
        b[:24] = b[:24] % 3 + 1
        tog = O.fill_normal(seed + 2 + i, (planted, d)) > 0.8
        rows.append(np.where(tog, b[None, :] + 128, b[None, :]))
    F = np.array([0, 1, 2, 3, 129, 130, 131])[(np.abs(O.fill_normal(seed + 40, (n_fill, d))) * 2.6).astype(np.int64) % 7]
    F[:, 0] = 1                                                # no zero vectors: no NaN scores
    codes = np.concatenate(rows + [F]).astype(np.uint8)
    codes = codes[np.argsort(O.fill_normal(seed + 41, (len(codes),)), kind="stable")]
    X = inp[codes]
    assert np.array_equal(O.f8_encode(X), codes)
    return X, codes, Q
