"""Host-side references for the row-filter probe (coltt_hnsw_row_filter_probe): what a CONFORMING phase A may return for a (query, row) pair.

The proof of the filter (coltt_amd/csrc/row_filter8.hpp, row_filter.hpp) has a premise about the kernel: the shadow sum it forms is sum q_i * c_i over
the right element pairs, to within gamma_k * sum |q_i c_i| (step (c) of the 8-bit header, (b) of the binary16 one) plus the underflow allowance of
step (e).  This module turns that premise into an interval, with no tolerance of its own:

    S = fsum(q_i * c_i), A = fsum(|q_i c_i|)      in f64: the products are exact (24 + 7 bits for the codes, 24 + 11 for binary16), fsum rounds once
    [G_lo, G_hi] = S -+ (gamma_k A + dim 2^-149 + 2^-50 A)   rounded outwards to f32;  gamma_k = k u / (1 - k u), k = dim / 8 + 4, u = 2^-24
                                                  (2^-50 A pays for the f64 roundings of S, A and of the interval's own arithmetic)
    d_lo in [dlo(G_hi), dlo(G_lo)]                the headers' own functions, compiled with g++: every operation in them is correctly rounded and
                                                  s > 0, so d_lo is non-increasing in G

and generates the rows and queries both the CPU test of this reference and the GPU test of the kernels use."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (256, 512, 768, 1024, 1280, 1536, 2304)   # every branch of both dispatches in Group8FilterEval::filtered; bursts per row 1, 2, 3, 4 and 5
NBR_NONE = 0xFFFFFFFF

_SRC = r'''
#include <cmath>
#include "row_filter8.hpp"
extern "C" {
float rf8_dlo(float G, float s, float e, int dim, float qn, float rn) { return coltt::row_filter8_dlo(G, s, e, dim, qn, rn); }
float rf_dlo(float F, int dim, float qn, float rn) { return coltt::row_filter_dlo(F, dim, qn, rn); }
int rf_rejects(float dlo, float lb) { return coltt::row_filter_rejects(dlo, lb) ? 1 : 0; }
void rf8_dlo_many(long n, const float* G, const float* s, const float* e, int dim, const float* qn, const float* rn, float* out) {
  for (long i = 0; i < n; i++) out[i] = coltt::row_filter8_dlo(G[i], s[i], e[i], dim, qn[i], rn[i]);
}
void rf_dlo_many(long n, const float* F, int dim, const float* qn, const float* rn, float* out) {
  for (long i = 0; i < n; i++) out[i] = coltt::row_filter_dlo(F[i], dim, qn[i], rn[i]);
}
// the shadow sum in the kernel's shape (rows8.hpp: group8_stream_b / group8_burst_b / group8_stream_h): partial sum r takes the elements i % 8 == r
// in increasing i, each a fused multiply-add, then the 3-level tree of group8_hsum.  c: the shadow values as f32 (codes or binary16 values, exact)
float fused_kernel_order_sum(const float* q, const float* c, int dim) {
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < dim; i++) acc[i & 7] = fmaf(q[i], c[i], acc[i & 7]);
  const float a = acc[0] + acc[1], b = acc[2] + acc[3], c2 = acc[4] + acc[5], d = acc[6] + acc[7];
  const float ab = a + b, cd = c2 + d;
  return ab + cd;
}
}
'''


def compile_headers(tmpdir):
    """the two margin headers (and the kernel-order sum restated in C) as a ctypes library"""
    gxx = shutil.which("g++")
    assert gxx, "the margin headers are checked as compiled code: g++ is needed"
    src = os.path.join(str(tmpdir), "rfp.cpp"); so = os.path.join(str(tmpdir), "librfp.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "coltt_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    L.rf8_dlo.restype = C.c_float; L.rf8_dlo.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
    L.rf_dlo.restype = C.c_float; L.rf_dlo.argtypes = [C.c_float, C.c_int, C.c_float, C.c_float]
    L.rf_rejects.restype = C.c_int; L.rf_rejects.argtypes = [C.c_float, C.c_float]
    L.rf8_dlo_many.restype = None; L.rf8_dlo_many.argtypes = [C.c_long, fp, fp, fp, C.c_int, fp, fp, fp]
    L.rf_dlo_many.restype = None; L.rf_dlo_many.argtypes = [C.c_long, fp, C.c_int, fp, fp, fp]
    L.fused_kernel_order_sum.restype = C.c_float; L.fused_kernel_order_sum.argtypes = [fp, fp, C.c_int]
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32c(a, shape):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), shape))


def dlo8(L, G, s, e, dim, qn, rn):
    """row_filter8_dlo element-wise (arrays are broadcast against G)"""
    G = np.ascontiguousarray(G, np.float32); out = np.empty(G.shape, np.float32)
    s, e, qn, rn = (_f32c(a, G.shape) for a in (s, e, qn, rn))
    L.rf8_dlo_many(G.size, _fp(G), _fp(s), _fp(e), int(dim), _fp(qn), _fp(rn), _fp(out))
    return out


def dlo16(L, F, dim, qn, rn):
    """row_filter_dlo element-wise"""
    F = np.ascontiguousarray(F, np.float32); out = np.empty(F.shape, np.float32)
    qn, rn = (_f32c(a, F.shape) for a in (qn, rn))
    L.rf_dlo_many(F.size, _fp(F), int(dim), _fp(qn), _fp(rn), _fp(out))
    return out


def fused_kernel_order_sum(L, q, c):
    q = np.ascontiguousarray(q, np.float32); c = np.ascontiguousarray(c, np.float32)
    return np.float32(L.fused_kernel_order_sum(_fp(q), _fp(c), int(q.size)))


def _f32_down(v):
    """the largest f32 <= v (v a finite f64 inside the f32 range)"""
    f = np.float32(v)
    return np.nextafter(f, np.float32(-np.inf), dtype=np.float32) if float(f) > v else f


def _f32_up(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf), dtype=np.float32) if float(f) < v else f


def sum_interval(q, shadow):
    """[G_lo, G_hi] (f32 arrays) and S, A (f64) for one query against the shadow values of m rows (shadow [m, dim]: int8 codes or float16 values,
    every one finite).  Only the query's non-zero elements are summed: a zero product adds nothing to S or A."""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    dim = q64.size
    nz = np.flatnonzero(q64)
    P = q64[nz][None, :] * np.asarray(shadow)[:, nz].astype(np.float64)     # exact products
    assert np.all(np.isfinite(P))
    aP = np.abs(P)
    assert not np.any((aP > 0) & (aP < 2.0 ** -1000)), "a product below the f64 normal range: the f64 products would not be exact"
    S = np.array([math.fsum(r) for r in P]); A = np.array([math.fsum(r) for r in aP])
    k = dim // 8 + 4; u = 2.0 ** -24; gam = k * u / (1 - k * u)
    w = (gam * A + dim * 2.0 ** -149 + 2.0 ** -50 * A) * (1 + 2.0 ** -50)     # (the three f64 operations that form w itself)
    lo = np.array([_f32_down(v) for v in S - w], np.float32); hi = np.array([_f32_up(v) for v in S + w], np.float32)
    return lo, hi, S, A


def f32_below(x):
    return np.nextafter(np.asarray(x, np.float32), np.float32(-np.inf), dtype=np.float32)


def f32_above(x):
    return np.nextafter(np.asarray(x, np.float32), np.float32(np.inf), dtype=np.float32)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------------------
N_RAMP = 32   # the first N_RAMP raw rows: locally distinct codes, for the element-mapping check

_COPRIME_255 = [a for a in range(1, 255) if math.gcd(a, 255) == 1]


def raw_rows(dim, seed=9000):
    """320 raw rows (what the test inserts; a cosine index stores them normalised): the adversarial families of the CPU bound tests, and
    N_RAMP 'ramp' rows in front whose codes c_i = (a i + b) mod 255 - 127 (a coprime to 255) differ from every code within 254 elements"""
    rng = np.random.default_rng(seed + dim)
    fam = []
    i = np.arange(dim)
    ramp = np.stack([((_COPRIME_255[(3 + 5 * r) % len(_COPRIME_255)] * i + 17 * r) % 255 - 127).astype(np.float32) for r in range(N_RAMP)])
    g = lambda k, n: O.fill_normal(seed + dim + k, (n, dim))
    fam.append(g(1, 126))                                                                      # Gaussian
    fam.append(g(2, 40) * np.linspace(0.1, 9.0, 40, dtype=np.float32)[:, None])               # ... scaled
    fam.append(np.abs(g(3, 16)) * np.where(np.arange(16) % 2, -1, 1).astype(np.float32)[:, None])   # same sign
    fam.append(np.array([0.3, -1.0, 1e-15, 7e15], np.float32)[:, None] * np.ones((4, dim), np.float32))   # constant
    oh = np.zeros((24, dim), np.float32)
    for t in range(24):                                                                        # one-hot: first / last elements, every residue
        oh[t, [0, dim - 1, 7, dim - 8][t] if t < 4 else int(rng.integers(0, dim))] = 1.0 if t % 2 else -2.5
    fam.append(oh)
    sp = g(4, 20); sp[rng.random((20, dim)) < 0.95] = 0; fam.append(sp)                        # 95 % zeros
    ol = g(5, 20) * np.float32(0.01)
    for t in range(20):                                                                        # 3 huge outliers: everything else rounds to code 0
        ol[t, rng.choice(dim, 3, replace=False)] = np.float32(1e3) * rng.choice([-1, 1], 3).astype(np.float32)
    fam.append(ol)
    hs = ((rng.integers(-126, 126, (16, dim)) + 0.5) * 2.0 ** -7).astype(np.float32)           # half-steps of the code grid (before Normalize)
    hs[np.arange(16), rng.integers(0, dim, 16)] = np.float32(127 * 2.0 ** -7)
    fam.append(hs)
    fam.append(g(6, 10) * np.float32(1e-15)); fam.append(g(7, 10) * np.float32(1e15))          # tiny and huge rows
    big = g(8, 1); big[0, 5] = np.float32(1e30); fam.append(big)                               # rows without a certificate
    fam.append(np.zeros((1, dim), np.float32))
    rest = np.concatenate(fam)
    rest = rest[rng.permutation(len(rest))]                                                    # every chunk of 32 mixes the families
    return np.ascontiguousarray(np.concatenate([ramp, rest]), np.float32)


def one_hot_queries(dim):
    """dim queries, q_i = 0.75 at element i, alternating sign"""
    Q = np.zeros((dim, dim), np.float32)
    Q[np.arange(dim), np.arange(dim)] = np.where(np.arange(dim) % 2, -0.75, 0.75).astype(np.float32)
    return Q


def dense_queries(dim, rows, codes, meta, seed=9500):
    """(queries [nq, dim], slot of the row each one was derived from or -1): Gaussian, same-sign, far from unit norm, near-duplicates of stored rows,
    and queries parallel / anti-parallel to the quantisation error x - s c of a stored row (Cauchy-Schwarz with the stored e is tight there)"""
    rng = np.random.default_rng(seed + dim)
    g = lambda k, n: O.fill_normal(seed + dim + k, (n, dim))
    Q = [g(1, 6), np.abs(g(2, 2)), -np.abs(g(3, 2))]; src = [-1] * 10
    for t, sc in enumerate((1e-6, 1e-3, 37.0, 1e6)):
        Q.append(g(10 + t, 1) * np.float32(sc)); src.append(-1)
    ok = np.flatnonzero(np.isfinite(meta[:, 1]))
    for t, r in enumerate(rng.choice(ok, 6, replace=False)):
        Q.append((rows[r] + g(20 + t, 1)[0] * np.float32(1e-3 * 4 ** t) / np.float32(np.sqrt(dim)))[None, :]); src.append(int(r))
    for t, r in enumerate(rng.choice(ok, 4, replace=False)):
        err = rows[r].astype(np.float64) - np.float64(meta[r, 0]) * codes[r].astype(np.float64)
        n = np.linalg.norm(err)
        if n > 0:
            q = (err / n).astype(np.float32)
            Q.append(q[None, :]); src.append(int(r)); Q.append(-q[None, :]); src.append(int(r))
    return np.ascontiguousarray(np.concatenate(Q), np.float32), np.array(src)


def distinct_share(vals):
    """share of (row, element) pairs whose shadow value differs from every value at the same residue i % 8 within +-64 elements (vals [m, dim])"""
    m, dim = vals.shape
    same = np.zeros((m, dim), bool)
    for k in range(1, 9):
        eq = vals[:, 8 * k:] == vals[:, :-8 * k]
        same[:, 8 * k:] |= eq; same[:, :-8 * k] |= eq
    return 1.0 - same.mean()
