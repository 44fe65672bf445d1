"""The query quantiser of the row filter's integer phase A (coltt_amd/csrc/rows8.hpp: query_digits8i; the scalar steps are row_filter8i.hpp's),
restated in numpy for the tests that check the bound (test_row_filter8i_bound.py) and the device's sums (test_gpu_row_filter8i.py), and the header
itself compiled with g++ for both."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QMAX = 16256
BITS_8I = 80   # coltt::ROW_FILTER_8I


def quantise_query(q):
    """(t, levels qh [dim] int32, h [dim] int8, l [dim] int8, stored e_q) of one f32 query; a zero query, a query with a non-finite element and a
    scale that underflows to 0 get t = 0, levels 0 and e_q = +inf"""
    q = np.ascontiguousarray(q, np.float32)
    z = np.zeros(q.size, np.int32)
    none = (np.float32(0), z, z.astype(np.int8), z.astype(np.int8), np.float32(np.inf))
    if not np.all(np.isfinite(q)):
        return none
    t = np.float32(np.float64(np.max(np.abs(q))) / np.float64(QMAX))   # the f64 quotient of two f32 values, rounded to f32
    if not t > 0:
        return none
    with np.errstate(over="ignore"):
        qh = np.clip(np.rint((q.astype(np.float64) / np.float64(t)).astype(np.float32)), -QMAX, QMAX).astype(np.int32)
    h = (qh + 64) >> 7
    l = qh - 128 * h
    assert h.min() >= -127 and h.max() <= 127 and l.min() >= -64 and l.max() <= 63
    d = q.astype(np.float64) - np.float64(t) * qh.astype(np.float64)   # the product is exact in f64
    ev = math.sqrt(float(np.sum(d * d))) * (1.0 + 2.0 ** -20)
    e = np.float32(ev)
    if float(e) < ev:
        e = np.nextafter(e, np.float32(np.inf), dtype=np.float32)
    return t, qh, h.astype(np.int8), l.astype(np.int8), e


def int_dot(qh, codes):
    """sum qh_i c_i per row, exact (int64); codes [m, dim] int8"""
    return np.asarray(codes, np.int64) @ np.asarray(qh, np.int64)


_SRC = r'''
#include <cmath>
#include "row_filter8i.hpp"
extern "C" {
float rf8i_dlo(long long I, float t, float eq, float s, float e, int dim, float qn, float rn) { return coltt::row_filter8i_dlo(I, t, eq, s, e, dim, qn, rn); }
void rf8i_dlo_many(long n, const long long* I, const float* t, const float* eq, const float* s, const float* e, int dim, const float* qn, const float* rn, float* out) {
  for (long i = 0; i < n; i++) out[i] = coltt::row_filter8i_dlo(I[i], t[i], eq[i], s[i], e[i], dim, qn[i], rn[i]);
}
float rf8i_upper(long long I, float t, float eq, float s, float e, int dim, float qn, float rn) {   // U of row_filter8i_dlo
  const float den = (float)sqrt((double)(qn * rn));
  return (float)(((double)t * (double)s) * (double)I) + coltt::row_filter8i_margin(e, eq, dim, qn, rn, den);
}
int rf_rejects(float dlo, float lb) { return coltt::row_filter_rejects(dlo, lb) ? 1 : 0; }
// the quantiser's scalar steps, as the kernel calls them
float rf8i_scale(float mx, int bad) { return coltt::row_filter8i_scale(mx, bad != 0); }
int rf8i_level(float x, float t) { return coltt::row_filter8i_level(x, t); }
void rf8i_digits(int qh, int* h, int* l) { coltt::row_filter8i_digits(qh, *h, *l); }
float rf8i_err(double err) { return coltt::row_filter8i_err(err); }
}
'''


def compile_header(tmpdir):
    gxx = shutil.which("g++")
    assert gxx, "the margin header is checked as compiled code: g++ is needed"
    src = os.path.join(str(tmpdir), "rf8i.cpp"); so = os.path.join(str(tmpdir), "librf8i.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "coltt_amd", "csrc"), src, "-o", so])
    L = C.CDLL(so)
    fp = C.POINTER(C.c_float); lp = C.POINTER(C.c_longlong); ip = C.POINTER(C.c_int)
    sig = [C.c_longlong, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
    L.rf8i_dlo.restype = C.c_float; L.rf8i_dlo.argtypes = sig
    L.rf8i_upper.restype = C.c_float; L.rf8i_upper.argtypes = sig
    L.rf8i_dlo_many.restype = None; L.rf8i_dlo_many.argtypes = [C.c_long, lp, fp, fp, fp, fp, C.c_int, fp, fp, fp]
    L.rf_rejects.restype = C.c_int; L.rf_rejects.argtypes = [C.c_float, C.c_float]
    L.rf8i_scale.restype = C.c_float; L.rf8i_scale.argtypes = [C.c_float, C.c_int]
    L.rf8i_level.restype = C.c_int; L.rf8i_level.argtypes = [C.c_float, C.c_float]
    L.rf8i_digits.restype = None; L.rf8i_digits.argtypes = [C.c_int, ip, ip]
    L.rf8i_err.restype = C.c_float; L.rf8i_err.argtypes = [C.c_double]
    return L


def dlo8i(L, I, t, eq, s, e, dim, qn, rn):
    """row_filter8i_dlo element-wise (arrays are broadcast against I)"""
    I = np.ascontiguousarray(I, np.int64); out = np.empty(I.shape, np.float32)
    f = lambda a: np.ascontiguousarray(np.broadcast_to(np.asarray(a, np.float32), I.shape))
    t, eq, s, e, qn, rn = (f(a) for a in (t, eq, s, e, qn, rn))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    L.rf8i_dlo_many(I.size, I.ctypes.data_as(C.POINTER(C.c_longlong)), fp(t), fp(eq), fp(s), fp(e), int(dim), fp(qn), fp(rn), fp(out))
    return out
