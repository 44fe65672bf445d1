"""The margin of the level-0 row filter over the 8-BIT shadow is a theorem, not a tolerance (coltt_amd/csrc/row_filter8.hpp).

The header is compiled with the host compiler — the very function the kernel runs — and the ingest quantiser (rows8_ingest.hpp: rows_b_kernel) is restated
here in numpy.  Against exact rational arithmetic (fractions.Fraction over the exact binary values of the f32 inputs):

    dot_exact_f32  <=  s G + E_exact  <=  U = fl(fl(s G) + E)            and            d_exact >= d_lo

where dot_exact_f32 / d_exact come from the oracle's AVX-order kernel (what the exact GPU kernel reproduces bit for bit), G is the f32 sum of
q_i * (float)c_i over the row's codes, E_exact the derivation's steps (a)-(c) evaluated exactly with the TRUE sums (gamma_k P, the true
sum q_i (x_i - s c_i), gamma_k s sum |q_i c_i|), and U / d_lo what the header returns from the f32 squared norms and the STORED (s, e) alone.
The stored e is checked to be no smaller than the exact error norm.  Zero violations: a condition, not a rate."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import oracle as O
from row_filter8_ref import quantise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "the margin header is checked as compiled code: g++ is needed"
    d = tmp_path_factory.mktemp("rf8")
    src = d / "rf8.cpp"
    src.write_text('#include "row_filter8.hpp"\n'
                   'extern "C" float rf8_margin(float e, int dim, float qn, float rn, float den) { return coltt::row_filter8_margin(e, dim, qn, rn, den); }\n'
                   'extern "C" float rf8_dlo(float G, float s, float e, int dim, float qn, float rn) { return coltt::row_filter8_dlo(G, s, e, dim, qn, rn); }\n'
                   'extern "C" int rf_rejects(float dlo, float lb) { return coltt::row_filter_rejects(dlo, lb) ? 1 : 0; }\n')
    so = d / "librf8.so"
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "coltt_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.rf8_margin.restype = C.c_float; L.rf8_margin.argtypes = [C.c_float, C.c_int, C.c_float, C.c_float, C.c_float]
    L.rf8_dlo.restype = C.c_float; L.rf8_dlo.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
    L.rf_rejects.restype = C.c_int; L.rf_rejects.argtypes = [C.c_float, C.c_float]
    return L


def _sum_kernel_order(q, c):
    """the filter's f32 sum in the kernel's shape: partial sum r takes the elements i % 8 == r in increasing i (multiply and add rounded
    separately here; the kernel fuses them, which rounds less), then the 3-level tree"""
    q8 = q.reshape(-1, 8); c8 = c.astype(np.float32).reshape(-1, 8)
    acc = np.zeros(8, np.float32)
    for s in range(q8.shape[0]):
        acc = (acc + (q8[s] * c8[s]).astype(np.float32)).astype(np.float32)
    a = [np.float32(acc[0] + acc[1]), np.float32(acc[2] + acc[3]), np.float32(acc[4] + acc[5]), np.float32(acc[6] + acc[7])]
    return np.float32(np.float32(a[0] + a[1]) + np.float32(a[2] + a[3]))


def _sum_rounded_once(q, c):
    """the other end of 'any order, fused or not': the exact sum rounded once"""
    return np.float32(float(sum(Fr(float(a)) * int(b) for a, b in zip(q, c))))


def _check(rf, q, x, tag, stats=None):
    q = np.ascontiguousarray(q, np.float32); x = np.ascontiguousarray(x, np.float32)
    dim = q.size
    c, s, e = quantise(x)
    assert np.isfinite(e), tag
    fq = [Fr(float(v)) for v in q]; fx = [Fr(float(v)) for v in x]; fs = Fr(float(s)); fc = [int(v) for v in c]
    bad = []
    err2 = sum((a - fs * b) ** 2 for a, b in zip(fx, fc))
    if not Fr(float(e)) ** 2 >= err2:
        bad.append((tag, "stored e below the exact error norm", float(e), float(err2) ** 0.5))
    if not Fr(float(e)) ** 2 <= err2 * Fr(1025, 1024) ** 2 + Fr(1, 2 ** 290):
        bad.append((tag, "stored e more than 2^-10 above the exact error norm", float(e), float(err2) ** 0.5))
    K, qn, rn = O.cosine_parts(q, x)                  # the exact kernel's dot product and the two squared norms, AVX order, f32
    d_exact = O.cosine(q, x)
    P = sum(abs(a * b) for a, b in zip(fq, fx))
    A = sum(abs(a) * abs(b) for a, b in zip(fq, fc))
    T_gap = sum(a * (b - fs * cc) for a, b, cc in zip(fq, fx, fc))   # T - T^
    k = dim // 8 + 4; u = Fr(1, 2 ** 24); gam = k * u / (1 - k * u)
    e_exact = gam * P + T_gap + gam * fs * A
    den = np.float32(np.sqrt(np.float64(np.float32(qn * rn))))
    for name, G in (("kernel-order", _sum_kernel_order(q, c)), ("rounded-once", _sum_rounded_once(q, c))):
        E = np.float32(rf.rf8_margin(float(e), dim, float(qn), float(rn), float(den)))
        U = np.float32(np.float32(s * G) + E)
        d_lo = np.float32(rf.rf8_dlo(float(G), float(s), float(e), dim, float(qn), float(rn)))
        if np.isfinite(U) and np.isfinite(K):
            sG = fs * Fr(float(G))
            if not (Fr(float(K)) <= sG + e_exact):
                bad.append((tag, name, "theorem (a)-(c)", float(K), float(sG), float(e_exact)))
            if not (sG + e_exact <= Fr(float(U))):
                bad.append((tag, name, "f32 margin below the exact bound", float(sG), float(e_exact), float(U)))
            if not (K <= U):
                bad.append((tag, name, "K > U", float(K), float(U)))
            if stats is not None and den > 0:
                stats.append(float(E / den))
        if np.isfinite(d_lo) and not (d_exact >= d_lo):
            bad.append((tag, name, "d_exact < d_lo", float(d_exact), float(d_lo)))
        if np.isfinite(d_lo) and np.isfinite(d_exact):   # the verdict can never reject what the exact kernel would admit
            for lb in (d_exact, np.nextafter(d_exact, np.float32(4), dtype=np.float32)):
                if rf.rf_rejects(float(d_lo), float(lb)) and d_exact < lb:
                    bad.append((tag, name, "rejected an admissible neighbour", float(d_exact), float(d_lo), float(lb)))
    return bad


def _unit(seed, dim):
    return O.normalize(O.fill_normal(seed, (dim,)))


def test_margin_covers_the_exact_kernel_on_every_adversarial_family(rf):
    bad = []; n = 0
    rng = np.random.default_rng(20261017)
    for dim in (256, 768, 1536):
        # random unit rows, random (not normalised) queries
        for t in range(16):
            bad += _check(rf, O.fill_normal(100 * dim + t, (dim,)), _unit(7 * dim + t, dim), f"random d{dim} #{t}"); n += 1
        # all-same-sign: no cancellation, every error adds up
        for t in range(4):
            x = np.abs(_unit(900 + dim + t, dim)); q = np.abs(O.fill_normal(950 + dim + t, (dim,)))
            bad += _check(rf, q, x, f"same-sign d{dim} #{t}"); bad += _check(rf, -q, x, f"opposite-sign d{dim} #{t}"); n += 2
        # the query PARALLEL to the quantisation error x - s c: Cauchy-Schwarz with the stored e is tight (and anti-parallel)
        for t in range(6):
            x = _unit(1200 + dim + t, dim); c, s, e = quantise(x)
            r = (x.astype(np.float64) - np.float64(s) * c.astype(np.float64))
            q = (r / np.linalg.norm(r) * (1.0 if t % 2 == 0 else 37.0)).astype(np.float32)
            bad += _check(rf, q, x, f"error-parallel d{dim} #{t}"); bad += _check(rf, -q, x, f"error-antiparallel d{dim} #{t}"); n += 2
            # ... and its sign pattern on a dense query
            q = (np.abs(O.fill_normal(1250 + dim + t, (dim,))) * np.where(r >= 0, 1, -1)).astype(np.float32)
            bad += _check(rf, q, x, f"error-aligned d{dim} #{t}"); n += 1
        # elements ON half-steps of the code grid: s = 2^-7 exactly, x_i = (m + 1/2) s — rint ties, to even both ways
        for t in range(4):
            m = rng.integers(-126, 126, dim); x = ((m + 0.5) * 2.0 ** -7).astype(np.float32); x[int(rng.integers(0, dim))] = np.float32(127 * 2.0 ** -7)
            c, s, e = quantise(x)
            assert s == np.float32(2.0 ** -7) and np.all(c[x != x.max()] % 2 == 0)
            q = np.abs(O.fill_normal(1500 + dim + t, (dim,))) * (np.where(x.astype(np.float64) - 2.0 ** -7 * c >= 0, 1, -1) if t % 2 else 1)
            bad += _check(rf, q, x, f"half-steps d{dim} #{t}"); n += 1
        # one-hot rows, against a query that is one-hot there too, and a dense one
        for t in range(4):
            x = np.zeros(dim, np.float32); i = int(rng.integers(0, dim)); x[i] = 1.0 if t % 2 else -1.0
            q = np.zeros(dim, np.float32); q[i] = 0.75
            bad += _check(rf, q, x, f"one-hot/one-hot d{dim} #{t}"); bad += _check(rf, O.fill_normal(1900 + dim + t, (dim,)), x, f"one-hot d{dim} #{t}"); n += 2
        # a few huge outliers: everything else rounds to code 0
        for t in range(4):
            x = (O.fill_normal(2000 + dim + t, (dim,)) * np.float32(0.01)).astype(np.float32)
            x[rng.integers(0, dim, 3)] = np.float32(1e3) * rng.choice([-1, 1], 3).astype(np.float32)
            c, s, e = quantise(x); assert np.count_nonzero(c) <= 3
            q = O.fill_normal(2050 + dim + t, (dim,)); q[np.abs(x) > 1] *= np.float32(1e-3)   # the dot product lives in what the codes miss
            bad += _check(rf, q, x, f"outliers d{dim} #{t}"); bad += _check(rf, np.abs(q) * np.sign(x), x, f"outliers aligned d{dim} #{t}"); n += 2
        # constant rows
        for t, v in enumerate((0.3, -1.0, 1e-20, 7e18)):
            x = np.full(dim, v, np.float32)
            bad += _check(rf, O.fill_normal(2080 + dim + t, (dim,)), x, f"constant {v} d{dim}"); bad += _check(rf, np.abs(O.fill_normal(2090 + dim + t, (dim,))), x, f"constant {v} same-sign d{dim}"); n += 2
        # queries far from unit norm (queries are not normalised)
        for t, sc in enumerate((1e-6, 1e-3, 37.0, 1e3, 1e6, 1e12)):
            bad += _check(rf, O.fill_normal(2100 + dim + t, (dim,)) * np.float32(sc), _unit(2150 + dim + t, dim), f"|q| x{sc} d{dim}"); n += 1
        # near-duplicates of the query: the distances the walk's lowerBound lives among
        for t in range(6):
            x = _unit(2300 + dim + t, dim); q = x + O.fill_normal(2350 + dim + t, (dim,)) * np.float32(1e-3 * 4 ** t)
            bad += _check(rf, q, x, f"near d{dim} #{t}"); n += 1
    assert n > 150
    assert not bad, bad[:10]


def test_nothing_is_certified_for_rows_without_an_error_norm_or_inputs_out_of_range(rf):
    """zero rows, rows with inf / NaN: the quantiser stores e = +inf and the header gives no verdict; the same for overflowing sums, vanishing or
    overflowing norms, NaN anywhere"""
    inf = float("inf"); nan = float("nan")
    for x in (np.zeros(256, np.float32), np.r_[np.ones(255, np.float32), np.float32(inf)], np.r_[np.float32(nan), np.ones(255, np.float32)],
              np.r_[np.float32(-inf), np.zeros(767, np.float32)], np.full(256, 1e-45, np.float32)):
        c, s, e = quantise(x)
        assert e == np.inf and s == 0 and not np.any(c)
        for G in (0.0, 1.0, -1e30):
            d = rf.rf8_dlo(G, float(s), float(e), x.size, 1.0, max(float(np.sum(x[np.isfinite(x)] ** 2)), 1.0))
            for lb in (-1.0, 0.0, 0.5, 2.0):
                assert not rf.rf_rejects(d, lb), (x[:4], G, d, lb)
    for G, s, e, qn, rn in ((inf, .01, .01, 1.0, 1.0), (-inf, .01, .01, 1.0, 1.0), (nan, .01, .01, 1.0, 1.0), (0.5, .01, .01, 0.0, 1.0), (0.5, .01, .01, 1e-20, 1e-20),
                            (0.5, .01, .01, inf, 1.0), (0.5, .01, .01, 1e30, 1e30), (0.5, .01, .01, nan, 1.0), (0.5, .01, .01, 1.0, nan), (0.5, nan, .01, 1.0, 1.0),
                            (0.5, .01, nan, 1.0, 1.0), (0.5, .01, inf, 1.0, 1.0), (0.5, inf, .01, 1.0, 1.0), (0.5, 0.0, .01, 1.0, 1.0), (0.5, .01, -1.0, 1.0, 1.0), (3e38, 3e38, .01, 1.0, 1.0)):
        d = rf.rf8_dlo(G, s, e, 768, qn, rn)
        for lb in (-1.0, 0.0, 0.5, 2.0):
            assert not rf.rf_rejects(d, lb), (G, s, e, qn, rn, d, lb)
    # a 1e30 outlier: finite, quantised (every other code 0), certified like any row — the bound holds (checked above on the outlier family) and
    # the squared norm overflows, so no verdict either way
    x = np.ones(256, np.float32); x[7] = 1e30
    c, s, e = quantise(x)
    assert np.isfinite(e) and np.count_nonzero(c) == 1
    with np.errstate(over="ignore"):
        rn = float(np.float32(np.sum(x.astype(np.float32) ** 2, dtype=np.float32)))
    assert not rf.rf_rejects(rf.rf8_dlo(1.0, float(s), float(e), 256, 256.0, rn), 0.1)


def test_the_margin_is_small_enough_to_filter(rf):
    """not a correctness condition — the size the design was reasoned with: about 8e-3 den for 768-d Gaussian rows (e = 0.0076 ||x||)"""
    x = _unit(42, 768); c, s, e = quantise(x)
    assert 0.006 < float(e) < 0.009
    m = rf.rf8_margin(float(e), 768, 1.0, 1.0, 1.0)
    assert float(e) < m < 1.01 * float(e) + 3e-5
