"""The margin of the level-0 row filter is a theorem, not a tolerance (coltt_amd/csrc/row_filter.hpp).

The header is compiled with the host compiler — the very function the kernel runs — and checked against exact rational arithmetic
(fractions.Fraction over the exact binary values of the f32 inputs):

    dot_exact_f32  <=  F + E_exact(P, ||q||_1)  <=  U = fl(F + E)            and            d_exact >= d_lo

where dot_exact_f32 / d_exact come from the oracle's AVX-order kernel (what the exact GPU kernel reproduces bit for bit), F is the f32 sum over the
binary16 shadow of the row, E_exact the derivation's bound (a)-(c) evaluated exactly with the TRUE sum |q_i x_i| and 1-norm, and U / d_lo what the
header returns from the f32 squared norms alone.  Zero violations: a condition, not a rate."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction as Fr

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "the margin header is checked as compiled code: g++ is needed"
    d = tmp_path_factory.mktemp("rf")
    src = d / "rf.cpp"
    src.write_text('#include "row_filter.hpp"\n'
                   'extern "C" float rf_margin(int dim, float qn, float rn, float den) { return coltt::row_filter_margin(dim, qn, rn, den); }\n'
                   'extern "C" float rf_dlo(float F, int dim, float qn, float rn) { return coltt::row_filter_dlo(F, dim, qn, rn); }\n'
                   'extern "C" int rf_rejects(float dlo, float lb) { return coltt::row_filter_rejects(dlo, lb) ? 1 : 0; }\n')
    so = d / "librf.so"
    subprocess.check_call([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", os.path.join(ROOT, "coltt_amd", "csrc"), str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.rf_margin.restype = C.c_float; L.rf_margin.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float]
    L.rf_dlo.restype = C.c_float; L.rf_dlo.argtypes = [C.c_float, C.c_int, C.c_float, C.c_float]
    L.rf_rejects.restype = C.c_int; L.rf_rejects.argtypes = [C.c_float, C.c_float]
    return L


def _shadow_sum_kernel_order(q, h):
    """the filter's f32 sum in the kernel's shape: partial sum r takes the elements i % 8 == r in increasing i (multiply and add rounded
    separately here; the kernel fuses them, which rounds less), then the 3-level tree"""
    q8 = q.reshape(-1, 8); h8 = h.astype(np.float32).reshape(-1, 8)
    acc = np.zeros(8, np.float32)
    for s in range(q8.shape[0]):
        acc = (acc + (q8[s] * h8[s]).astype(np.float32)).astype(np.float32)
    a = [np.float32(acc[0] + acc[1]), np.float32(acc[2] + acc[3]), np.float32(acc[4] + acc[5]), np.float32(acc[6] + acc[7])]
    return np.float32(np.float32(a[0] + a[1]) + np.float32(a[2] + a[3]))


def _shadow_sum_rounded_once(q, h):
    """the other end of 'any order, fused or not': the exact sum rounded once"""
    return np.float32(float(sum(Fr(float(a)) * Fr(float(b)) for a, b in zip(q, h.astype(np.float32)))))


def _check(rf, q, x, tag):
    q = np.ascontiguousarray(q, np.float32); x = np.ascontiguousarray(x, np.float32)
    dim = q.size
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)                      # round to nearest even, as the ingest kernel's conversion
    K, qn, rn = O.cosine_parts(q, x)                  # the exact kernel's dot product and the two squared norms, AVX order, f32
    d_exact = O.cosine(q, x)
    fq = [Fr(float(v)) for v in q]; fx = [Fr(float(v)) for v in x]
    P = sum(abs(a * b) for a, b in zip(fq, fx)); Q1 = sum(abs(a) for a in fq)
    k = dim // 8 + 4; u = Fr(1, 2 ** 24); gam = k * u / (1 - k * u)
    e_exact = (Fr(1, 2 ** 11) + (2 + Fr(1, 2 ** 11)) * gam) * P + (1 + gam) * Fr(1, 2 ** 25) * Q1
    den = np.float32(np.sqrt(np.float64(np.float32(qn * rn))))
    bad = []
    for name, F in (("kernel-order", _shadow_sum_kernel_order(q, h)), ("rounded-once", _shadow_sum_rounded_once(q, h))):
        if not np.isfinite(F):
            continue                                  # an infinity in the shadow: the header must not certify (checked below)
        E = np.float32(rf.rf_margin(dim, float(qn), float(rn), float(den)))
        U = np.float32(F + E)
        d_lo = np.float32(rf.rf_dlo(float(F), dim, float(qn), float(rn)))
        if np.isfinite(U) and np.isfinite(K):
            if not (Fr(float(K)) <= Fr(float(F)) + e_exact):
                bad.append((tag, name, "theorem (a)-(c)", float(K), float(F), float(e_exact)))
            if not (Fr(float(F)) + e_exact <= Fr(float(U))):
                bad.append((tag, name, "f32 margin below the exact bound", float(F), float(e_exact), float(U)))
            if not (K <= U):
                bad.append((tag, name, "K > U", float(K), float(U)))
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
    rng = np.random.default_rng(20261016)
    for dim in (256, 768, 1536):
        # random unit rows, random (not normalised) queries
        for t in range(24):
            bad += _check(rf, O.fill_normal(100 * dim + t, (dim,)), _unit(7 * dim + t, dim), f"random d{dim} #{t}"); n += 1
        # all-same-sign: no cancellation, every error adds up
        for t in range(6):
            x = np.abs(_unit(900 + dim + t, dim)); q = np.abs(O.fill_normal(950 + dim + t, (dim,)))
            bad += _check(rf, q, x, f"same-sign d{dim} #{t}"); bad += _check(rf, -q, x, f"opposite-sign d{dim} #{t}"); n += 2
        # the query's signs follow the shadow's rounding errors: sum q_i (x_i - h_i) is as large as it gets
        for t in range(6):
            x = _unit(1200 + dim + t, dim); e = x.astype(np.float64) - x.astype(np.float16).astype(np.float64)
            q = (np.abs(O.fill_normal(1250 + dim + t, (dim,))) * np.where(e >= 0, 1, -1)).astype(np.float32)
            bad += _check(rf, q, x, f"error-aligned d{dim} #{t}"); n += 1
        # elements ON binary16 rounding midpoints (1 + (2 j + 1) 2^-11) 2^e: the largest relative error, ties to even both ways
        for t in range(4):
            j = rng.integers(0, 1024, dim); e = rng.integers(-9, -3, dim)
            x = ((1.0 + (2 * j + 1) * 2.0 ** -11) * 2.0 ** e).astype(np.float32) * rng.choice([-1, 1], dim).astype(np.float32)
            assert np.all(np.abs(x.astype(np.float64) - x.astype(np.float16).astype(np.float64)) == 2.0 ** (e - 11.0))
            q = np.abs(O.fill_normal(1500 + dim + t, (dim,))) * np.sign(x) * (1 if t % 2 else -1)
            bad += _check(rf, q, x, f"midpoints d{dim} #{t}"); n += 1
        # binary16's subnormal range, exact zeros, and a few ordinary elements
        for t in range(4):
            x = (2.0 ** rng.uniform(-30, -14, dim) * rng.choice([-1, 1], dim)).astype(np.float32)
            x[rng.integers(0, dim, dim // 4)] = 0.0
            if t >= 2:
                x[rng.integers(0, dim, 8)] = rng.uniform(0.1, 0.3, 8).astype(np.float32)
            q = O.fill_normal(1700 + dim + t, (dim,)); q[rng.integers(0, dim, dim // 8)] = 0.0
            bad += _check(rf, q, x, f"subnormal d{dim} #{t}"); n += 1
            bad += _check(rf, np.abs(q) * np.where(x >= 0, 1, -1).astype(np.float32), x, f"subnormal aligned d{dim} #{t}"); n += 1
        # one-hot rows (|x_i| = 1), against a query that is one-hot there too, and a dense one
        for t in range(4):
            x = np.zeros(dim, np.float32); i = int(rng.integers(0, dim)); x[i] = 1.0 if t % 2 else -1.0
            q = np.zeros(dim, np.float32); q[i] = 0.75
            bad += _check(rf, q, x, f"one-hot/one-hot d{dim} #{t}"); bad += _check(rf, O.fill_normal(1900 + dim + t, (dim,)), x, f"one-hot d{dim} #{t}"); n += 2
        # queries far from unit norm (queries are not normalised)
        for t, s in enumerate((1e-6, 1e-3, 37.0, 1e3, 1e6, 1e12)):
            bad += _check(rf, O.fill_normal(2100 + dim + t, (dim,)) * np.float32(s), _unit(2150 + dim + t, dim), f"|q| x{s} d{dim}"); n += 1
        # near-duplicates of the query: the distances the walk's lowerBound lives among
        for t in range(6):
            x = _unit(2300 + dim + t, dim); q = x + O.fill_normal(2350 + dim + t, (dim,)) * np.float32(1e-3 * 4 ** t)
            bad += _check(rf, q, x, f"near d{dim} #{t}"); n += 1
    assert n > 150
    assert not bad, bad[:10]


def test_nothing_is_certified_when_an_input_is_out_of_range(rf):
    """overflowing shadow sums, vanishing or overflowing norms, NaN: d_lo is not finite or the verdict is 'read the f32 row'"""
    inf = float("inf"); nan = float("nan")
    for F, qn, rn in ((inf, 1.0, 1.0), (-inf, 1.0, 1.0), (nan, 1.0, 1.0), (0.5, 0.0, 1.0), (0.5, 1e-20, 1e-20), (0.5, inf, 1.0), (0.5, 1e30, 1e30), (0.5, nan, 1.0), (0.5, 1.0, nan)):
        d = rf.rf_dlo(F, 768, qn, rn)
        for lb in (-1.0, 0.0, 0.5, 2.0):
            assert not rf.rf_rejects(d, lb), (F, qn, rn, d, lb)
    assert not rf.rf_rejects(0.9, nan) and not rf.rf_rejects(0.9, inf) and not rf.rf_rejects(nan, 0.5)
    assert rf.rf_rejects(0.9, 0.5) and rf.rf_rejects(0.5, 0.5) and not rf.rf_rejects(0.4, 0.5)
    # a row element beyond binary16's range becomes an infinity in the shadow: the sum is not finite, nothing is rejected
    x = np.zeros(256, np.float32); x[3] = 1e6; q = np.ones(256, np.float32)
    with np.errstate(over="ignore"):
        F = float(np.sum(q * x.astype(np.float16).astype(np.float32)))
    assert not np.isfinite(F) and not rf.rf_rejects(rf.rf_dlo(F, 256, 256.0, 1e12), 0.1)


def test_the_margin_is_small_enough_to_filter(rf):
    """not a correctness condition — the size the design was reasoned with: E = ~1.0e-3 den for 768-d rows"""
    e = rf.rf_margin(768, 1.0, 1.0, 1.0)
    assert 0.9e-3 < e < 1.2e-3
