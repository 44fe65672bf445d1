// row_filter8.hpp — the CERTIFIED margin of the level-0 row filter over the 8-BIT shadow (rows8.hpp: rows_b, one signed code byte per stored f32 element,
// a scale s and an error norm e per row; hnsw_walk2.hpp: Group8FilterEval<.., 8>).  row_filter.hpp holds the binary16 shadow's margin; the verdict
// (row_filter_rejects) and the epilogue are shared.  Plain C++ on purpose (no HIP header): tests/test_row_filter8_bound.py compiles this file with g++ and
// calls the very code the kernel runs.
//
// The quantiser (rows8_ingest.hpp: rows_b_kernel; restated in the tests): s = fl(max|x_i| / 127), c_i = clamp(rint(fl(x_i / s)), -127, 127) (an integer, stored
// signed), e >= ||x - s c||_2: the squared differences summed in f64, the root inflated by 1 + 2^-20 (the f64 roundings: (dim + 4) 2^-53) and rounded
// towards +infinity to f32.  Nothing below depends on HOW c was chosen: whatever the codes are — clipped, tied, rounded the other way — e measures it.
// A zero row, a row with a non-finite element and a row whose scale underflows to 0 get e = +infinity: no certificate.
//
// Derivation.  u = 2^-24, gamma_k = k u / (1 - k u), x = the stored f32 row, q = the query, n = dim / 8, k = n + 4,
// P = sum |q_i x_i|, T = sum q_i x_i, S = sum q_i c_i, T^ = s S (real numbers), G = the filter's f32 sum of q_i * (float)c_i.
//  (a) the exact kernel (rows8.hpp: 8 partial sums of n products, multiply and add rounded separately, 3-level tree) returns K with
//      K - T <= gamma_{n+3} P <= gamma_k P <= gamma_k ||q|| ||x||                                              (Cauchy-Schwarz);
//  (b) T - T^ = sum q_i (x_i - s c_i) <= ||q|| ||x - s c|| <= ||q|| e                                           (Cauchy-Schwarz with the STORED e);
//  (c) the filter's own sum (8 partial sums of n products in any order, fused or not, the same tree; (float)c_i is exact):
//      |G - S| <= gamma_k sum |q_i c_i|, and s sum |q_i c_i| = sum |q_i| |s c_i| <= ||q|| ||s c|| <= ||q|| (||x|| + e), so
//      |s G - T^| <= gamma_k ||q|| (||x|| + e)   and   |s G| <= (1 + gamma_k) ||q|| (||x|| + e);
//      the one rounding of the product: |fl(s G) - s G| <= u |s G|.
//  Together, with V = fl(s G):   K <= V + [2 gamma_k + u (1 + gamma_k)] ||q|| ||x|| + [1 + gamma_k + u (1 + gamma_k)] ||q|| e.
//  (d) as in row_filter.hpp: the kernel holds SQUARED norms summed in f32; for dim <= 8192: ||q|| ||x|| <= den (1 + 3 dim u) with
//      den = fl(sqrt(fl(qnorm rnorm))), and ||q|| <= sqrtf(qnorm) (1 + 2 dim u).
//  (e) underflow, as in row_filter.hpp: elements with |q_i| < 2^-60 or |x_i| < 2^-60 are not reliably seen by the squared norms.  They add at most
//      dim 2^-60 (max|q_i| + max|x_i|) <= 2^-47 (1 + qnorm + rnorm) to P, and such q_i add at most sqrt(dim) 2^-60 e <= 2^-53 e to ||q|| e.
//      A product q_i c_i of such a q_i may be subnormal: an absolute error <= 2^-150 each, times s <= 2^58 (rnorm <= 3e38): below 2^-78 in all.
//      FLOOR = 2^-45 (1 + qnorm + rnorm) + 2^-53 e covers the three.  nsq below 2^-100, and anything not finite (e above all), is not certified:
//      NaN is returned (every comparison with it is false, the caller reads the f32 row).
//  (f) what is rounded HERE.  With gamma_k <= 1.001 k u (k u <= 1e-3):
//      E_thm = C1 den + C2 sqrtf(qnorm) e + FLOOR,   C1 = (2.004 k u + 1.01 u)(1 + 3 dim u),   C2 = (1 + 1.002 k u + 1.01 u)(1 + 2 dim u).
//      The final addition U = fl(V + E) is off by at most u |V + E|, and |V| <= 1.01 (||q|| ||x|| + ||q|| e): 1.02 u more on C1 and on C2 and u E.
//      E itself is formed by about a dozen f32 operations on positive terms (relative 2^-24 each, constants included): the code multiplies by 1 + 2^-18,
//      which pays for those and for u E.  No factor 2 as in the binary16 margin: the term C2 sqrtf(qnorm) e IS the margin (768-d Gaussian rows:
//      e = 0.0076 ||x||, E = 7.7e-3 den), doubling it would double the survivors' band.
//  (g) the epilogue (exact.hpp: cos_epilogue) is |1 - div_rn(K, den)| with den > 0; div_rn and the f32 subtraction are correctly rounded, hence
//      monotone: K <= U gives 1 - div_rn(K, den) >= 1 - div_rn(U, den) = d_lo, and |1 - c| >= 1 - c.  No further slack.
#pragma once
#include <cmath>
#include "row_filter.hpp"

namespace coltt {

// E: dot_exact_f32 <= fl(fl(s G) + E) whenever everything is finite (see above).  den = (float)sqrt((double)(qnorm * rnorm)), the epilogue's denominator.
COLTT_RF_HD inline float row_filter8_margin(float e, int dim, float qnorm, float rnorm, float den) {
  const float u = 5.9604644775390625e-08f;                                  // 2^-24
  const float fd = (float)dim, k = (float)(dim / 8 + 4);
  const float c1 = (2.004f * k * u + 2.03f * u) * (1.0f + 3.0f * fd * u);
  const float c2 = (1.0f + 1.002f * k * u + 2.03f * u) * (1.0f + 2.0f * fd * u);
  const float floor_ = 2.8421709430404007e-14f * (1.0f + qnorm + rnorm) + 1.1102230246251565e-16f * e;    // 2^-45 (1 + qnorm + rnorm) + 2^-53 e
  return (c1 * den + c2 * ((float)sqrt((double)qnorm) * e) + floor_) * 1.000003814697265625f;   // 1 + 2^-18
}

// Lower bound on the cosine distance the exact f32 kernel computes for this (query, row), from the shadow sum G = sum q_i * (float)c_i and the row's
// stored scale s and error norm e; NaN when nothing is certified.
COLTT_RF_HD inline float row_filter8_dlo(float G, float s, float e, int dim, float qnorm, float rnorm) {
  const float nsq = qnorm * rnorm;
  const float den = (float)sqrt((double)nsq);
  const float U = s * G + row_filter8_margin(e, dim, qnorm, rnorm, den);
  const float d = 1.0f - (float)((double)U / (double)den);
  const bool ok = nsq >= 7.888609052210118e-31f /* 2^-100 */ && nsq <= 3.0e38f && qnorm <= 3.0e38f && rnorm <= 3.0e38f && dim <= ROW_FILTER_MAX_DIM &&
                  e >= 0.0f && e <= 3.0e38f && s > 0.0f && s <= 3.0e38f;
  return ok ? d : (float)NAN;
}

}  // namespace coltt
