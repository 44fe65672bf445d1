// row_filter8i.hpp — the CERTIFIED margin of the level-0 row filter over the 8-bit shadow with a QUANTISED QUERY ("8i": rows8.hpp: query_digits8i,
// group8_burst_bi / group8_stream_bi; hnsw_walk2.hpp: Group8FilterEval<.., ROW_FILTER_8I>).  Phase A is an exact INTEGER dot product of the row's code
// bytes with two signed digit planes of the query; everything that is approximate sits in this header.  row_filter8.hpp holds the f32-query margin over
// the same shadow, row_filter.hpp the binary16 one; the verdict (row_filter_rejects) and the epilogue are shared.  Plain C++ on purpose (no HIP header):
// tests/test_row_filter8i_bound.py compiles this file with g++ and calls the very code the kernel runs.
//
// The row's quantiser is row_filter8.hpp's: s, codes c_i in [-127, 127], a stored e >= ||x - s c||_2 (or e = +infinity: no certificate).
// The query's quantiser (once per traversal, rows8.hpp: query_digits8i; restated in tests/row_filter8i_ref.py), the functions below in this order:
//   t   = fl(max|q_i| / 16256)                                       row_filter8i_scale   (0: a zero query, a non-finite element, a scale that underflows)
//   qh_i = clamp(rint(fl(q_i / t)), -16256, 16256)                   row_filter8i_level   (an integer)
//   qh_i = 128 h_i + l_i,  h_i in [-127, 127], l_i in [-64, 63]      row_filter8i_digits  (two signed bytes: v_dot4_i32_i8 serves both planes)
//   e_q >= ||q - t qh||_2                                             row_filter8i_err     (the squared differences summed in f64 — t qh_i is exact in f64 —
//                                                                     the root inflated by 1 + 2^-20 and rounded towards +infinity to f32, as the rows' e)
// Nothing below depends on HOW qh was chosen: whatever the levels are — clipped, tied, rounded the other way — e_q measures it.  t = 0 gives
// e_q = +infinity: no certificate, every neighbour goes to the exact evaluation.
//
// Derivation.  u = 2^-24, gamma_k = k u / (1 - k u), x = the stored f32 row, q = the query, n = dim / 8, k = n + 4, P = sum |q_i x_i|, T = sum q_i x_i,
// I = sum qh_i c_i (an integer, computed exactly: |I| <= 8192 * 127 * 16256 < 2^34).
//  (a) the exact kernel returns K with K - T <= gamma_k P <= gamma_k ||q|| ||x||                                  (row_filter8.hpp (a));
//  (b) T = t qh . s c + t qh . (x - s c) + (q - t qh) . x = t s I + R1 + R2 with, by Cauchy-Schwarz and the STORED error norms,
//      R1 <= ||t qh|| ||x - s c|| <= (||q|| + e_q) e      and      R2 <= ||q - t qh|| ||x|| <= e_q ||x||;
//      hence K <= t s I + ||q|| e + e_q e + e_q ||x|| + gamma_k ||q|| ||x||;
//  (c) the norms, as row_filter.hpp (d): the kernel holds SQUARED norms summed in f32; for dim <= 8192: ||q|| ||x|| <= den (1 + 3 dim u) with
//      den = fl(sqrt(fl(qnorm rnorm))), ||q|| <= sqrtf(qnorm) (1 + 2 dim u) and ||x|| <= sqrtf(rnorm) (1 + 2 dim u);
//  (d) underflow, as row_filter8.hpp (e): elements with |q_i| < 2^-60 or |x_i| < 2^-60 are not reliably seen by the squared norms.  They add at most
//      2^-47 (1 + qnorm + rnorm) to P, such q_i at most sqrt(dim) 2^-60 e <= 2^-53 e to ||q|| e and such x_i at most 2^-53 e_q to e_q ||x||.
//      FLOOR = 2^-45 (1 + qnorm + rnorm) + 2^-53 (e + e_q) covers the three and the f32 underflow of V below (at most 2^-149).  nsq below 2^-100, and
//      anything not finite (e and e_q above all), is not certified: NaN is returned (every comparison with it is false, the caller reads the f32 row);
//  (e) what is rounded HERE.  t s is exact in f64 (24 + 24 bits), its product with the integer I (< 2^34, exact in f64) is rounded once (2^-53), the
//      result is rounded to f32 (V, relative u) and U = fl(V + E) is off by at most u |V + E|.  |t s I| = |t qh . s c| <= (||q|| + e_q)(||x|| + e):
//      2.03 u on each of the four products pays for the three.  With gamma_k <= 1.001 k u (k u <= 1e-3):
//      E_thm = C1 den + C2 [sqrtf(qnorm) e + e_q sqrtf(rnorm) + e_q e] + FLOOR,  C1 = (1.002 k u + 2.03 u)(1 + 3 dim u),  C2 = (1 + 2.03 u)(1 + 2 dim u).
//      E itself is formed by about twenty f32 operations on positive terms (relative 2^-24 each, constants included): the code multiplies by 1 + 2^-18,
//      which pays for those and for u E.  (768-d Gaussian rows and queries: e = 7.7e-3 ||x||, e_q = 6e-5 ||q||: E = 7.8e-3 den, against 7.7e-3 with the
//      f32 query.)
//  (f) the epilogue is row_filter8.hpp (g): K <= U gives 1 - div_rn(K, den) >= 1 - div_rn(U, den) = d_lo.  No further slack.
#pragma once
#include <cmath>
#include "row_filter.hpp"

namespace coltt {

constexpr int ROW_FILTER_8I = 80;          // the value of this kind wherever 8 / 16 name the other two (template argument, C-ABI `bits`; the knob spells it "8i")
constexpr int ROW_FILTER8I_QMAX = 16256;   // 127 * 128: the largest level, digits (127, 0)

// t from max|q_i| (bad: some element is not finite); 0 = no certificate
COLTT_RF_HD inline float row_filter8i_scale(float mx, bool bad) {
  const float t = bad ? 0.f : (float)((double)mx / 16256.0);   // division rounded once (a f64 quotient of two f32 values rounds to f32 innocuously)
  return t > 0.f ? t : 0.f;
}
// the level of one element (t > 0)
COLTT_RF_HD inline int row_filter8i_level(float x, float t) {
  float f = rintf((float)((double)x / (double)t));   // the f32 quotient, ties to even
  f = f > 16256.f ? 16256.f : (f < -16256.f ? -16256.f : f);
  return (int)f;
}
// qh = 128 h + l
COLTT_RF_HD inline void row_filter8i_digits(int qh, int& h, int& l) {
  h = (qh + 64) >> 7;   // floor((qh + 64) / 128): -127 .. 127 for |qh| <= 16256
  l = qh - 128 * h;     // -64 .. 63
}
// the stored error norm from the f64 sum of squared differences
COLTT_RF_HD inline float row_filter8i_err(double err) {
  const double ev = sqrt(err) * (1.0 + 9.5367431640625e-07);   // 1 + 2^-20, then towards +infinity:
  float ef = (float)ev;
  if ((double)ef < ev) ef = nextafterf(ef, INFINITY);   // (an infinity stays)
  return ef;
}

// E: dot_exact_f32 <= fl(fl(t s I) + E) whenever everything is finite (see above).  den = (float)sqrt((double)(qnorm * rnorm)), the epilogue's denominator.
COLTT_RF_HD inline float row_filter8i_margin(float e, float eq, int dim, float qnorm, float rnorm, float den) {
  const float u = 5.9604644775390625e-08f;                                  // 2^-24
  const float fd = (float)dim, k = (float)(dim / 8 + 4);
  const float c1 = (1.002f * k * u + 2.03f * u) * (1.0f + 3.0f * fd * u);
  const float c2 = (1.0f + 2.03f * u) * (1.0f + 2.0f * fd * u);
  const float sq = (float)sqrt((double)qnorm), sx = (float)sqrt((double)rnorm);
  const float floor_ = 2.8421709430404007e-14f * (1.0f + qnorm + rnorm) + 1.1102230246251565e-16f * (e + eq);    // 2^-45 (1 + qnorm + rnorm) + 2^-53 (e + e_q)
  return (c1 * den + c2 * (sq * e + eq * sx + eq * e) + floor_) * 1.000003814697265625f;   // 1 + 2^-18
}

// Lower bound on the cosine distance the exact f32 kernel computes for this (query, row), from the integer sum I = sum qh_i c_i, the query's scale t and
// error norm e_q and the row's stored scale s and error norm e; NaN when nothing is certified.
COLTT_RF_HD inline float row_filter8i_dlo(long long I, float t, float eq, float s, float e, int dim, float qnorm, float rnorm) {
  const float nsq = qnorm * rnorm;
  const float den = (float)sqrt((double)nsq);
  const float V = (float)(((double)t * (double)s) * (double)I);
  const float U = V + row_filter8i_margin(e, eq, dim, qnorm, rnorm, den);
  const float d = 1.0f - (float)((double)U / (double)den);
  const bool ok = nsq >= 7.888609052210118e-31f /* 2^-100 */ && nsq <= 3.0e38f && qnorm <= 3.0e38f && rnorm <= 3.0e38f && dim <= ROW_FILTER_MAX_DIM &&
                  e >= 0.0f && e <= 3.0e38f && s > 0.0f && s <= 3.0e38f && eq >= 0.0f && eq <= 3.0e38f && t > 0.0f && t <= 3.0e38f;
  return ok ? d : (float)NAN;
}

}  // namespace coltt
