// row_filter.hpp — the CERTIFIED margin of the level-0 row filter (hnsw_walk2.hpp: Group8FilterEval; rows8.hpp: the binary16 shadow rows_h).
//
// Once the result set of a traversal is full, a fresh neighbour with d >= lowerBound is marked, counted and never looked at again: the walk needs a
// PROOF of d >= lowerBound, not d.  The filter reads the row's binary16 shadow (half the bytes), sums F = sum q_i * h_i in f32 and turns it into a
// lower bound d_lo on the distance the exact kernel WOULD produce; the f32 row is read only when d_lo < lowerBound (or anything is not finite).
// Plain C++ on purpose (no HIP header): the host (tests/test_row_filter_bound.py compiles this file with g++) calls the very code the kernel runs.
//
// Derivation.  u = 2^-24, gamma_k = k u / (1 - k u), x = the stored f32 row, h_i = binary16(x_i) (round to nearest even), q = the query,
// P = sum |q_i x_i|, T = sum q_i x_i, T_h = sum q_i h_i (real numbers), n = dim / 8, k = n + 4.
//  (a) the exact kernel (rows8.hpp: 8 partial sums of n products, multiply and add rounded separately, 3-level tree) returns K with
//      |K - T| <= gamma_{n+3} P <= gamma_k P                               (n - 1 additions behind the first, 1 multiplication, 3 tree levels);
//  (b) the filter's own sum (8 partial sums of n products in any order, fused or not, the same tree) returns F with |F - T_h| <= gamma_k sum |q_i h_i|;
//  (c) |x_i - h_i| <= 2^-11 |x_i| in binary16's normal range and <= 2^-25 below it (half an ulp of a subnormal), so
//      |T - T_h| <= 2^-11 P + 2^-25 ||q||_1      and      sum |q_i h_i| <= (1 + 2^-11) P + 2^-25 ||q||_1
//      (|x_i| >= 65520 becomes an infinity: F is then infinite or NaN, d_lo not finite, and the caller reads the f32 row);
//  hence  K - F <= [2^-11 + (2 + 2^-11) gamma_k] P + (1 + gamma_k) 2^-25 ||q||_1.
//  (d) P <= ||q|| ||x|| (Cauchy-Schwarz) and ||q||_1 <= sqrt(dim) ||q||.  The kernel holds SQUARED norms summed in f32 (qnorm, rnorm: at most dim
//      rounded operations each, all terms non-negative): ||q||^2 <= qnorm / (1 - gamma_dim), the same for x, and the epilogue's own denominator
//      den = fl(sqrt(fl(qnorm * rnorm))) >= sqrt(qnorm rnorm) (1 - u)^(3/2).  For dim <= 8192: ||q|| ||x|| <= den (1 + 3 dim u), ||q|| <= sqrtf(qnorm) (1 + 2 dim u).
//  (e) underflow: elements with |q_i| < 2^-60 or |x_i| < 2^-60 are not reliably seen by the squared norms, and their products may round to subnormals.
//      Together they contribute at most dim * 2^-60 * (max|q_i| + max|x_i|) <= 2^-47 (1 + qnorm + rnorm) to P and far less in rounding: the FLOOR term.
//      All other squares and products are normal numbers (>= 2^-120), so (a)-(d) hold for them as written.  nsq below 2^-100, and anything
//      not finite, is not certified (NaN is returned: every comparison with it is false, the caller reads the f32 row).
//  With gamma_k <= 1.001 k u (k u <= 1e-3):
//      E_thm = C1 den + C2 sqrtf(qnorm) + FLOOR,   C1 = (2^-11 + 2.004 k u)(1 + 3 dim u),   C2 = 1.002 * 2^-25 sqrt(dim) (1 + 2 dim u).
//  The code uses E = 2 * E_thm.  The spare E_thm >= 2^-11 den pays for everything that is rounded here: the handful of f32 operations that
//  form E (relative 2^-24 each) and the final addition U = fl(F + E) (|F + E| <= 1.01 den + E, so at most 2^-24 * 1.01 den + 2^-24 E off).
//  (768-d rows: E = 1.0e-3 den; a CPU walk of the headline shape left 0.13 % of the rejected evaluations unproven at E_thm, the factor 2 costs a few more.)
//  (f) the epilogue (exact.hpp: cos_epilogue) is |1 - div_rn(K, den)| with den > 0; div_rn and the f32 subtraction are correctly rounded, hence
//      monotone: K <= U gives 1 - div_rn(K, den) >= 1 - div_rn(U, den) = d_lo, and |1 - c| >= 1 - c.  No further slack.
#pragma once
#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COLTT_RF_HD __host__ __device__
#else
#define COLTT_RF_HD
#endif

namespace coltt {

constexpr int ROW_FILTER_MAX_DIM = 8192;

// E: dot_exact_f32 <= fl(F + E) whenever the result is finite (see above).  den = (float)sqrt((double)(qnorm * rnorm)), the epilogue's denominator.
COLTT_RF_HD inline float row_filter_margin(int dim, float qnorm, float rnorm, float den) {
  const float u = 5.9604644775390625e-08f;                                  // 2^-24
  const float fd = (float)dim, k = (float)(dim / 8 + 4);
  const float c1 = (4.8828125e-04f + 2.004f * k * u) * (1.0f + 3.0f * fd * u);                                  // 2^-11 + ...
  const float c2 = 1.002f * 2.98023223876953125e-08f * (float)sqrt((double)fd) * (1.0f + 2.0f * fd * u);        // 2^-25 sqrt(dim) ...
  const float floor_ = 7.105427357601002e-15f * (1.0f + qnorm + rnorm);                                         // 2^-47 (1 + qnorm + rnorm)
  return 2.0f * (c1 * den + c2 * (float)sqrt((double)qnorm) + floor_);
}

// Lower bound on the cosine distance the exact f32 kernel computes for this (query, row), from the shadow sum F; NaN when nothing is certified.
COLTT_RF_HD inline float row_filter_dlo(float F, int dim, float qnorm, float rnorm) {
  const float nsq = qnorm * rnorm;
  const float den = (float)sqrt((double)nsq);
  const float U = F + row_filter_margin(dim, qnorm, rnorm, den);
  const float d = 1.0f - (float)((double)U / (double)den);
  const bool ok = nsq >= 7.888609052210118e-31f /* 2^-100 */ && nsq <= 3.0e38f && qnorm <= 3.0e38f && rnorm <= 3.0e38f && dim <= ROW_FILTER_MAX_DIM;
  return ok ? d : (float)NAN;
}

// the filter's verdict: true = the exact kernel's distance is certainly >= lower_bound
COLTT_RF_HD inline bool row_filter_rejects(float d_lo, float lower_bound) {
  const float big = 3.0e38f;
  return d_lo >= lower_bound && d_lo <= big && d_lo >= -big && lower_bound <= big && lower_bound >= -big;
}

}  // namespace coltt
