// rows8_ingest.hpp — the ingest kernels of the row-filter shadows (rows8.hpp describes the layouts they write): the binary16 shadow rows_h and
// the 8-bit shadow rows_b with its per-row (scale, error norm).  Not templates, so a header of their own that only the translation unit which
// launches them includes (hnsw.hip: prep_rows_any): every other unit that reads the layouts includes rows8.hpp alone and carries no copy.
#pragma once
#include "rows8.hpp"

namespace coltt {
namespace dev {

// n natural-order f32 rows at `rows` (the ingest staging block) -> their shadow at `rows_h`.  One thread per 16-byte destination chunk.
__global__ __launch_bounds__(256) void rows_shadow_kernel(const uint8_t* __restrict__ rows, size_t stride, uint8_t* __restrict__ rows_h, size_t hstride, int dim, uint64_t n) {
  const int chunks = dim >> 3;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * (uint64_t)chunks) return;
  const uint64_t row = t / chunks;
  const int c = (int)(t % chunks), lp = c >> 3, r = c & 7;
  const float* src = reinterpret_cast<const float*>(rows + row * stride);
  unsigned short h[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int l = 2 * lp + (j >> 2), s = j & 3;
    h[j] = __builtin_bit_cast(unsigned short, (_Float16)src[8 * (4 * l + s) + r]);   // fptrunc: round to nearest even, overflow -> infinity
  }
  const u32x4e v = {(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16), (uint32_t)h[4] | ((uint32_t)h[5] << 16),
                    (uint32_t)h[6] | ((uint32_t)h[7] << 16)};
  *reinterpret_cast<u32x4e*>(rows_h + row * hstride + (size_t)c * 16) = v;
}

// n natural-order f32 rows at `rows` (the ingest staging block) -> their codes at `rows_b` and (s, e) at `meta`.  One wave per row.
__global__ __launch_bounds__(256) void rows_b_kernel(const uint8_t* __restrict__ rows, size_t stride, uint8_t* __restrict__ rows_b, size_t bstride,
                                                     RowMeta8* __restrict__ meta, int dim, uint64_t n) {
  const int lane = threadIdx.x & 63;
  const uint64_t row = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;   // (wave-uniform)
  const float* src = reinterpret_cast<const float*>(rows + row * stride);
  float mx = 0.f; bool bad = false;
  for (int i = lane; i < dim; i += 64) { const float a = __builtin_fabsf(src[i]); bad = bad || !(a <= 3.4028234663852886e38f); mx = a > mx ? a : mx; }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const float o = __shfl_xor(mx, m, 64); mx = o > mx ? o : mx; }
  bad = __ballot(bad) != 0ull;
  const float s = bad ? 0.f : (float)((double)mx / 127.0);   // division rounded once (a f64 quotient of two f32 values rounds to f32 innocuously)
  const bool none = !(s > 0.f);                              // zero row, not finite, or a scale that underflows: codes 0, e = +infinity
  double err = 0.0;
  const int chunks = dim >> 4;
  for (int c = lane; c < chunks; c += 64) {
    const int L = c >> 3, r = c & 7;
    uint32_t wds[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      uint32_t wd = 0;
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const float x = src[8 * (4 * (4 * L + j) + t) + r];
        int ci = 0;
        if (!none) {
          float f = __builtin_rintf((float)((double)x / (double)s));
          f = f > 127.f ? 127.f : (f < -127.f ? -127.f : f);
          ci = (int)f;
          const double d = (double)x - (double)s * (double)ci;   // the product is exact in f64
          err += d * d;
        }
        wd |= ((uint32_t)ci & 0xffu) << (8 * t);
      }
      wds[j] = wd;
    }
    *reinterpret_cast<u32x4e*>(rows_b + row * bstride + (size_t)c * 16) = u32x4e{wds[0], wds[1], wds[2], wds[3]};
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) err += __shfl_xor(err, m, 64);
  if (lane == 0) {
    RowMeta8 mt;
    mt.s = none ? 0.f : s;
    const double ev = __builtin_sqrt(err) * (1.0 + 9.5367431640625e-07);   // 1 + 2^-20, then towards +infinity:
    float ef = (float)ev;                                                   // (ev >= 0: the next f32 up is the next bit pattern; an infinity stays)
    if ((double)ef < ev) ef = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, ef) + 1u);
    mt.e = none ? __builtin_inff() : ef;
    meta[row] = mt;
  }
}

}  // namespace dev
}  // namespace coltt
