// attr_filter.hpp — comparison predicates over device-resident attribute columns as leaves of a filter programme
// (coltt_hnsw_attr_* / coltt_hnsw_filter_eval_attr / _eval_attr_batch; include/coltt_gpu.h, "Attribute columns and predicates").
//
// A column is one 8-byte value per slot and a "set" bitmap (hnsw.hip: HnswAttr).  The evaluation keeps the launch shape of filter_expr.hpp:
//   attr_filter_eval_kernel  filter_eval_kernel with one more kind of push: a value v >= n_leaves pushes predicate v - n_leaves.  A thread owns
//                            whole bitmap words, so it cannot read its own 32 values (a 256-byte stride per lane); the wave produces its 64 words
//                            together: 32 coalesced 512-byte loads, a compare and a ballot each, the two owning lanes keep a half of the mask;
//   filter_compact_kernel    reused as it is for the lists.
//   attr_scatter_kernel / attr_gather_kernel   coltt_hnsw_attr_set / _get.
#pragma once
#include "filter_expr.hpp"

namespace coltt {
namespace kern {

// The one comparison (coltt_attr_cmp_host and the kernel): value OP operand, both as the 8 bytes the column stores.  I64 compares as signed
// 64-bit integers, never through a double; F64 as IEEE doubles (-0.0 == +0.0; NaN never reaches here: attr_set and the predicate check refuse it).
__host__ __device__ __forceinline__ bool attr_cmp(int type, int op, uint64_t value, uint64_t operand) {
  if (op == COLTT_CMP_SET) return true;
  if (type == COLTT_ATTR_I64) {
    const long long a = (long long)value, b = (long long)operand;
    switch (op) {
      case COLTT_CMP_EQ: return a == b;
      case COLTT_CMP_NE: return a != b;
      case COLTT_CMP_GT: return a > b;
      case COLTT_CMP_GE: return a >= b;
      case COLTT_CMP_LT: return a < b;
      default: return a <= b;
    }
  }
  double a, b;
  memcpy(&a, &value, 8); memcpy(&b, &operand, 8);
  switch (op) {
    case COLTT_CMP_EQ: return a == b;
    case COLTT_CMP_NE: return a != b;
    case COLTT_CMP_GT: return a > b;
    case COLTT_CMP_GE: return a >= b;
    case COLTT_CMP_LT: return a < b;
    default: return a <= b;
  }
}

inline bool attr_is_nan(uint64_t bits) { return (bits & 0x7ff0000000000000ull) == 0x7ff0000000000000ull && (bits & 0x000fffffffffffffull) != 0; }

// a predicate as the kernel reads it: slots at or past `covered` hold no value
struct AttrPredDev { const uint64_t* vals; const uint32_t* set; uint64_t operand; uint32_t covered; int32_t op_type /* op | type << 8 */; };

// filter_eval_kernel (filter_expr.hpp) with predicate leaves.  Thread i of wave wv owns word t * TILE + j * 256 + wv * 64 + lane in pass j, so a
// wave's words of one pass are 64 consecutive words = 2 048 consecutive slots.  The programme counter is uniform over the launch, so every lane of
// every wave reaches every ballot: no lane returns early, a slot at or past the column's coverage or n_slots contributes 0 through the guarded load.
__global__ __launch_bounds__(FEX_THREADS) void attr_filter_eval_kernel(const FexLeaf* __restrict__ leaves, uint32_t n_leaves,
                                                                       const AttrPredDev* __restrict__ preds, const uint32_t* __restrict__ prog_off,
                                                                       const int32_t* __restrict__ progs, const uint32_t* __restrict__ del,
                                                                       uint32_t n_slots, uint32_t n_words, uint32_t n_wg,
                                                                       uint32_t* __restrict__ out_bits, size_t out_stride /* words */,
                                                                       uint32_t* __restrict__ counts /* [n_out][n_wg] */) {
  __shared__ uint32_t wsum[FEX_THREADS / 64];
  const uint32_t p = blockIdx.x / n_wg, t = blockIdx.x - p * n_wg, lane = threadIdx.x & 63;
  uint32_t w[FEX_ITEMS], live[FEX_ITEMS], st[FEX_MAX_DEPTH][FEX_ITEMS];
#pragma unroll
  for (int j = 0; j < FEX_ITEMS; j++) {
    w[j] = t * FEX_TILE_WORDS + j * FEX_THREADS + threadIdx.x;
    live[j] = fex_live_word(del, w[j], n_words, n_slots);
  }
#pragma unroll
  for (int l = 0; l < FEX_MAX_DEPTH; l++)
#pragma unroll
    for (int j = 0; j < FEX_ITEMS; j++) st[l][j] = 0u;
  const uint32_t pe = prog_off[p + 1];
  for (uint32_t pc = prog_off[p]; pc < pe; pc++) {
    const int32_t op = progs[pc];
    if (op >= 0 || op == COLTT_FOP_ALL) {
      uint32_t v[FEX_ITEMS];
      if (op >= 0 && (uint32_t)op >= n_leaves) {
        const AttrPredDev P = preds[(uint32_t)op - n_leaves];
        const int cmp = P.op_type & 0xff, type = P.op_type >> 8;
        const uint32_t lim = P.covered < n_slots ? P.covered : n_slots, set_words = (lim + 31) / 32;
#pragma unroll
        for (int j = 0; j < FEX_ITEMS; j++) {
          const uint64_t base = (uint64_t)(w[j] - lane) * 32u;   // the first slot of this wave's 64 words of pass j
          uint32_t mine = 0u;
#pragma unroll 8
          for (uint32_t s = 0; s < 32; s++) {
            const uint64_t slot = base + 64u * s + lane;
            const bool hit = slot < lim && attr_cmp(type, cmp, P.vals[slot], P.operand);
            const unsigned long long m = __ballot(hit);           // words 2 s and 2 s + 1 of the wave
            if ((lane >> 1) == s) mine = (lane & 1u) ? (uint32_t)(m >> 32) : (uint32_t)m;
          }
          v[j] = w[j] < set_words ? (mine & P.set[w[j]]) : 0u;
        }
      } else if (op >= 0) {
        const FexLeaf L = leaves[op];
#pragma unroll
        for (int j = 0; j < FEX_ITEMS; j++) v[j] = w[j] < L.words ? L.bits[w[j]] : 0u;
      } else {
#pragma unroll
        for (int j = 0; j < FEX_ITEMS; j++) v[j] = live[j];
      }
#pragma unroll
      for (int l = FEX_MAX_DEPTH - 1; l > 0; l--)
#pragma unroll
        for (int j = 0; j < FEX_ITEMS; j++) st[l][j] = st[l - 1][j];
#pragma unroll
      for (int j = 0; j < FEX_ITEMS; j++) st[0][j] = v[j];
    } else if (op == COLTT_FOP_NOT) {
#pragma unroll
      for (int j = 0; j < FEX_ITEMS; j++) st[0][j] = live[j] & ~st[0][j];
    } else {   // a b -> st[1] op st[0]
#pragma unroll
      for (int j = 0; j < FEX_ITEMS; j++) {
        const uint32_t a = st[1][j], b = st[0][j];
        st[0][j] = op == COLTT_FOP_AND ? (a & b) : op == COLTT_FOP_OR ? (a | b) : (a & ~b);
      }
#pragma unroll
      for (int l = 1; l < FEX_MAX_DEPTH - 1; l++)
#pragma unroll
        for (int j = 0; j < FEX_ITEMS; j++) st[l][j] = st[l + 1][j];
    }
  }
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < FEX_ITEMS; j++) {
    const uint32_t r = st[0][j] & live[j];
    if (w[j] < n_words) out_bits[(size_t)p * out_stride + w[j]] = r;
    c += (uint32_t)__popc(r);
  }
  c = fex_wave_sum(c);
  if (lane == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < FEX_THREADS / 64; i++) s += wsum[i];
    counts[(size_t)p * n_wg + t] = s;
  }
}

// coltt_hnsw_attr_set: vals[slots[i]] = v[i].  The host resolved duplicates, so no two threads write one slot; every slot is below the column's capacity.
__global__ void attr_scatter_kernel(const uint32_t* __restrict__ slots, const uint64_t* __restrict__ v, uint64_t n, uint64_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vals[slots[i]] = v[i];
}

// coltt_hnsw_attr_get: out[i] = the value of slots[i], flag[i] = it has one (a slot of 0xffffffff — an unknown or removed id — or one at or past the coverage has none)
__global__ void attr_gather_kernel(const uint32_t* __restrict__ slots, uint64_t n, const uint64_t* __restrict__ vals, const uint32_t* __restrict__ set,
                                   uint32_t covered, uint64_t* __restrict__ out, uint8_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = slots[i];
  const bool has = s < covered && ((set[s >> 5] >> (s & 31)) & 1u);
  out[i] = has ? vals[s] : 0ull;
  flag[i] = has ? 1 : 0;
}

}  // namespace kern
}  // namespace coltt
