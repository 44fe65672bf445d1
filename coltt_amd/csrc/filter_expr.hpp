// filter_expr.hpp — filter expressions on the device (coltt_hnsw_filter_eval / _eval_batch / _ids; include/coltt_gpu.h, "Filter expressions").
//
// A filter is a slot bitmap and the ascending list of its set slots (hnsw_index.hpp: HnswFilter).  An expression over resident filters is a
// postfix programme; its result is built here in two launches with one host round trip between them (the counts that size the lists):
//   filter_eval_kernel     one pass over the bitmap words: the stack machine runs per word, the result word is masked with the live slots
//                          and written, every workgroup writes the popcount of its FEX_TILE_WORDS words;
//   filter_compact_kernel  every workgroup sums the popcounts of the workgroups before it (a few hundred values at 10 M slots: no scan
//                          kernel, no atomics, no workgroup waits on another) and writes its slots ascending through wave prefix popcounts;
//   filter_ids_kernel      the read-back of coltt_hnsw_filter_ids: list -> ids.
// A batch of programmes runs in the same two launches: workgroup b serves programme b / n_wg, tile b % n_wg.
#pragma once
#include "common.hpp"

namespace coltt {
namespace kern {

constexpr int FEX_MAX_DEPTH = 8;          // the stack lives in statically indexed registers: 8 levels x FEX_ITEMS words per thread
constexpr size_t FEX_MAX_PROG = 4096;
constexpr int FEX_THREADS = 256, FEX_ITEMS = 4;
constexpr uint32_t FEX_TILE_WORDS = FEX_THREADS * FEX_ITEMS;   // 1024 words = 32 768 slots per workgroup

// The programme rules, with no device (coltt_hnsw_filter_prog_check_host; the evaluation calls that entry point).  why/pos: the first offence.
inline int fex_prog_check(const int32_t* prog, size_t n_prog, size_t n_leaves, uint32_t* out_depth, size_t* pos, const char** why) {
  *pos = 0;
  if (n_prog == 0) { *why = "an empty programme"; return COLTT_E_INVALID; }
  if (n_prog > FEX_MAX_PROG) { *why = "more than 4096 entries"; return COLTT_E_UNSUPPORTED; }
  if (!prog) { *why = "NULL programme"; return COLTT_E_INVALID; }
  uint32_t depth = 0, top = 0;
  for (size_t i = 0; i < n_prog; i++) {
    const int32_t v = prog[i];
    *pos = i;
    if (v >= 0) {
      if ((uint64_t)v >= n_leaves) { *why = "a leaf index past the leaf table"; return COLTT_E_INVALID; }
      depth++;
    } else if (v == COLTT_FOP_ALL) {
      depth++;
    } else if (v == COLTT_FOP_NOT) {
      if (depth < 1) { *why = "stack underflow"; return COLTT_E_INVALID; }
    } else if (v == COLTT_FOP_AND || v == COLTT_FOP_OR || v == COLTT_FOP_ANDNOT) {
      if (depth < 2) { *why = "stack underflow"; return COLTT_E_INVALID; }
      depth--;
    } else {
      *why = "an unknown operator"; return COLTT_E_INVALID;
    }
    if (depth > (uint32_t)FEX_MAX_DEPTH) { *why = "stack depth above 8"; return COLTT_E_UNSUPPORTED; }
    top = std::max(top, depth);
  }
  *pos = n_prog;
  if (depth != 1) { *why = "the programme does not end with exactly one value on the stack"; return COLTT_E_INVALID; }
  if (out_depth) *out_depth = top;
  return COLTT_OK;
}

struct FexLeaf { const uint32_t* bits; uint32_t words, pad_; };   // a leaf as the kernel reads it: words past `words` read as 0

// the live slots of word w: not tombstoned (del == nullptr: nothing was ever removed), below n_slots (the ragged last word)
__device__ __forceinline__ uint32_t fex_live_word(const uint32_t* __restrict__ del, uint32_t w, uint32_t n_words, uint32_t n_slots) {
  if (w >= n_words) return 0u;
  uint32_t m = del ? ~del[w] : ~0u;
  if (w == n_words - 1 && (n_slots & 31u)) m &= (1u << (n_slots & 31u)) - 1u;
  return m;
}

__device__ __forceinline__ uint32_t fex_wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Workgroup b: programme p = b / n_wg over the words [t * FEX_TILE_WORDS, ...) of tile t = b % n_wg; thread i owns the words t * TILE + j * 256 + i.
// The programme counter and the stack pointer are uniform across the launch, so the stack is a shift register of named values: the top is always
// st[0], a push moves every level down by one, a binary operator moves them up — every index is a compile-time constant (no scratch).
__global__ __launch_bounds__(FEX_THREADS) void filter_eval_kernel(const FexLeaf* __restrict__ leaves, const uint32_t* __restrict__ prog_off,
                                                                  const int32_t* __restrict__ progs, const uint32_t* __restrict__ del,
                                                                  uint32_t n_slots, uint32_t n_words, uint32_t n_wg,
                                                                  uint32_t* __restrict__ out_bits, size_t out_stride /* words */,
                                                                  uint32_t* __restrict__ counts /* [n_out][n_wg] */) {
  __shared__ uint32_t wsum[FEX_THREADS / 64];
  const uint32_t p = blockIdx.x / n_wg, t = blockIdx.x - p * n_wg;
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
      if (op >= 0) {
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
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t s = 0;
#pragma unroll
    for (int i = 0; i < FEX_THREADS / 64; i++) s += wsum[i];
    counts[(size_t)p * n_wg + t] = s;
  }
}

// Workgroup b = (programme p, tile t): base = the popcounts of p's tiles before t, then FEX_ITEMS passes of 256 consecutive words — an exclusive prefix
// of the words' popcounts across the workgroup (wave prefix + the waves' totals), every thread writes its word's slots ascending.
__global__ __launch_bounds__(FEX_THREADS) void filter_compact_kernel(const uint32_t* __restrict__ bits, size_t bits_stride /* words */, uint32_t n_words,
                                                                     uint32_t n_wg, const uint32_t* __restrict__ counts,
                                                                     const uint64_t* __restrict__ list_off /* [n_out], entries */,
                                                                     uint32_t* __restrict__ lists) {
  __shared__ uint32_t wsum[FEX_THREADS / 64];
  __shared__ uint32_t tot[FEX_THREADS / 64];
  const uint32_t p = blockIdx.x / n_wg, t = blockIdx.x - p * n_wg, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t pre = 0;
  for (uint32_t i = threadIdx.x; i < t; i += FEX_THREADS) pre += counts[(size_t)p * n_wg + i];
  pre = fex_wave_sum(pre);
  if (lane == 0) wsum[wv] = pre;
  __syncthreads();
  uint32_t base = 0;
#pragma unroll
  for (int i = 0; i < FEX_THREADS / 64; i++) base += wsum[i];
  uint32_t* const out = lists + list_off[p];
#pragma unroll
  for (int j = 0; j < FEX_ITEMS; j++) {
    const uint32_t w = t * FEX_TILE_WORDS + j * FEX_THREADS + threadIdx.x;
    uint32_t b = w < n_words ? bits[(size_t)p * bits_stride + w] : 0u;
    const uint32_t c = (uint32_t)__popc(b);
    uint32_t inc = c;   // inclusive prefix over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(inc, o, 64);
      if (lane >= (uint32_t)o) inc += u;
    }
    if (lane == 63) tot[wv] = inc;
    __syncthreads();
    uint32_t at = base + inc - c;
#pragma unroll
    for (int i = 0; i < FEX_THREADS / 64; i++) {
      if ((uint32_t)i < wv) at += tot[i];
      base += tot[i];
    }
    for (; b; b &= b - 1) out[at++] = w * 32u + (uint32_t)__builtin_ctz(b);
    __syncthreads();   // tot is rewritten by the next pass
  }
}

// coltt_hnsw_filter_ids: out[i] = the id of slot list[i] (ids == nullptr: dense ids, id = base + slot)
__global__ void filter_ids_kernel(const uint32_t* __restrict__ list, uint64_t n, const uint64_t* __restrict__ ids, uint64_t base,
                                  uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t s = list[i];
  out[i] = ids ? ids[s] : base + s;
}

}  // namespace kern
}  // namespace coltt
