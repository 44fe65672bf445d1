// filter_carry.hpp — carrying slot bitmaps through a compaction (coltt_hnsw_compact_carry; include/coltt_gpu.h, "HNSW compaction").
//
// A compaction renumbers the slots by new(s) = live slots below s.  A bitmap over the old slots (a resident filter, the "set" bitmap of an
// attribute column) becomes a bitmap over the new ones by dropping the bits of the tombstoned slots and closing the gaps: per source word w,
// with live = the word's live slots, the bits of the word selected by `live` are packed to the low end (bits_compress, a pext) and land at the
// new bit position rank[w] = live slots below slot 32 w — popc(live) bits that straddle at most two output words.
//   bits_compress          the word function, host and device: the five-round parallel-suffix compress (Hacker's Delight 7-4)
//   carry_bits_host        the definition, host only (coltt_hnsw_carry_bits_host)
//   filter_carry_kernel    workgroup b serves bitmap b / n_wg, OUTPUT tile b % n_wg (FEX_TILE_WORDS words, the tile filter_compact_kernel
//                          shares): it finds its source words from old_of_new at the tile's first and last new slot, streams them coalesced,
//                          ORs each word's one or two pieces into the tile's LDS image (a piece outside the tile belongs to the neighbour,
//                          which reads the same source word), then writes the tile with 16-byte stores and its popcount to counts[p][t].
// No global atomics, no zero-fill pass, no workgroup waits on another; the OR into LDS commutes, so the result does not depend on the order.
// The slot lists of the carried filters are then built by the unchanged filter_compact_kernel from the same counts.
#pragma once
#include "filter_expr.hpp"

namespace coltt {
namespace kern {

// the bits of x selected by m, packed to the low end in their order (pext)
__host__ __device__ __forceinline__ uint32_t bits_compress(uint32_t x, uint32_t m) {
  x &= m;
  uint32_t mk = ~m << 1;   // the bits that have a 0 of m to their right count it
#pragma unroll
  for (int i = 0; i < 5; i++) {
    uint32_t mp = mk ^ (mk << 1);   // parallel suffix: bit j = parity of the zeros of m below j
    mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16;
    const uint32_t mv = mp & m;     // the bits that move by 2^i in this round
    m = (m ^ mv) | (mv >> (1 << i));
    const uint32_t t = x & mv;
    x = (x ^ t) | (t >> (1 << i));
    mk &= ~mp;
  }
  return x;
}

// the live slots of word w on the host: fex_live_word's twin
inline uint32_t carry_live_word_host(const uint32_t* del, uint64_t w, uint64_t n_words, uint64_t n_slots) {
  if (w >= n_words) return 0u;
  uint32_t m = del ? ~del[w] : ~0u;
  if (w == n_words - 1 && (n_slots & 31u)) m &= (1u << (n_slots & 31u)) - 1u;
  return m;
}

// The definition.  bits: n_words words over the old slots (words past it read as 0); del: the tombstones (nullptr: none); out_bits
// [ceil(live / 32)] (may be nullptr); *out_allowed = the bits that survive, *out_live = the live slots (either may be nullptr).
inline void carry_bits_host(const uint32_t* bits, uint64_t n_words, const uint32_t* del, uint64_t n_slots, uint32_t* out_bits,
                            uint64_t* out_allowed, uint64_t* out_live) {
  const uint64_t words = (n_slots + 31) / 32;
  uint64_t live = 0;
  for (uint64_t w = 0; w < words; w++) live += (uint64_t)__builtin_popcount(carry_live_word_host(del, w, words, n_slots));
  if (out_bits) std::fill(out_bits, out_bits + (live + 31) / 32, 0u);
  uint64_t r = 0, allowed = 0;
  for (uint64_t w = 0; w < words; w++) {
    const uint32_t lv = carry_live_word_host(del, w, words, n_slots);
    const uint32_t x = bits_compress(w < n_words ? bits[w] : 0u, lv);
    if (x && out_bits) {
      const uint32_t sh = (uint32_t)(r & 31);
      out_bits[r >> 5] |= x << sh;
      if (sh && (x >> (32 - sh))) out_bits[(r >> 5) + 1] |= x >> (32 - sh);
    }
    allowed += (uint64_t)__builtin_popcount(x);
    r += (uint64_t)__builtin_popcount(lv);
  }
  if (out_allowed) *out_allowed = allowed;
  if (out_live) *out_live = live;
}

// one bitmap of a carry launch: the source as the kernel reads it (words past `words` read as 0) and where its output words go
struct CarryMap { const uint32_t* bits; uint32_t* out; uint32_t words, pad_; };

// Workgroup b: bitmap p = b / n_wg, output words [t * FEX_TILE_WORDS, ...) of it, t = b % n_wg; n_wg = ceil(ceil(live / 32) / FEX_TILE_WORDS), live > 0.
// out_words: the words of an output bitmap's slice, a multiple of 4 (the words between ceil(live / 32) and it are written as 0).
__global__ __launch_bounds__(FEX_THREADS) void filter_carry_kernel(const CarryMap* __restrict__ maps, const uint32_t* __restrict__ del, uint32_t n_slots,
                                                                   uint32_t n_words /* of the old slots */, const uint32_t* __restrict__ rank,
                                                                   const uint32_t* __restrict__ old_of_new, uint32_t live, uint32_t n_wg,
                                                                   uint32_t out_words, uint32_t* __restrict__ counts /* [n_maps][n_wg] */) {
  __shared__ __align__(16) uint32_t img[FEX_TILE_WORDS];
  __shared__ uint32_t wsum[FEX_THREADS / 64];
  const uint32_t p = blockIdx.x / n_wg, t = blockIdx.x - p * n_wg;
#pragma unroll
  for (int j = 0; j < FEX_ITEMS; j++) img[j * FEX_THREADS + threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t ow0 = t * FEX_TILE_WORDS;                                    // the tile's first output word
  const uint32_t j0 = ow0 * 32u, j1 = min(live - j0, FEX_TILE_WORDS * 32u) - 1u + j0;   // its first and last new slot (j0 < live)
  const uint32_t w0 = old_of_new[j0] >> 5, w1 = old_of_new[j1] >> 5;          // the source words that hold them
  const CarryMap M = maps[p];
  for (uint32_t w = w0 + threadIdx.x; w <= w1; w += FEX_THREADS) {
    const uint32_t lv = fex_live_word(del, w, n_words, n_slots);
    if (!lv) continue;
    const uint32_t x = bits_compress(w < M.words ? M.bits[w] : 0u, lv);
    if (!x) continue;
    const uint32_t r = rank[w], sh = r & 31u;
    const uint32_t wi = (r >> 5) - ow0;          // (wraps for a word below the tile: not < FEX_TILE_WORDS)
    if (wi < FEX_TILE_WORDS) atomicOr(&img[wi], x << sh);
    if (sh) {
      const uint32_t hi = x >> (32u - sh), wi1 = wi + 1u;   // (the word below the tile's first: wi1 == 0)
      if (hi && wi1 < FEX_TILE_WORDS) atomicOr(&img[wi1], hi);
    }
  }
  __syncthreads();
  const uint32_t lw = threadIdx.x * 4u;
  const uint4 v = *reinterpret_cast<const uint4*>(&img[lw]);
  if (ow0 + lw < out_words) *reinterpret_cast<uint4*>(M.out + ow0 + lw) = v;
  uint32_t c = (uint32_t)(__popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w));
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

// the words of one output slice for `live` new slots: 256-byte slices, as the outputs of an evaluation
inline size_t carry_stride(uint64_t live) { return (size_t)(((live + 31) / 32 + 63) & ~(uint64_t)63); }
inline uint32_t carry_n_wg(uint64_t live) { return ceil_div((live + 31) / 32, FEX_TILE_WORDS); }

// n_maps bitmaps in one launch (live > 0, n_maps * carry_n_wg(live) within a grid: the callers check)
inline void launch_carry(hipStream_t s, const CarryMap* d_maps, uint32_t n_maps, const uint32_t* d_del, uint32_t n_slots, const uint32_t* d_rank,
                         const uint32_t* d_old_of_new, uint32_t live, uint32_t* d_counts) {
  const uint32_t n_wg = carry_n_wg(live);
  filter_carry_kernel<<<n_maps * n_wg, FEX_THREADS, 0, s>>>(d_maps, d_del, n_slots, (n_slots + 31) / 32, d_rank, d_old_of_new, live, n_wg,
                                                            (uint32_t)carry_stride(live), d_counts);
}

}  // namespace kern
}  // namespace coltt
