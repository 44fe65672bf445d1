// hnsw_kernels.hpp — the search kernels of hnsw.hip (Hnsw.Search, core/vectorindex/hnsw.go:243-278): the one-wave walk, the large-ef walk,
// the single-query latency kernel, the walk over product-quantiser codes with its exact re-rank.  A header of their own so that a scratch
// translation unit can instantiate a handful of them for ISA inspection (tools/isa/walks.hip, tools/isa_loops.py) in seconds instead of the
// whole of hnsw.hip.  Included by hnsw.hip inside its anonymous namespace users; nothing here is host code.
#pragma once
#include "common.hpp"
#include "exact.hpp"
#include "hnsw_dev.hpp"
#include "hnsw_walk2.hpp"
#include "hnsw_lat.hpp"
#include "hnsw_pq.hpp"

namespace coltt {
namespace kern {
using namespace coltt::dev;

// Hnsw.Search (hnsw.go:243-278) for a batch: one wave per query, queries pulled from a global counter.  The body of hnsw_search_kernel and
// hnsw_search_filtered_kernel.  FILTER (coltt_hnsw_search_filtered, WALK): the same walk, plus the allowed set R (hnsw_dev.hpp: FiltSet) of
// k_pad = k rounded up to 64 entries in LDS between the result set and the visited hash; the answer is R instead of the walk's k nearest.
// PERQ (coltt_hnsw_search_filtered_batch, with FILTER): the claimed index selects a descriptor fq[qi] (hnsw_dev.hpp: FiltQuery) that
// gives the query's filter, ef, LDS geometry and batch row; ef / ef_pad / hcap / fv are then ignored.
template <int METRIC, int QUANT, bool VISG, bool R8, bool FILTER, bool PERQ = false>
__device__ __forceinline__ void search_one_wave(uint8_t* smem, GraphView g, int32_t entry, int32_t entry_level,
                                                const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                uint32_t nq, uint32_t k, uint32_t ef, uint32_t ef_pad, uint32_t hcap,
                                                uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                size_t vis_stride, uint32_t* __restrict__ vis_epoch, FilterView fv,
                                                const FiltQuery* __restrict__ fq = nullptr) {
  constexpr int PROF = VISG ? PROF_SEARCH_HBM : PROF_SEARCH_LDS;
  const int lane = threadIdx.x;
  WaveCtx w;
  size_t off = ((size_t)g.dim * 4 + 15) & ~(size_t)15;
  w.qs = reinterpret_cast<float*>(smem);
  w.res0 = reinterpret_cast<unsigned long long*>(smem + off);
  FiltSet fs;
  uint32_t k_pad = 0;
  if constexpr (FILTER) { k_pad = (k + 63) & ~63u; fs.r = w.res0 + (size_t)ef_pad; fs.len = 0; fs.cap = k; fs.f = fv; }
  w.vis = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad + k_pad);
  w.ef_pad = ef_pad; w.hcap = hcap; w.hcap_mask = hcap - 1;
  w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0;
  if constexpr (VISG) { w.visg = visg + (size_t)blockIdx.x * vis_stride; w.vis_bytes = vis_stride; w.epoch = vis_epoch[blockIdx.x]; }
  for (;;) {
    // dynamic work fetch.  Branch-free on purpose: with `if (lane == 0) t = atomicAdd(..)` hipcc threads the
    // loop-invariant divergent branch through the back edge, lanes 1..63 re-enter the loop without lane 0 and the
    // cross-lane broadcast below reads a stale value forever.
    const uint32_t qt = atomicAdd(counter, lane == 0 ? 1u : 0u);
    const uint32_t qi = (uint32_t)__shfl((int)qt, 0, 64);
    if (qi >= nq) break;
    uint32_t row = qi;
    if constexpr (PERQ) {   // the descriptor is wave-uniform: its words go to scalar registers
      const uint32_t* dw = reinterpret_cast<const uint32_t*>(fq + qi);
      auto rf = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)dw[i]); };
      fs.f = FilterView{reinterpret_cast<const uint32_t*>(((uint64_t)rf(1) << 32) | rf(0)), rf(2)};
      ef = rf(3); ef_pad = rf(4); hcap = rf(5); row = rf(6);
      fs.r = w.res0 + (size_t)ef_pad;
      w.vis = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad + k_pad);
      w.ef_pad = ef_pad; w.hcap = hcap; w.hcap_mask = hcap - 1;
    }
    w.n_dist = w.n_exp = w.n_hops = w.n_resets = 0; w.err = 0;
#ifdef COLTT_PHASE_TIMING
    for (int i_ = 0; i_ < 8; i_++) w.pt[i_] = 0;
    w.t_last = __builtin_amdgcn_s_memtime();
#endif
    wave_sync();
    for (int e = lane; e < g.dim; e += 64) w.qs[e] = q_eff[(size_t)row * g.dim + e];
    w.qnorm = qnorms[row];
    wave_sync();
    // minDistance := Distance(query, entrypoint.vector) (hnsw.go:253)
    uint32_t cur = (uint32_t)entry;
    float curd = eval_pair<METRIC, QUANT, PROF, R8>(g, w, cur, lane & 1);
    curd = __shfl(curd, 0, 64);
    w.n_dist += 1;
    for (int l = entry_level; l > 0; l--) greedy_level<METRIC, QUANT, PROF, R8>(g, w, cur, curd, l, lane);  // :254-256
    COLTT_PT(w, 5)  // query load + entry distance + upper levels
    // searchLevel re-evaluates the entrypoint distance (hnsw.go:346)
    w.n_dist += 1;
    uint32_t len; int buf;
    search_level<METRIC, QUANT, VISG, PROF, R8, FILTER>(g, w, cur, curd, ef, 0, lane, len, buf, &fs);  // :258-259
    // selectNeighbors + pop into result[n-1..0] (:261-277) == the k smallest, ascending
    uint32_t n = len < k ? len : k;
    const unsigned long long* res = w.res0 + (size_t)buf * ef_pad;
    if constexpr (FILTER) { n = fs.len; res = fs.r; }   // filtered: R, ascending
    for (uint32_t i = lane; i < n; i += 64) {
      unsigned long long e = res[i];
      uint32_t slot = (uint32_t)e >> 1;
      out_ids[(size_t)row * k + i] = g.ids ? g.ids[slot] : (uint64_t)slot;
      out_scores[(size_t)row * k + i] = __uint_as_float((uint32_t)(e >> 32));
    }
    if (lane == 0) {
      out_counts[row] = n;
      atomicAdd(&stats[0], (unsigned long long)w.n_dist);
      atomicAdd(&stats[1], (unsigned long long)w.n_exp);
      atomicAdd(&stats[2], (unsigned long long)w.n_hops);
      atomicAdd(&stats[3], (unsigned long long)w.n_resets);
      if (w.err) atomicOr(&stats[4], (unsigned long long)w.err);
#ifdef COLTT_PHASE_TIMING
      COLTT_PT(w, 6)  // result write-out
      for (int i_ = 0; i_ < 8; i_++) atomicAdd(&stats[8 + i_], w.pt[i_]);
#endif
    }
  }
  if constexpr (VISG) { if (lane == 0) vis_epoch[blockIdx.x] = w.epoch; }
}
template <int METRIC, int QUANT, bool VISG, bool R8 = false>   // R8: the index's ONE row array is line-transposed (rows8.hpp)
__global__ __launch_bounds__(64) void hnsw_search_kernel(GraphView g, int32_t entry, int32_t entry_level,
                                                        const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                        uint32_t nq, uint32_t k, uint32_t ef, uint32_t ef_pad, uint32_t hcap,
                                                        uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                        float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                        unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                        size_t vis_stride, uint32_t* __restrict__ vis_epoch) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  search_one_wave<METRIC, QUANT, VISG, R8, false>(smem, g, entry, entry_level, q_eff, qnorms, nq, k, ef, ef_pad, hcap, counter, out_ids, out_scores,
                                                  out_counts, stats, visg, vis_stride, vis_epoch, FilterView{nullptr, 0u});
}
// coltt_hnsw_search_filtered, WALK: the one-wave walk with the allowed set (its own instances: the unfiltered ones stay as they are)
template <int METRIC, int QUANT, bool VISG, bool R8 = false>
__global__ __launch_bounds__(64) void hnsw_search_filtered_kernel(GraphView g, int32_t entry, int32_t entry_level,
                                                                 const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                                 uint32_t nq, uint32_t k, uint32_t ef, uint32_t ef_pad, uint32_t hcap,
                                                                 uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                                 float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                                 unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                                 size_t vis_stride, uint32_t* __restrict__ vis_epoch, FilterView fv) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  search_one_wave<METRIC, QUANT, VISG, R8, true>(smem, g, entry, entry_level, q_eff, qnorms, nq, k, ef, ef_pad, hcap, counter, out_ids, out_scores,
                                                 out_counts, stats, visg, vis_stride, vis_epoch, fv);
}

// coltt_hnsw_search_filtered_batch, WALK: the same walk with one filter, breadth and LDS geometry per query (fq[0..nq)); the launch's
// dynamic LDS is the largest of its queries'.  A third instance family: the two above stay as they are.
template <int METRIC, int QUANT, bool VISG, bool R8 = false>
__global__ __launch_bounds__(64) void hnsw_search_filtered_batch_kernel(GraphView g, int32_t entry, int32_t entry_level,
                                                                       const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                                       uint32_t nq, uint32_t k, const FiltQuery* __restrict__ fq,
                                                                       uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                                       float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                                       unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                                       size_t vis_stride, uint32_t* __restrict__ vis_epoch) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  search_one_wave<METRIC, QUANT, VISG, R8, true, true>(smem, g, entry, entry_level, q_eff, qnorms, nq, k, 0u, 0u, 64u, counter, out_ids, out_scores,
                                                       out_counts, stats, visg, vis_stride, vis_epoch, FilterView{nullptr, 0u}, fq);
}


// Hnsw.Search for large ef (HBM visited map): the level-0 walk of hnsw_walk2.hpp — delta result set, LDS Bloom filter in front
// of the byte map, neighbour norms riding with the adjacency rows (OPT bits) — at two register/occupancy profiles.
// EV8: the level-0 distances come from the eight-lanes-per-row core over GraphView::rows8 (rows8.hpp); the upper levels and the
// entrypoint (a few dozen evaluations) stay on the pair-owned rows.
template <int METRIC, int QUANT, int PROFILE, int OPT, int VISMODE = VIS_HBM, bool APREF = false, bool EV8 = false, bool R8 = false, bool NT = false>   // NT (EV8 only): non-temporal row loads, for collections far larger than the caches (exact.hpp: row_ld); APREF: adjacency prefetch for f32 rows too (small batches); R8 (without EV8): the pair-owned core over line-transposed rows
#ifndef COLTT_OP_WAVES_PER_EU   // experiment knob: minimum waves per SIMD the register allocator must leave room for in the HBM-visited eight-lane 2-byte walk (the operating point)
#define COLTT_OP_WAVES_PER_EU 1
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu((EV8 && QUANT != Q_NONE && VISMODE == VIS_HBM) ? COLTT_OP_WAVES_PER_EU : 1)))
void hnsw_search2_kernel(GraphView g, int32_t entry, int32_t entry_level,
                                                         const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                         uint32_t nq, uint32_t k, uint32_t ef, uint32_t ef_pad, uint32_t bloom_words,
                                                         uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                         float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                         unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                         size_t vis_stride, uint32_t* __restrict__ vis_epoch) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x;
  WaveCtx w;
  size_t off = ((size_t)g.dim * 4 + 15) & ~(size_t)15;
  w.qs = reinterpret_cast<float*>(smem);
  w.qp = nullptr; w.scr = nullptr;
  if constexpr (EV8) {   // [query in rows8 order | scratch] then the result set (plan_search adds the same bytes); no natural-order copy
    w.qp = w.qs; w.qs = nullptr;
    w.scr = reinterpret_cast<uint32_t*>(smem + off);
    off += 96 * 4;
  }
  w.res0 = reinterpret_cast<unsigned long long*>(smem + off);
  w.ef_pad = ef_pad;
  if constexpr (VISMODE == VIS_LDS) {   // small ef: the LDS hash (bloom_words carries its capacity); a table that fills up is err 8
    w.vis = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad);
    w.hcap = bloom_words; w.hcap_mask = bloom_words - 1;
    w.bloom = nullptr; w.bloom_words = 0; w.bloom_shift = 0;
    w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0;
  } else {
    w.vis = nullptr;
    w.bloom = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad);
    w.bloom_words = bloom_words; w.bloom_shift = 32u - (uint32_t)__builtin_ctz(bloom_words | 0x80000000u);
    w.hcap = 0; w.hcap_mask = 0;
    w.visg = visg + (size_t)blockIdx.x * vis_stride; w.vis_bytes = vis_stride; w.epoch = vis_epoch[blockIdx.x];
  }
  for (;;) {
    const uint32_t qt = atomicAdd(counter, lane == 0 ? 1u : 0u);  // branch-free work fetch, see hnsw_search_kernel
    const uint32_t qi = (uint32_t)__shfl((int)qt, 0, 64);
    if (qi >= nq) break;
    w.n_dist = w.n_exp = w.n_hops = w.n_resets = 0; w.err = 0;
#ifdef COLTT_PHASE_TIMING
    for (int i_ = 0; i_ < 8; i_++) w.pt[i_] = 0;
    w.t_last = __builtin_amdgcn_s_memtime();
#endif
    wave_sync();
    for (int e = lane; e < g.dim; e += 64) {
      const float v = q_eff[(size_t)qi * g.dim + e];
      if constexpr (EV8) w.qp[rows8_qindex<QUANT>(e)] = v; else w.qs[e] = v;
    }
    w.qnorm = qnorms[qi];
    wave_sync();
    uint32_t cur = (uint32_t)entry;
    float curd;
    constexpr bool H16 = EV8 && QUANT != Q_NONE && VISMODE == VIS_HBM;   // Group8Eval: rows x burst depth of the HBM-visited 2-byte kernels
    if constexpr (EV8) curd = Group8Eval<METRIC, QUANT, false, H16, NT>().one(g, w, cur, lane);
    else curd = eval_pair<METRIC, QUANT, PROFILE, R8>(g, w, cur, lane & 1);  // hnsw.go:253
    curd = __shfl(curd, 0, 64);
    w.n_dist += 1;
    for (int l = entry_level; l > 0; l--) {  // :254-256
      if constexpr (EV8) greedy_level8<METRIC, QUANT, H16, NT>(g, w, cur, curd, l, lane);
      else greedy_level<METRIC, QUANT, PROFILE, R8>(g, w, cur, curd, l, lane);
    }
    COLTT_PT(w, 5)
    w.n_dist += 1;  // searchLevel re-evaluates the entrypoint distance (hnsw.go:346)
    uint32_t len;
    if constexpr (EV8) search_level2<METRIC, QUANT, PROFILE, OPT, VISMODE, APREF>(g, w, cur, curd, ef, lane, len, Group8Eval<METRIC, QUANT, (OPT & W2_ADJN) != 0 && METRIC == M_COS, H16, NT>());
    else search_level2<METRIC, QUANT, PROFILE, OPT, VISMODE, APREF>(g, w, cur, curd, ef, lane, len, PairEval<METRIC, QUANT, PROFILE, (OPT & W2_ADJN) != 0 && METRIC == M_COS, R8>());  // :258-259
    const uint32_t n = len < k ? len : k;  // selectNeighbors + pop (:261-277) == the k smallest, ascending
    for (uint32_t i = lane; i < n; i += 64) {
      const unsigned long long e = w.res0[i];
      const uint32_t slot = (uint32_t)e >> 1;
      out_ids[(size_t)qi * k + i] = g.ids ? g.ids[slot] : (uint64_t)slot;
      out_scores[(size_t)qi * k + i] = __uint_as_float((uint32_t)(e >> 32));
    }
    if (lane == 0) {
      out_counts[qi] = n;
      atomicAdd(&stats[0], (unsigned long long)w.n_dist);
      atomicAdd(&stats[1], (unsigned long long)w.n_exp);
      atomicAdd(&stats[2], (unsigned long long)w.n_hops);
      if (w.err) atomicOr(&stats[4], (unsigned long long)w.err);
#ifdef COLTT_PHASE_TIMING
      COLTT_PT(w, 6)
      for (int i_ = 0; i_ < 8; i_++) atomicAdd(&stats[8 + i_], w.pt[i_]);
#endif
    }
  }
  if constexpr (VISMODE == VIS_HBM) { if (lane == 0) vis_epoch[blockIdx.x] = w.epoch; }
}

// The ROW-FILTER twin of the eight-lane f32 cosine instances above (COLTT_ROW_FILTER; hnsw.hip: row_filter_on).  A kernel of its own, so that the instances
// above stay, instruction for instruction, what they were: the same prologue (query in rows8 order, entrypoint, upper levels through Group8Eval), then the
// level-0 walk with Group8FilterEval (hnsw_walk2.hpp) — binary16 shadow rows first, f32 rows for what the shadow cannot reject.
// stats[6] / stats[7] / stats[5]: evaluations the filter rejected / f32 rows read at level 0 / shadow rows read.
// BITS: the shadow phase A reads (16: rows_h; 8: rows_b + adj0_m).  stats[5] counts the shadow rows of whichever kind.
// VISMODE == VIS_LDS16 (the headline instance alone: walk variant 4, BITS == ROW_FILTER_8I): the LDS visited set at 16 bits per entry (vis16.hpp), which is what
// lets seven traversals share a CU's LDS; the instance leaves the register allocator room for two waves per SIMD.  bloom_words then carries
// (capacity limit << 8) | log2(buckets); stats[16] / stats[17]: the largest stash count / visited count of a traversal (atomic maxima).
// upper (kernel argument, wave-uniform): how the prologue descends.  ROWF_UPPER_FILTER: the 8-bit kinds run the upper levels through the certified filter
// (hnsw_walk2.hpp: greedy_level8_filtered; stats[18] / [19] / [20]: shadow rows / rejected evaluations / f32 rows above level 0, the entrypoint's own row
// not among them).  ROWF_UPPER_CACHED: the entrypoint row and the descent's rows are loaded without the launch's non-temporal hint — they are what all the
// queries of a launch share.  The level-0 loads keep the hint either way.
enum { ROWF_UPPER_FILTER = 1u, ROWF_UPPER_CACHED = 2u };
// entrypoint + upper levels of the row-filter kernel: DNT is the hint of THESE loads.  fev: the level-0 evaluator, for the query's digit planes.
template <bool DNT, int BITS, class FEV>
__device__ __forceinline__ void rowfilter_descent(const GraphView& g, WaveCtx& w, const FEV& fev, uint32_t& cur, float& curd, int entry_level, int lane, bool filter,
                                                  uint32_t& up_sh, uint32_t& up_rej, uint32_t& up_f32) {
  curd = Group8Eval<M_COS, Q_NONE, false, false, DNT>().one(g, w, cur, lane);   // hnsw.go:253
  curd = __shfl(curd, 0, 64);
  w.n_dist += 1;
  if constexpr (BITS == 8 || BITS == ROW_FILTER_8I) {
    if (filter) {
      Group8FilterEval<M_COS, Q_NONE, true, DNT, BITS> uev;
      uev.qd = fev.qd; uev.qt = fev.qt; uev.qe = fev.qe;
      for (int l = entry_level; l > 0; l--) greedy_level8_filtered(g, w, cur, curd, l, lane, uev);  // :254-256
      up_sh += uev.n_h16; up_rej += uev.n_rej; up_f32 += uev.n_f32;
      return;
    }
  }
  for (int l = entry_level; l > 0; l--) greedy_level8<M_COS, Q_NONE, false, DNT>(g, w, cur, curd, l, lane);  // :254-256
}

template <int PROFILE, int OPT, int VISMODE, bool NT, int BITS = 16>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(VISMODE == VIS_LDS16 ? 2 : 1)))
void hnsw_search2_rowfilter_kernel(GraphView g, int32_t entry, int32_t entry_level,
                                                                   const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                                   uint32_t nq, uint32_t k, uint32_t ef, uint32_t ef_pad, uint32_t bloom_words,
                                                                   uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                                   float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                                   unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                                   size_t vis_stride, uint32_t* __restrict__ vis_epoch, uint32_t upper) {
  static_assert((OPT & W2_ADJN) != 0, "the filter takes the neighbours' norms from the adjacency rows");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x;
  WaveCtx w;
  size_t off = ((size_t)g.dim * 4 + 15) & ~(size_t)15;
  w.qp = reinterpret_cast<float*>(smem); w.qs = nullptr;   // [query in rows8 order | scratch | result set | visited hash or Bloom filter], as hnsw_search2_kernel<.., EV8>
  w.scr = reinterpret_cast<uint32_t*>(smem + off);
  off += 96 * 4;
  [[maybe_unused]] uint8_t* qd = nullptr;   // BITS == ROW_FILTER_8I: the query's two digit planes between the scratch and the result set (plan_search adds the same bytes)
  if constexpr (BITS == ROW_FILTER_8I) { qd = smem + off; off += (size_t)g.dim * 2; }
  w.res0 = reinterpret_cast<unsigned long long*>(smem + off);
  w.ef_pad = ef_pad;
  if constexpr (VISMODE == VIS_LDS16) {
    static_assert(BITS == ROW_FILTER_8I && OPT == 4, "the 16-bit visited set serves the headline instance");
    w.vis = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad);
    w.hcap = bloom_words >> 8; w.hcap_mask = bloom_words & 0xffu;
    w.bloom = nullptr; w.bloom_words = 0; w.bloom_shift = 0;
    w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0;
  } else if constexpr (VISMODE == VIS_LDS) {
    w.vis = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad);
    w.hcap = bloom_words; w.hcap_mask = bloom_words - 1;
    w.bloom = nullptr; w.bloom_words = 0; w.bloom_shift = 0;
    w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0;
  } else {
    w.vis = nullptr;
    w.bloom = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad);
    w.bloom_words = bloom_words; w.bloom_shift = 32u - (uint32_t)__builtin_ctz(bloom_words | 0x80000000u);
    w.hcap = 0; w.hcap_mask = 0;
    w.visg = visg + (size_t)blockIdx.x * vis_stride; w.vis_bytes = vis_stride; w.epoch = vis_epoch[blockIdx.x];
  }
  for (;;) {
    const uint32_t qt = atomicAdd(counter, lane == 0 ? 1u : 0u);  // branch-free work fetch, see hnsw_search_kernel
    const uint32_t qi = (uint32_t)__shfl((int)qt, 0, 64);
    if (qi >= nq) break;
    w.n_dist = w.n_exp = w.n_hops = w.n_resets = 0; w.err = 0;
    if constexpr (VISMODE == VIS_LDS16) w.v16_stash = w.v16_count = 0;
#ifdef COLTT_PHASE_TIMING
    for (int i_ = 0; i_ < 8; i_++) w.pt[i_] = 0;
    w.t_last = __builtin_amdgcn_s_memtime();
#endif
    wave_sync();
    for (int e = lane; e < g.dim; e += 64) w.qp[rows8_qindex<Q_NONE>(e)] = q_eff[(size_t)qi * g.dim + e];
    w.qnorm = qnorms[qi];
    wave_sync();
    Group8FilterEval<M_COS, Q_NONE, true, NT, BITS> fev;
    if constexpr (BITS == ROW_FILTER_8I) {   // the query's digit planes, scale and error norm: once per traversal
      fev.qd = qd;
      query_digits8i(w.qp, qd, g.dim, lane, fev.qt, fev.qe);
      wave_sync();
    }
    uint32_t cur = (uint32_t)entry;
    // (two waves per SIMD: the entry row's line addresses are the same for every query, and hoisted out of this loop they are 24 registers the instance has to
    // spill and reload one by one in front of each line's load; re-derived per query they cost a dozen additions)
    if constexpr (VISMODE == VIS_LDS16) asm volatile("" : "+s"(cur));
    float curd;
    uint32_t up_sh = 0, up_rej = 0, up_f32 = 0;   // the descent's own filter counters (stats[18 .. 20])
    // (both branches wave-uniform, decided by a kernel argument: one of the descents runs per launch)
    if (NT && (upper & ROWF_UPPER_CACHED)) rowfilter_descent<false, BITS>(g, w, fev, cur, curd, entry_level, lane, (upper & ROWF_UPPER_FILTER) != 0, up_sh, up_rej, up_f32);
    else rowfilter_descent<NT, BITS>(g, w, fev, cur, curd, entry_level, lane, (upper & ROWF_UPPER_FILTER) != 0, up_sh, up_rej, up_f32);
    COLTT_PT(w, 5)
    w.n_dist += 1;  // searchLevel re-evaluates the entrypoint distance (hnsw.go:346)
    uint32_t len;
    search_level2<M_COS, Q_NONE, PROFILE, OPT, VISMODE, false>(g, w, cur, curd, ef, lane, len, fev);  // :258-259
    const uint32_t n = len < k ? len : k;  // selectNeighbors + pop (:261-277) == the k smallest, ascending
    for (uint32_t i = lane; i < n; i += 64) {
      const unsigned long long e = w.res0[i];
      const uint32_t slot = (uint32_t)e >> 1;
      out_ids[(size_t)qi * k + i] = g.ids ? g.ids[slot] : (uint64_t)slot;
      out_scores[(size_t)qi * k + i] = __uint_as_float((uint32_t)(e >> 32));
    }
    if (lane == 0) {
      out_counts[qi] = n;
      atomicAdd(&stats[0], (unsigned long long)w.n_dist);
      atomicAdd(&stats[1], (unsigned long long)w.n_exp);
      atomicAdd(&stats[2], (unsigned long long)w.n_hops);
      if (w.err) atomicOr(&stats[4], (unsigned long long)w.err);
      atomicAdd(&stats[6], (unsigned long long)fev.n_rej);
      atomicAdd(&stats[7], (unsigned long long)fev.n_f32);
      atomicAdd(&stats[5], (unsigned long long)fev.n_h16);
      if constexpr (BITS == 8 || BITS == ROW_FILTER_8I) {
        if (upper & ROWF_UPPER_FILTER) { atomicAdd(&stats[18], (unsigned long long)up_sh); atomicAdd(&stats[19], (unsigned long long)up_rej); atomicAdd(&stats[20], (unsigned long long)up_f32); }
      }
      if constexpr (VISMODE == VIS_LDS16) { atomicMax(&stats[16], (unsigned long long)w.v16_stash); atomicMax(&stats[17], (unsigned long long)w.v16_count); }
#ifdef COLTT_PHASE_TIMING
      COLTT_PT(w, 6)
      for (int i_ = 0; i_ < 8; i_++) atomicAdd(&stats[8 + i_], w.pt[i_]);
#endif
    }
  }
  if constexpr (VISMODE == VIS_HBM) { if (lane == 0) vis_epoch[blockIdx.x] = w.epoch; }
}

// The row filter's evaluator on CHOSEN (query, slot) pairs — a test-and-diagnostics kernel (coltt_hnsw_row_filter_probe), not a search.  One wave per
// query, the LDS layout of the kernel above's prologue (query in rows8 order | 96 words of scratch); lane pair p holds slots[q][p] (NBR_NONE: not fresh)
// with its norm and, for the 8-bit shadow, its (scale, error norm) from the per-slot arrays, and the wave makes ONE call of Group8FilterEval::filtered —
// the dispatch, the streams and both phases are the walk's own code, nothing of them is restated here.  out_r: the value the even lane of every pair got
// back; out_counts: (n_rej, n_f32, n_h16) of the call.  A chunk without a fresh pair makes no call, as in search_level2.
template <bool NT, int BITS>
__global__ __launch_bounds__(64) void hnsw_row_filter_probe_kernel(GraphView g, const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                                  const uint32_t* __restrict__ slots, const float* __restrict__ lower_bound, int full_at_pop,
                                                                  float* __restrict__ out_r, float* __restrict__ out_rnorm, uint32_t* __restrict__ out_counts,
                                                                  long long* __restrict__ out_isum, float* __restrict__ out_qte) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x;
  const uint32_t qi = blockIdx.x;
  WaveCtx w = {};
  const size_t off = ((size_t)g.dim * 4 + 15) & ~(size_t)15;
  w.qp = reinterpret_cast<float*>(smem);
  w.scr = reinterpret_cast<uint32_t*>(smem + off);
  for (int e = lane; e < g.dim; e += 64) w.qp[rows8_qindex<Q_NONE>(e)] = q_eff[(size_t)qi * g.dim + e];
  w.qnorm = qnorms[qi];
  wave_sync();
  const int half = lane & 1, p = lane >> 1;
  const uint32_t nb = slots[(size_t)qi * 32 + p];
  const bool fresh = nb != NBR_NONE;
  const float nrm = fresh ? g.norms[nb] : 0.f;
  Group8FilterEval<M_COS, Q_NONE, true, NT, BITS> fev;
  if constexpr (BITS == 8 || BITS == ROW_FILTER_8I) fev.mt = fresh ? g.rows_m[nb] : float2{0.f, 0.f};
  if constexpr (BITS == ROW_FILTER_8I) {   // the walk's own prologue step: the planes behind the scratch
    uint8_t* const qd = smem + off + 96 * 4;
    fev.qd = qd;
    query_digits8i(w.qp, qd, g.dim, lane, fev.qt, fev.qe);
    wave_sync();
  }
  float r = 0.f;
  if (__ballot(fresh)) r = fev.filtered(g, w, nb, fresh, nrm, half, lane, lower_bound[qi], full_at_pop != 0);   // (wave-uniform)
  if (half == 0) { out_r[(size_t)qi * 32 + p] = r; out_rnorm[(size_t)qi * 32 + p] = nrm; }
  if constexpr (BITS == ROW_FILTER_8I) {   // the integer sum of every fresh pair of a full-set call, and the query's (scale, error norm)
    if (out_isum && half == 0) out_isum[(size_t)qi * 32 + p] = fev.isum;
    if (out_qte && lane == 0) { out_qte[(size_t)qi * 2] = fev.qt; out_qte[(size_t)qi * 2 + 1] = fev.qe; }
  }
  if (lane == 0) { out_counts[(size_t)qi * 3] = fev.n_rej; out_counts[(size_t)qi * 3 + 1] = fev.n_f32; out_counts[(size_t)qi * 3 + 2] = fev.n_h16; }
}


// Hnsw.Search with a 256-thread workgroup per query (hnsw_lat.hpp): the latency path for small batches — the reference serves one
// query per RPC (core/core.go:633-667).  One workgroup per CU, queries pulled from a global counter.  Same answers, score bits and
// counters as the one-wave kernel (the parity tests run both).
// TP: how the rows are read (hnsw_lat.hpp: lat_eval_chunk) — > 0 line-transposed rows of TP 128-byte lines, -1 line-transposed of any length, 0 natural order
// (staged through LDS).  SEQ: hnsw_walk2.hpp's level-0 walk on wave 0 with the chunks evaluated by all four waves (rows of more than one chunk, mMax0 > 32, and
// the COLTT_LAT_SEQ=1 A/B partner) instead of the walk that is software-pipelined over expansions.  One walk and one evaluation per instance (round 6).
template <int METRIC, int QUANT, int TP = 0, bool SEQ = false>
__global__ __launch_bounds__(256) void hnsw_search_lat_kernel(GraphView g, int32_t entry, int32_t entry_level,
                                                             const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                             uint32_t nq, uint32_t k, uint32_t ef, uint32_t ef_pad, uint32_t hcap,
                                                             uint32_t* __restrict__ counter, uint64_t* __restrict__ out_ids,
                                                             float* __restrict__ out_scores, uint32_t* __restrict__ out_counts,
                                                             unsigned long long* __restrict__ stats, unsigned long long* __restrict__ mbox, int helpers) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // helped launches (mbox != null; batches of <= LAT_MASTERS queries): blocks 0 .. LAT_MASTERS - 1 walk, block m + 8 (h + 1) is walking block m's helper h
  unsigned long long* hint_box = nullptr;
  if (mbox) {
    const uint32_t m = blockIdx.x & (uint32_t)(LAT_MASTERS - 1);
    unsigned long long* const box = mbox + (size_t)m * (LAT_HELPERS_MAX + 1);
    if (blockIdx.x >= (uint32_t)LAT_MASTERS) {
      lat_helper_loop(g, box, (int)(blockIdx.x / LAT_MASTERS) - 1, reinterpret_cast<LatShared*>(smem));
      return;
    }
    hint_box = box;
  }
  WaveCtx w;
  size_t off = (lat_q_floats(g.dim) * 4 + 15) & ~(size_t)15;   // the query, residue-major (hnsw_lat.hpp: lat_n8p)
  w.qs = reinterpret_cast<float*>(smem);
  w.res0 = reinterpret_cast<unsigned long long*>(smem + off);
  LatShared* xs = reinterpret_cast<LatShared*>(w.res0 + (size_t)ef_pad);
  uint8_t* stage = reinterpret_cast<uint8_t*>(xs + 1);                                   // TP == 0: [32][stride + pad] rows of the chunk being evaluated
  w.vis = reinterpret_cast<uint32_t*>(stage + (TP == LAT_TP_STAGED ? (size_t)LAT_ROWS * (g.stride + LAT_PAD) : (size_t)0));
  w.ef_pad = ef_pad; w.hcap = hcap; w.hcap_mask = hcap - 1;
  w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0; w.bloom = nullptr; w.bloom_words = 0; w.bloom_shift = 0;
  for (;;) {
    __syncthreads();   // everybody is done with the previous query's LDS state (and with ctl[1])
    if (threadIdx.x == 0) xs->ctl[1] = atomicAdd(counter, 1u);
    __syncthreads();
    const uint32_t qi = xs->ctl[1];
    if (qi >= nq) break;
    w.n_dist = w.n_exp = w.n_hops = w.n_resets = 0; w.err = 0;
#ifdef COLTT_PHASE_TIMING
    for (int i_ = 0; i_ < 8; i_++) w.pt[i_] = 0;
    w.t_last = __builtin_amdgcn_s_memtime();
#endif
    {
      const int n8 = g.dim >> 3, n8p = lat_n8p(g.dim);
      for (int e = threadIdx.x; e < g.dim; e += 256) {
        const float v = q_eff[(size_t)qi * g.dim + e];
        if (e < n8 * 8) w.qs[(size_t)(e & 7) * n8p + (e >> 3)] = v; else w.qs[(size_t)8 * n8p + (e - n8 * 8)] = v;
      }
    }
    w.qnorm = qnorms[qi];
    // minDistance := Distance(query, entrypoint.vector) (hnsw.go:253): a chunk with one live row
    if (threadIdx.x < LAT_ROWS) { xs->nb[threadIdx.x] = threadIdx.x == 0 ? (uint32_t)entry : NBR_NONE; xs->fresh[threadIdx.x] = threadIdx.x == 0 ? 1u : 0u; }
    lat_chunk<METRIC, QUANT, TP>(g, w, xs, stage, wave, lane);
    uint32_t cur = (uint32_t)entry;
    float curd = xs->d[0];
    w.n_dist += 1;
    __syncthreads();   // xs->d[0] has been read by every wave before the next chunk overwrites it
    for (int l = entry_level; l > 0; l--) greedy_level_lat<METRIC, QUANT, TP>(g, w, xs, stage, cur, curd, l, wave, lane);  // :254-256
#ifdef COLTT_PHASE_TIMING
    if (wave == 0) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); w.pt[6] += t_ - w.t_last; w.t_last = t_; }   // query load + entry + upper levels
#endif
    w.n_dist += 1;  // searchLevel re-evaluates the entrypoint distance (hnsw.go:346)
    uint32_t len;
    if constexpr (!SEQ) {   // rows of one chunk (mMax0 <= 32: the host checks): the walk that is software-pipelined over expansions (hnsw_lat.hpp)
      search_level_lat3<METRIC, QUANT, TP>(g, w, xs, stage, cur, curd, ef, wave, lane, len, hint_box, helpers);  // :258-259
    } else if (wave == 0) {   // hnsw_walk2.hpp's level-0 walk on wave 0, the chunks evaluated by all four waves (hnsw_lat.hpp: LatEval)
      if (lane == 0) xs->ctl[0] = 1u;
      LatEval<METRIC, QUANT, TP> ev{xs, stage};
      search_level2<METRIC, QUANT, PROF_SEARCH_LDS, W2_DELTA, VIS_LDS, true>(g, w, cur, curd, ef, lane, len, ev);  // :258-259
      wave_sync();
      if (lane == 0) xs->ctl[0] = 0u;
      lds_barrier();   // releases the companions
    } else {
      len = 0;
      lat_companion<METRIC, QUANT, TP>(g, w, xs, stage, wave, lane);
    }
    if (wave == 0) {
      const uint32_t n = len < k ? len : k;
      for (uint32_t i = lane; i < n; i += 64) {
        const unsigned long long e = w.res0[i];
        const uint32_t slot = (uint32_t)e >> 1;
        out_ids[(size_t)qi * k + i] = g.ids ? g.ids[slot] : (uint64_t)slot;
        out_scores[(size_t)qi * k + i] = __uint_as_float((uint32_t)(e >> 32));
      }
      if (lane == 0) {
        out_counts[qi] = n;
        atomicAdd(&stats[0], (unsigned long long)w.n_dist);
        atomicAdd(&stats[1], (unsigned long long)w.n_exp);
        atomicAdd(&stats[2], (unsigned long long)w.n_hops);
        if (w.err) atomicOr(&stats[4], (unsigned long long)w.err);
#ifdef COLTT_PHASE_TIMING
        for (int i_ = 0; i_ < 8; i_++) atomicAdd(&stats[8 + i_], w.pt[i_]);
#endif
      }
    }
  }
  if (hint_box && threadIdx.x == 0) __hip_atomic_store(hint_box + LAT_HELPERS_MAX, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // releases this block's helpers
}



// Hnsw.Search over product-quantiser codes + exact re-rank (hnsw_pq.hpp): one wave per query, queries pulled from a global counter.
// OPT / VISMODE as hnsw_search2_kernel (0 + VIS_LDS: the LDS hash; 2 + VIS_HBM: byte map, delta result set; no Bloom filter — see pq_geom).
// The walk touches no stored row: its survivors (slots, nearest first by table distance) go to HBM and the exact re-rank is two small kernels of its
// own (below) — inside the walk kernel it was 19 % of the time (one 128-byte line per row in flight, the burst depth the walk's register budget left:
// profiles/r05p_phase_breakdown.txt) and tied 24 instances of this kernel to the row format.
// LS: the table's row length (log2) when it is one of the common ones (16, 32, 256 centroids), 0 = any; NP: 16-byte pieces per code row, 0 = any;
// NBR: level-0 code rows come from the neighbourhood blocks, requested with the adjacency row (hnsw_pq.hpp: AdcEval<LS, NP, NBR>).
// FILTER (coltt_hnsw_pq_search_filtered, WALK): the same walk, plus the allowed set R (hnsw_dev.hpp: FiltSet; hnsw_walk2.hpp: search_level2<.., FILTER>) of
// fcap entries, padded to 64, in LDS between the result set and the visited hash; the survivors handed to the re-rank are R's slots, nearest first, instead
// of the result set's.  fv / fcap are read by the FILTER instances only.
// PERQ (coltt_hnsw_pq_search_filtered_batch, with FILTER): the claimed index qi selects a descriptor (hnsw_dev.hpp: PqFiltQuery) that gives the query's
// filter, ef, LDS geometry and capacity of R; the wave lays out [result set | R | visited hash] behind the table anew for every query it claims (the table
// stays at 0).  The descriptors arrive in fv.bits (the kernel's parameter list is the one its other instances have); ef / rerank / vis_words / fcap are
// then ignored, ef_pad is the stride of surv (the largest of the launch's queries'), and the dynamic LDS is the largest of the launch's queries'.  A
// query whose LDS hash would have needed its reset path leaves err 8 in its descriptor, no survivors and nothing in the sums: the host runs it again.
template <int OPT, int VISMODE, int LS, int NP = 0, bool NBR = false, bool FILTER = false, bool PERQ = false>
// amdgpu_waves_per_eu(3): <= 168 VGPRs, three waves per SIMD — the walk is latency-bound, resident traversals are its throughput
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void hnsw_pq_search_kernel(GraphView g, int32_t entry, int32_t entry_level, const unsigned short* __restrict__ lut_g,
                                                            const uint8_t* __restrict__ codes, const uint8_t* __restrict__ nbrc, uint32_t row_bytes, uint32_t lut_shift, uint32_t nq, uint32_t k,
                                                            uint32_t ef, uint32_t ef_pad, uint32_t rerank, uint32_t vis_words,
                                                            uint32_t* __restrict__ counter, uint32_t* __restrict__ surv, uint32_t* __restrict__ surv_cnt,
                                                            unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                            size_t vis_stride, uint32_t* __restrict__ vis_epoch, FilterView fv, uint32_t fcap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x;
  WaveCtx w;
  // LDS: [table | result set | R (FILTER) | visited hash or Bloom filter] — the table first: its lookups address it by immediate offsets (AdcEval<LS>).
  // No copy of the query: the walk only needs its table.
  unsigned short* const lut = reinterpret_cast<unsigned short*>(smem);
  if constexpr (LS != 0) {   // AdcEval<LS> addresses the table by absolute LDS offsets: this kernel has no static LDS, so its dynamic LDS starts at 0
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)smem != 0u) { if (lane == 0) atomicOr(&stats[4], 128ull); return; }
  }
  static_assert(!PERQ || FILTER, "a descriptor per query is the filtered batch's");
  const size_t off_table = ((size_t)pq_walk_table_rows(row_bytes >> 4) << lut_shift) * 2;   // the pair-interleaved table (hnsw_pq.hpp); a multiple of 512
  w.qs = nullptr; w.qp = nullptr; w.scr = nullptr;
  FiltSet fs;
  (void)fs;
  if constexpr (FILTER) { fs.len = 0; fs.f = fv; }
  // what lies behind the table, for one geometry: once per launch, or (PERQ) once per claimed query
  auto lay_out = [&](uint32_t ef_pad_q, uint32_t fcap_q, uint32_t vis_words_q) {
    size_t off = off_table;
    w.res0 = reinterpret_cast<unsigned long long*>(smem + off); off += (size_t)ef_pad_q * 8;
    w.ef_pad = ef_pad_q;
    if constexpr (FILTER) { fs.r = reinterpret_cast<unsigned long long*>(smem + off); off += (size_t)((fcap_q + 63u) & ~63u) * 8; fs.cap = fcap_q; }
    if constexpr (VISMODE == VIS_LDS) {
      w.vis = reinterpret_cast<uint32_t*>(smem + off); off += (size_t)vis_words_q * 4;
      w.hcap = vis_words_q; w.hcap_mask = vis_words_q - 1;
      w.bloom = nullptr; w.bloom_words = 0; w.bloom_shift = 0;
    } else {
      w.vis = nullptr; w.hcap = 0; w.hcap_mask = 0;
      w.bloom = reinterpret_cast<uint32_t*>(smem + off); off += (size_t)vis_words_q * 4;
      w.bloom_words = vis_words_q; w.bloom_shift = 32u - (uint32_t)__builtin_ctz(vis_words_q | 0x80000000u);
    }
  };
  if constexpr (!PERQ) lay_out(ef_pad, fcap, vis_words);
  if constexpr (VISMODE == VIS_LDS) { w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0; }
  else { w.visg = visg + (size_t)blockIdx.x * vis_stride; w.vis_bytes = vis_stride; w.epoch = vis_epoch[blockIdx.x]; }
  AdcEval<LS, NP, NBR> ev; ev.codes = codes; ev.row_bytes = row_bytes; ev.lut = lut; ev.lut_shift = lut_shift; ev.nbrc = nbrc; ev.nbr_stride = g.mMax0 * row_bytes;
  ev.hsel = (uint32_t)lane & 1u;
  for (;;) {
    const uint32_t qt = atomicAdd(counter, lane == 0 ? 1u : 0u);  // branch-free work fetch, see hnsw_search_kernel
    const uint32_t qi = (uint32_t)__shfl((int)qt, 0, 64);
    if (qi >= nq) break;
    if constexpr (PERQ) {   // the descriptor is wave-uniform: its words go to scalar registers
      const uint32_t* dw = reinterpret_cast<const uint32_t*>(reinterpret_cast<const PqFiltQuery*>(fv.bits) + qi);
      auto rf = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)dw[i]); };
      fs.f = FilterView{reinterpret_cast<const uint32_t*>(((uint64_t)rf(1) << 32) | rf(0)), rf(2)};
      ef = rf(3);
      lay_out(rf(4), rf(6), rf(5));
    }
    w.n_dist = w.n_exp = w.n_hops = w.n_resets = 0; w.err = 0;
#ifdef COLTT_PHASE_TIMING
    for (int i_ = 0; i_ < 8; i_++) w.pt[i_] = 0;
    w.t_last = __builtin_amdgcn_s_memtime();
#endif
    wave_sync();
    {  // the query's table as pq_lut16_kernel wrote it — row_bytes rows of (1 << lut_shift) binary16 entries — copied 16 bytes per lane and step into the
      // PAIR-INTERLEAVED layout the lane pairs read (hnsw_pq.hpp): table row j -> LDS row 2 (j mod JS) + (j div JS), JS = 16 * ceil(pieces / 2)
      const u32x4v* src = reinterpret_cast<const u32x4v*>(lut_g + ((size_t)qi * row_bytes << lut_shift));
      u32x4v* dst = reinterpret_cast<u32x4v*>(lut);
      const uint32_t psh = lut_shift - 3;                    // log2 of the 16-byte pieces per table row (lut_shift >= 4)
      const uint32_t total = row_bytes << psh;               // 16-byte pieces (row_bytes is a multiple of 16)
      const uint32_t js = 16u * (((row_bytes >> 4) + 1u) >> 1);
      for (uint32_t i = (uint32_t)lane; i < total; i += 64) {
        const uint32_t j = i >> psh, within = i & ((1u << psh) - 1u);
        const uint32_t r = j < js ? 2u * j : 2u * (j - js) + 1u;
        dst[(r << psh) + within] = src[i];
      }
    }
    w.qnorm = 0.f;
    wave_sync();
    uint32_t cur = (uint32_t)entry;
    float curd = ev.adc(cur);   // minDistance := d(query, entrypoint) (hnsw.go:253), the same value in every lane
    w.n_dist += 1;
    for (int l = entry_level; l > 0; l--) greedy_level_adc(g, w, ev, cur, curd, l, lane);  // :254-256
    w.n_dist += 1;  // searchLevel re-evaluates the entrypoint distance (hnsw.go:346)
    COLTT_PT(w, 5)  // table load + entry + upper levels
    uint32_t len;
    uint32_t r;
    if constexpr (FILTER) {
      search_level2<M_L2, Q_F16, PROF_SEARCH_HBM, OPT, VISMODE, true, AdcEval<LS, NP, NBR>&, true>(g, w, cur, curd, ef, lane, len, ev, &fs);
      r = fs.len;   // <= fcap <= ef: the host folded `rerank` into fcap
      if constexpr (PERQ) {
        const uint32_t qerr = (uint32_t)__shfl((int)w.err, 0, 64);
        if (qerr) {   // reported per query; it hands nothing to the re-rank and stays out of the sums
          if (lane == 0) { const_cast<PqFiltQuery*>(reinterpret_cast<const PqFiltQuery*>(fv.bits))[qi].err = qerr; surv_cnt[qi] = 0u; atomicOr(&stats[4], (unsigned long long)qerr); }
          continue;
        }
      }
      for (uint32_t i = (uint32_t)lane; i < r; i += 64) surv[(size_t)qi * ef_pad + i] = (uint32_t)fs.r[i] >> 1;   // R, nearest first by table distance
    } else {
      search_level2<M_L2, Q_F16, PROF_SEARCH_HBM, OPT, VISMODE, true>(g, w, cur, curd, ef, lane, len, ev);  // :258-259 (M_L2: no norms ride along; Q_F16: the adjacency prefetch)
      r = rerank == 0 ? len : (rerank > k ? rerank : k);
      r = r < len ? r : len;
      for (uint32_t i = (uint32_t)lane; i < r; i += 64) surv[(size_t)qi * ef_pad + i] = (uint32_t)w.res0[i] >> 1;   // the r nearest by table distance, in that order
    }
    COLTT_PT(w, 6)  // final delta flush + survivors' write-out
    if (lane == 0) {
#ifdef COLTT_PHASE_TIMING
      for (int i_ = 0; i_ < 8; i_++) atomicAdd(&stats[8 + i_], w.pt[i_]);
#endif
      surv_cnt[qi] = r;
      atomicAdd(&stats[0], (unsigned long long)w.n_dist);
      atomicAdd(&stats[1], (unsigned long long)w.n_exp);
      atomicAdd(&stats[2], (unsigned long long)w.n_hops);
      atomicAdd(&stats[3], (unsigned long long)r);
      if (w.err) atomicOr(&stats[4], (unsigned long long)w.err);
    }
  }
  if constexpr (VISMODE == VIS_HBM) { if (lane == 0) vis_epoch[blockIdx.x] = w.epoch; }
}

// Exact re-rank, step 1: the index's distance (reference summation order, exact.hpp) of every survivor.  One wave per (query, 32 survivors): lane pair p
// owns survivor 32 * chunk + p; key = exact score bits << 32 | slot << 1, the walk's own key layout.  The query is read from the prepared batch.
template <int METRIC, int QUANT, bool R8>
__global__ __launch_bounds__(64) void hnsw_pq_rerank_kernel(GraphView g, const float* __restrict__ q_eff, const float* __restrict__ qnorms, const uint32_t* __restrict__ surv,
                                                            const uint32_t* __restrict__ surv_cnt, uint32_t ef_pad, unsigned long long* __restrict__ keys) {
  const uint32_t qi = blockIdx.y, r = surv_cnt[qi];
  if (blockIdx.x * 32u >= r) return;   // wave-uniform
  const int lane = threadIdx.x, half = lane & 1, p = lane >> 1;
  WaveCtx w;
  w.qs = const_cast<float*>(q_eff + (size_t)qi * g.dim); w.qnorm = qnorms[qi];
  const uint32_t i = blockIdx.x * 32u + (uint32_t)p;
  const bool valid = i < r;
  const uint32_t slot = surv[(size_t)qi * ef_pad + (valid ? i : blockIdx.x * 32u)];   // an idle pair re-evaluates a live survivor (DPP partners stay active)
  const float d = eval_pair<METRIC, QUANT, PROF_SEARCH_HBM, R8>(g, w, slot, half);
  if (valid && half == 0) keys[(size_t)qi * ef_pad + i] = ((unsigned long long)__float_as_uint(d) << 32) | ((unsigned long long)slot << 1);
}
// step 2, hnsw_pq_select_kernel: hnsw.hip, beside its launcher (not a template: it stands in the one translation unit that launches it)

// coltt_hnsw_search_filtered, EXACT: the k nearest live allowed vertices by (score bits, slot), over the filter's compacted slot list.
// Step 1: one wave per (query group of <= FILT_QG queries, chunk of the list).  The group's queries sit in LDS; lane pair p scores slot
// base + p against each of them in turn with the walk's own evaluator (exact.hpp pair core; over line-transposed rows the pair core that
// reads them, pair_distance_r8 — same values, same order, same bits), so a row comes from HBM once per group and from the caches after.
// Each query keeps the chunk's k smallest keys in LDS (hnsw_dev.hpp: sorted_offer); they go to part[q][chunk][0..cnt).
constexpr uint32_t FILT_QG = 8;
template <int METRIC, int QUANT, bool R8>
__global__ __launch_bounds__(64) void hnsw_filter_scan_kernel(GraphView g, const float* __restrict__ q_eff, const float* __restrict__ qnorms, uint32_t nq,
                                                              uint32_t qg, const uint32_t* __restrict__ slots, uint32_t n_slots, uint32_t chunk, uint32_t k,
                                                              uint32_t k_pad, unsigned long long* __restrict__ part, uint32_t* __restrict__ part_cnt,
                                                              unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane_in = threadIdx.x;
  const uint32_t q0 = blockIdx.y * qg, nchunks = gridDim.x;
  const uint32_t nqg = nq - q0 < qg ? nq - q0 : qg;
  const size_t qstride = ((size_t)g.dim + 3) & ~(size_t)3;
  float* const qs = reinterpret_cast<float*>(smem);                                              // [qg][qstride]
  unsigned long long* const top = reinterpret_cast<unsigned long long*>(qs + (size_t)qg * qstride);   // [qg][k_pad]
  for (uint32_t j = 0; j < nqg; j++)
    for (int e = lane_in; e < g.dim; e += 64) qs[(size_t)j * qstride + e] = q_eff[(size_t)(q0 + j) * g.dim + e];
  wave_sync();
  const uint32_t s0 = blockIdx.x * chunk, s1 = s0 + chunk < n_slots ? s0 + chunk : n_slots;
  uint32_t lens[FILT_QG];
#pragma unroll
  for (uint32_t j = 0; j < FILT_QG; j++) lens[j] = 0;
  unsigned long long rows = 0;
  for (uint32_t base = s0; base < s1; base += 32) {
    const int lane = opaque_lane(lane_in);
    const int half = lane & 1, p = lane >> 1;
    const uint32_t i = base + (uint32_t)p;
    const bool valid = i < s1;
    const uint32_t slot = slots[valid ? i : base];   // an idle pair re-evaluates a listed row (DPP partners stay active)
    const bool live = valid && !is_deleted(g, slot);   // tombstones at search time
    rows += __popcll(__ballot(live && half == 0));
#pragma unroll
    for (uint32_t j = 0; j < FILT_QG; j++) {
      if (j >= nqg) break;   // wave-uniform
      const float d = eval_pair_q<METRIC, QUANT, PROF_SEARCH_HBM, R8>(g, qs + (size_t)j * qstride, qnorms[q0 + j], slot, half);
      sorted_offer(top + (size_t)j * k_pad, lens[j], k, live && half == 0, ((unsigned long long)__float_as_uint(d) << 32) | ((unsigned long long)slot << 1),
                   lane, false);
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < FILT_QG; j++) {
    if (j >= nqg) break;
    const size_t q = q0 + j;
    for (uint32_t i = (uint32_t)lane_in; i < lens[j]; i += 64) part[(q * nchunks + blockIdx.x) * k + i] = top[(size_t)j * k_pad + i];
    if (lane_in == 0) part_cnt[q * nchunks + blockIdx.x] = lens[j];
  }
  if (lane_in == 0 && rows) atomicAdd(&stats[5], rows * nqg);
}
// step 2, hnsw_filter_select_kernel: hnsw_filter.hip, beside its launcher (as hnsw_pq_select_kernel)

// coltt_hnsw_search_filtered_batch, EXACT: the two steps above with a filter per query.  The host sorts the exact-path queries by filter
// and cuts groups of <= qg queries that share one; FiltExactQ e = such a query: its batch row and its run of chunk lists in part.  A tile
// = (group, chunk of the group's filter list): one wave of the scan, the same evaluator and the same top-k as hnsw_filter_scan_kernel.
struct FiltTile { const uint32_t* slots; uint32_t s0, s1, e0, nqg, chunk, pad_; };   // list[s0, s1) against queries e0 .. e0 + nqg - 1
struct FiltExactQ { uint32_t row, pbase, nchunks, pad_; };                        // part lists pbase .. pbase + nchunks - 1
template <int METRIC, int QUANT, bool R8>
__global__ __launch_bounds__(64) void hnsw_filter_scan_batch_kernel(GraphView g, const float* __restrict__ q_eff, const float* __restrict__ qnorms,
                                                                    const FiltTile* __restrict__ tiles, const FiltExactQ* __restrict__ eq, uint32_t qg,
                                                                    uint32_t k, uint32_t k_pad, unsigned long long* __restrict__ part,
                                                                    uint32_t* __restrict__ part_cnt, unsigned long long* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane_in = threadIdx.x;
  const uint32_t* tw = reinterpret_cast<const uint32_t*>(tiles + blockIdx.x);
  auto rf = [&](int i) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)tw[i]); };   // the tile is wave-uniform
  const uint32_t* const slots = reinterpret_cast<const uint32_t*>(((uint64_t)rf(1) << 32) | rf(0));
  const uint32_t s0 = rf(2), s1 = rf(3), e0 = rf(4), nqg = rf(5), c = rf(6);
  const size_t qstride = ((size_t)g.dim + 3) & ~(size_t)3;
  float* const qs = reinterpret_cast<float*>(smem);                                              // [qg][qstride]
  unsigned long long* const top = reinterpret_cast<unsigned long long*>(qs + (size_t)qg * qstride);   // [qg][k_pad]
  uint32_t rows_of[FILT_QG];
#pragma unroll
  for (uint32_t j = 0; j < FILT_QG; j++) rows_of[j] = j < nqg ? (uint32_t)__builtin_amdgcn_readfirstlane((int)eq[e0 + j].row) : 0u;
  for (uint32_t j = 0; j < nqg; j++)
    for (int e = lane_in; e < g.dim; e += 64) qs[(size_t)j * qstride + e] = q_eff[(size_t)eq[e0 + j].row * g.dim + e];
  wave_sync();
  uint32_t lens[FILT_QG];
#pragma unroll
  for (uint32_t j = 0; j < FILT_QG; j++) lens[j] = 0;
  unsigned long long rows = 0;
  for (uint32_t base = s0; base < s1; base += 32) {
    const int lane = opaque_lane(lane_in);
    const int half = lane & 1, p = lane >> 1;
    const uint32_t i = base + (uint32_t)p;
    const bool valid = i < s1;
    const uint32_t slot = slots[valid ? i : base];   // an idle pair re-evaluates a listed row (DPP partners stay active)
    const bool live = valid && !is_deleted(g, slot);   // tombstones at search time
    rows += __popcll(__ballot(live && half == 0));
#pragma unroll
    for (uint32_t j = 0; j < FILT_QG; j++) {
      if (j >= nqg) break;   // wave-uniform
      const float d = eval_pair_q<METRIC, QUANT, PROF_SEARCH_HBM, R8>(g, qs + (size_t)j * qstride, qnorms[rows_of[j]], slot, half);
      sorted_offer(top + (size_t)j * k_pad, lens[j], k, live && half == 0, ((unsigned long long)__float_as_uint(d) << 32) | ((unsigned long long)slot << 1),
                   lane, false);
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < FILT_QG; j++) {
    if (j >= nqg) break;
    const size_t l = (size_t)eq[e0 + j].pbase + c;
    for (uint32_t i = (uint32_t)lane_in; i < lens[j]; i += 64) part[l * k + i] = top[(size_t)j * k_pad + i];
    if (lane_in == 0) part_cnt[l] = lens[j];
  }
  if (lane_in == 0 && rows) atomicAdd(&stats[5], rows * nqg);
}
// step 2: one wave per exact-path query merges its own chunk lists and writes its batch row.  (A template, like every kernel added with it,
// so that it is instantiated after the pre-existing kernels and their assembly stays byte-identical.)
template <int = 0>
__global__ __launch_bounds__(64) void hnsw_filter_select_batch_kernel(const unsigned long long* __restrict__ part, const uint32_t* __restrict__ part_cnt,
                                                                      const FiltExactQ* __restrict__ eq, uint32_t k, const uint64_t* __restrict__ ids,
                                                                      uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                                      uint32_t* __restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  unsigned long long* const top = reinterpret_cast<unsigned long long*>(smem);
  const FiltExactQ d = eq[blockIdx.x];
  const size_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.row);
  const size_t pbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.pbase);
  const uint32_t nchunks = (uint32_t)__builtin_amdgcn_readfirstlane((int)d.nchunks);
  const int lane_in = threadIdx.x;
  uint32_t len = 0;
  for (uint32_t c = 0; c < nchunks; c++) {
    const uint32_t cnt = part_cnt[pbase + c];
    const unsigned long long* src = part + (pbase + c) * k;
    for (uint32_t b = 0; b < cnt; b += 64) {
      const int lane = opaque_lane(lane_in);
      const bool take = b + (uint32_t)lane < cnt;
      sorted_offer(top, len, k, take, take ? src[b + lane] : ~0ull, lane, false);
    }
  }
  for (uint32_t i = (uint32_t)lane_in; i < len; i += 64) {
    const unsigned long long e = top[i];
    const uint32_t slot = (uint32_t)e >> 1;
    out_ids[q * k + i] = ids ? ids[slot] : (uint64_t)slot;
    out_scores[q * k + i] = __uint_as_float((uint32_t)(e >> 32));
  }
  if (lane_in == 0) out_counts[q] = len;
}

}  // namespace kern
}  // namespace coltt
