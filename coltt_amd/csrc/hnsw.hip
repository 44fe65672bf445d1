// hnsw.hip — core/vectorindex.Hnsw on the GPU (core/vectorindex/hnsw.go).
//
// HBM layout (one index = one collection shard on one GPU), everything addressed by dense slot (u32 =
// insertion index, never reused until Compact — the oracle uses the same numbering as its canonical order):
//   rows      [cap][stride]     stored vectors (normalised for cosine; 4/2/1-byte codes)
//   norms     [cap] f32         ||row||^2 in AVX order
//   ids       [cap] u64         slot -> id                       (absent in dense-id mode)
//   adj0      [cap][mMax0] u32  level-0 neighbours, ascending slot, padded 0xffffffff   (+ adj0_d f32 distances)
//   upper_off [cap] u32         first upper row of the slot (a vertex of level L owns L consecutive rows)
//   adjU      [ucap][mMax] u32  levels >= 1                                                (+ adjU_d)
//   del_bits  [cap/32] u32      tombstones (hnswVertex.deleted)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <map>

#include "common.hpp"
#include "hnsw_index.hpp"   // HCtx, Hnsw and what hnsw_search2.hip / hnsw_filter.hip share with this file
#include "exact.hpp"
#include "hnsw_dev.hpp"
#include "hnsw_walk2.hpp"
#include "hnsw_lat.hpp"
#include "hnsw_pq.hpp"
#include "prep.hpp"
#include "rows8_ingest.hpp"   // the kernels that write the row-filter shadows

#include "hnsw_kernels.hpp"   // the search kernels (one-wave walk, large-ef walk, latency kernel, walk over PQ codes + re-rank)
#include "filter_expr.hpp"    // filter expressions: evaluate, compact, read-back
#include "attr_filter.hpp"    // attribute columns: predicate leaves of a filter programme, scatter, gather
#include "hnsw_compact.hpp"   // coltt_hnsw_compact: the plan, the row movers, the adjacency re-pack
#include "filter_carry.hpp"   // coltt_hnsw_compact_carry: resident filters and column bitmaps through the renumbering

using namespace coltt;
using namespace coltt::dev;
using namespace coltt::kern;
using namespace coltt::hnsw;

namespace {

// ---------------------------------------------------------------------------------------------------
// Graph construction (Hnsw.Insert, hnsw.go:104-167) for a batch of new vertices against the frozen graph.
// Phase A (this kernel, one wave per new vertex): greedy descent above the vertex level (:126-130), then per
// level searchLevel(efConstruction) + the m nearest (:132-140); the vertex's own rows are written here
// (nobody can reach a new vertex yet: it has no in-edges) and one link request per selected neighbour is
// queued: req[r] = {row id of the neighbour's level-l row, new slot, distance}, chained per target row through
// head[]/next[] with atomicExch.
// ---------------------------------------------------------------------------------------------------
struct BuildReq { uint32_t rid, from; float d; uint32_t next; };

template <int METRIC, int QUANT, bool VISG, bool R8 = false>
__global__ __launch_bounds__(64) void hnsw_build_search_kernel(GraphView g, int32_t entry, int32_t entry_level, uint32_t base,
                                                              uint32_t count, const int32_t* __restrict__ levels, uint32_t M,
                                                              uint32_t efc, uint32_t ef_pad, uint32_t hcap, uint64_t cap_slots,
                                                              uint32_t* __restrict__ counter, uint32_t* __restrict__ req_count,
                                                              BuildReq* __restrict__ req, uint32_t* __restrict__ head,
                                                              unsigned long long* __restrict__ stats, uint8_t* __restrict__ visg,
                                                              size_t vis_stride, uint32_t* __restrict__ vis_epoch,
                                                              uint32_t diverse /* 0 | 1 | 3 = keepPruned */, uint32_t ext_off) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x;
  WaveCtx w;
  size_t off = ((size_t)g.dim * 4 + 15) & ~(size_t)15;
  // diverse selection (algo 2): a second query buffer (the candidate's stored row), the chosen and the rejected keys — behind the walk's LDS
  float* const qs2 = reinterpret_cast<float*>(smem + ext_off);
  unsigned long long* const sel = reinterpret_cast<unsigned long long*>(smem + ext_off + off);
  unsigned long long* const prn = sel + 64;
  w.qs = reinterpret_cast<float*>(smem);
  w.res0 = reinterpret_cast<unsigned long long*>(smem + off);
  w.vis = reinterpret_cast<uint32_t*>(w.res0 + (size_t)ef_pad);
  w.ef_pad = ef_pad; w.hcap = hcap; w.hcap_mask = hcap - 1;
  w.visg = nullptr; w.vis_bytes = 0; w.epoch = 0;
  if constexpr (VISG) { w.visg = visg + (size_t)blockIdx.x * vis_stride; w.vis_bytes = vis_stride; w.epoch = vis_epoch[blockIdx.x]; }
  for (;;) {
    const uint32_t bt = atomicAdd(counter, lane == 0 ? 1u : 0u);  // branch-free, see hnsw_search_kernel
    const uint32_t bi = (uint32_t)__shfl((int)bt, 0, 64);
    if (bi >= count) break;
    const uint32_t vi = base + bi;
    const int lv = levels[bi];
    w.n_dist = w.n_exp = w.n_hops = w.n_resets = 0; w.err = 0;
    wave_sync();
    {  // the query is the vertex's own stored row, decoded to f32
      const uint8_t* row = g.rows + (size_t)vi * g.stride;
      for (int e = lane; e < g.dim; e += 64) {
        if constexpr (R8) w.qs[e] = load1<QUANT>(row, r8_index<QUANT>(e)); else w.qs[e] = load1<QUANT>(row, e);
      }
    }
    w.qnorm = METRIC == M_COS ? g.norms[vi] : 0.f;
    wave_sync();
    uint32_t cur = (uint32_t)entry;
    float curd = eval_pair<METRIC, QUANT, PROF_BUILD, R8>(g, w, cur, lane & 1);
    curd = __shfl(curd, 0, 64);
    w.n_dist += 1;
    for (int l = entry_level; l > lv; l--) greedy_level<METRIC, QUANT, PROF_BUILD, R8>(g, w, cur, curd, l, lane);
    for (int l = entry_level < lv ? entry_level : lv; l >= 0; l--) {
      uint32_t len; int buf;
      w.n_dist += 1;
      search_level<METRIC, QUANT, VISG, PROF_BUILD, R8>(g, w, cur, curd, efc, l, lane, len, buf);
      const unsigned long long* res = w.res0 + (size_t)buf * ef_pad;
      uint32_t m = len < M ? len : M;
      if (diverse) {
        // algo 2 — NOT reference behaviour; the oracle's select_diverse (coltt_oracle.cpp) is the definition: walk the result set in
        // ascending (distance, slot) order while fewer than M are chosen; a candidate is chosen iff no already chosen r has
        // D(candidate as the query, r) < d(new vertex, candidate); every chosen r is evaluated (lane pair per r, side by side).
        uint32_t ns = 0, np = 0;
        for (uint32_t ci = 0; ci < len && ns < M; ci++) {
          const int ln = opaque_lane(lane);
          const int half = ln & 1, p = ln >> 1;
          const unsigned long long ce = res[ci];
          const uint32_t es = (uint32_t)ce >> 1;
          const float ed = __uint_as_float((uint32_t)(ce >> 32));
          bool bad = false;
          if (ns) {
            const uint8_t* crow = g.rows + (size_t)es * g.stride;
            for (int t = ln; t < g.dim; t += 64) {
              if constexpr (R8) qs2[t] = load1<QUANT>(crow, r8_index<QUANT>(t)); else qs2[t] = load1<QUANT>(crow, t);
            }
            const float qn2 = METRIC == M_COS ? g.norms[es] : 0.f;
            wave_sync();
            for (uint32_t c0 = 0; c0 < ns; c0 += 32) {
              const uint32_t idx = c0 + (uint32_t)p;
              const bool valid = idx < ns;
              float dd = 0.f;
              if (valid) dd = eval_pair_q<METRIC, QUANT, PROF_BUILD, R8>(g, qs2, qn2, (uint32_t)sel[idx] >> 1, half);
              bad = bad || (valid && half == 0 && dd < ed);
            }
            w.n_dist += ns;
          }
          const bool rejected = __ballot(bad) != 0ull;
          wave_sync();   // every lane is done with qs2 / sel before either is written again
          if (!rejected) { if (ln == 0) sel[ns] = ce; ns++; }
          else if (np < 64u) { if (ln == 0) prn[np] = ce; np++; }   // at most M <= 64 rejected ones can ever be re-added
          wave_sync();
        }
        if (diverse & 2u) {   // heuristicKeepPruned: the rejected, nearest first, fill the row up to M
          for (uint32_t i = 0; i < np && ns < M; i++) { if (lane == 0) sel[ns] = prn[i]; ns++; }
          wave_sync();
        }
        m = ns;
        res = sel;
      }
      // the m nearest (or the m chosen), re-ordered by slot (canonical row order)
      unsigned long long e = (uint32_t)lane < m ? res[lane] : ~0ull;
      uint32_t myslot = (uint32_t)e >> 1;
      float myd = __uint_as_float((uint32_t)(e >> 32));
      uint32_t rank = 0;
      for (uint32_t j = 0; j < m; j++) {
        uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)myslot, (int)j);
        rank += sj < myslot ? 1u : 0u;
      }
      uint32_t width;
      uint32_t* row = const_cast<uint32_t*>(adj_row(g, vi, l, width));
      float* drow = (l == 0 ? g.adj0_d + (size_t)vi * g.mMax0 : g.adjU_d + ((size_t)g.upper_off[vi] + (uint32_t)(l - 1)) * g.mMax);
      const uint32_t rt = atomicAdd(req_count, lane == 0 ? m : 0u);  // branch-free, see hnsw_search_kernel
      const uint32_t r0 = (uint32_t)__shfl((int)rt, 0, 64);
      if ((uint32_t)lane < m) {
        row[rank] = myslot; drow[rank] = myd;
        if (l == 0 && g.adj0_n) g.adj0_n[(size_t)vi * g.mMax0 + rank] = g.norms[myslot];
        if (l == 0 && g.adj0_m) g.adj0_m[(size_t)vi * g.mMax0 + rank] = g.rows_m[myslot];
        uint32_t rid = l == 0 ? myslot : (uint32_t)cap_slots + g.upper_off[myslot] + (uint32_t)(l - 1);
        uint32_t r = r0 + lane;
        uint32_t old = atomicExch(&head[rid], r);
        req[r].rid = rid; req[r].from = vi; req[r].d = myd; req[r].next = old;
      }
      // next level starts from the nearest result (hnsw.go:145 `entrypoint = neighbor`, last popped = nearest; the nearest candidate is
      // always chosen first by the diverse selection, so sel[0] == the result set's first member)
      unsigned long long e0 = res[0];
      cur = (uint32_t)e0 >> 1; curd = __uint_as_float((uint32_t)(e0 >> 32));
      wave_sync();
    }
    if (lane == 0) {
      atomicAdd(&stats[0], (unsigned long long)w.n_dist);
      atomicAdd(&stats[1], (unsigned long long)w.n_exp);
      atomicAdd(&stats[2], (unsigned long long)w.n_hops);
      atomicAdd(&stats[3], (unsigned long long)w.n_resets);
      if (w.err) atomicOr(&stats[4], (unsigned long long)w.err);
    }
  }
  if constexpr (VISG) { if (lane == 0) vis_epoch[blockIdx.x] = w.epoch; }
}

// Phase B: apply the queued links to the neighbours' rows (hnsw.go:151-158: neighbor.addEdge + pruneNeighbors when
// the row exceeds mMax).  Exactly one request per touched row arrived first (next == NONE): its thread owns the
// row.  Closed form of "add one by one, prune on overflow" (order-independent): if existing + added <= width the
// row is the union; otherwise the deleted neighbours are dropped (pruneNeighbors skips them, hnsw.go:454-456) and
// the `width` nearest by (stored distance, slot) are kept (selectNeighbors, :391-397).  Rows stay sorted by slot.
constexpr int LINK_W = 64;    // widest row the builder supports
constexpr int LINK_CH = 64;   // requests merged per round
// dirty (may be NULL): the owner of a LEVEL-0 row appends its slot — the rows whose neighbourhood blocks the host re-gathers afterwards (PqNbrPatch).
__global__ void hnsw_link_kernel(GraphView g, uint64_t cap_slots, const BuildReq* __restrict__ req, uint32_t n_req,
                                 uint32_t* __restrict__ head, uint32_t* __restrict__ dirty, uint32_t dirty_cap) {
  uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_req) return;
  if (req[r].next != NBR_NONE) return;
  const uint32_t rid = req[r].rid;
  const bool lvl0 = rid < cap_slots;
  const uint32_t W = lvl0 ? g.mMax0 : g.mMax;
  uint32_t* row = lvl0 ? g.adj0 + (size_t)rid * g.mMax0 : g.adjU + (size_t)(rid - cap_slots) * g.mMax;
  float* drow = lvl0 ? g.adj0_d + (size_t)rid * g.mMax0 : g.adjU_d + (size_t)(rid - cap_slots) * g.mMax;
  uint32_t s[LINK_W + LINK_CH]; float d[LINK_W + LINK_CH];
  uint32_t n = 0;
  for (; n < W && row[n] != NBR_NONE; n++) { s[n] = row[n]; d[n] = drow[n]; }
  uint32_t cur = head[rid];
  head[rid] = NBR_NONE;
  while (cur != NBR_NONE) {
    uint32_t take = 0;
    while (cur != NBR_NONE && take < LINK_CH) { s[n + take] = req[cur].from; d[n + take] = req[cur].d; cur = req[cur].next; take++; }
    uint32_t tot = n + take;
    if (tot > W) {
      uint32_t m = 0;  // drop tombstoned neighbours
      for (uint32_t i = 0; i < tot; i++) if (!is_deleted(g, s[i])) { s[m] = s[i]; d[m] = d[i]; m++; }
      // insertion sort by (d, slot)
      for (uint32_t i = 1; i < m; i++) {
        uint32_t si = s[i]; float di = d[i]; uint32_t j = i;
        while (j > 0 && (d[j - 1] > di || (d[j - 1] == di && s[j - 1] > si))) { s[j] = s[j - 1]; d[j] = d[j - 1]; j--; }
        s[j] = si; d[j] = di;
      }
      n = m < W ? m : W;
    } else n = tot;
  }
  for (uint32_t i = 1; i < n; i++) {  // back to canonical slot order
    uint32_t si = s[i]; float di = d[i]; uint32_t j = i;
    while (j > 0 && s[j - 1] > si) { s[j] = s[j - 1]; d[j] = d[j - 1]; j--; }
    s[j] = si; d[j] = di;
  }
  for (uint32_t i = 0; i < W; i++) { row[i] = i < n ? s[i] : NBR_NONE; drow[i] = i < n ? d[i] : 0.f; }
  if (lvl0 && g.adj0_n) {
    float* nrow = g.adj0_n + (size_t)rid * g.mMax0;
    for (uint32_t i = 0; i < W; i++) nrow[i] = i < n ? g.norms[s[i]] : 0.f;
  }
  if (lvl0 && g.adj0_m) {
    float2* mrow = g.adj0_m + (size_t)rid * g.mMax0;
    for (uint32_t i = 0; i < W; i++) mrow[i] = i < n ? g.rows_m[s[i]] : float2{0.f, 0.f};
  }
  if (lvl0 && dirty) { const uint32_t di = atomicAdd(&dirty[0], 1u); if (di < dirty_cap) dirty[2 + di] = rid; }
}

// Phase B of the diverse mode (algo 2 — NOT reference behaviour; definition: the oracle's select_diverse + the batch rule of
// hnsw_insert_batch): a row receives ALL the batch's links and is pruned ONCE if it overflows — drop the tombstoned neighbours; if the
// live ones still do not fit, walk them in ascending (stored distance, slot) order and choose a candidate iff no already chosen r has
// D(candidate's stored row as the query, r's stored row) < the candidate's stored distance, until W are chosen; keepPruned re-adds the
// rejected, nearest first.  One WAVE per touched row (the owner request's wave; the others leave at once): candidates in LDS, the
// candidate under test decoded into LDS as a query, the chosen rows evaluated side by side by lane pairs — the builder's own distance code.
constexpr uint32_t LINKD_CAND = 1024;   // candidates per row (existing + the batch's links); more trips stats[4] |= 16 (lower the batch size)
template <int METRIC, int QUANT, bool R8>
__global__ __launch_bounds__(64) void hnsw_link_diverse_kernel(GraphView g, uint64_t cap_slots, const BuildReq* __restrict__ req, uint32_t n_req,
                                                              uint32_t* __restrict__ head, uint32_t keep_pruned,
                                                              unsigned long long* __restrict__ stats, uint32_t* __restrict__ dirty, uint32_t dirty_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t r = blockIdx.x;
  if (r >= n_req) return;
  if (req[r].next != NBR_NONE) return;
  const int lane_in = threadIdx.x;
  const size_t off = ((size_t)g.dim * 4 + 15) & ~(size_t)15;
  float* const qs2 = reinterpret_cast<float*>(smem);
  unsigned long long* const cand = reinterpret_cast<unsigned long long*>(smem + off);   // [LINKD_CAND] as gathered
  unsigned long long* const sorted = cand + LINKD_CAND;                                  // [LINKD_CAND] ascending (d bits, slot)
  unsigned long long* const sel = sorted + LINKD_CAND;                                   // [64] chosen
  unsigned long long* const prn = sel + 64;                                              // [64] rejected (first W of them)
  const uint32_t rid = req[r].rid;
  const bool lvl0 = rid < cap_slots;
  const uint32_t W = lvl0 ? g.mMax0 : g.mMax;
  uint32_t* row = lvl0 ? g.adj0 + (size_t)rid * g.mMax0 : g.adjU + (size_t)(rid - cap_slots) * g.mMax;
  float* drow = lvl0 ? g.adj0_d + (size_t)rid * g.mMax0 : g.adjU_d + (size_t)(rid - cap_slots) * g.mMax;
  int lane = lane_in;
  // ---- gather: the row's entries, then the chained requests (the chain is short: one lane walks it)
  uint32_t n = 0;
  {
    const uint32_t sl = (uint32_t)lane < W ? row[lane] : NBR_NONE;
    const float dl = (uint32_t)lane < W ? drow[lane] : 0.f;
    const unsigned long long have = __ballot(sl != NBR_NONE);
    if (sl != NBR_NONE) cand[__popcll(have & ((1ull << lane) - 1ull))] = ((unsigned long long)__float_as_uint(dl) << 32) | sl;
    n = (uint32_t)__popcll(have);
  }
  uint32_t tot = n;
  if (lane == 0) {
    uint32_t cur = head[rid];
    head[rid] = NBR_NONE;
    while (cur != NBR_NONE) {
      if (tot < LINKD_CAND) cand[tot] = ((unsigned long long)__float_as_uint(req[cur].d) << 32) | req[cur].from;
      tot++;
      cur = req[cur].next;
    }
  }
  tot = (uint32_t)__shfl((int)tot, 0, 64);
  if (tot > LINKD_CAND) { if (lane == 0) atomicOr(&stats[4], 16ull); return; }   // the host fails the batch loudly
  wave_sync();
  uint32_t ns;            // entries of the new row, in sel[]
  if (tot <= W) {
    for (uint32_t i = lane; i < tot; i += 64) sel[i] = cand[i];
    ns = tot;
  } else {
    // drop the tombstoned neighbours (pruneNeighbors skips them, hnsw.go:454-456), rank-sort the live ones by key
    uint32_t live = 0;
    for (uint32_t b = 0; b < tot; b += 64) {
      const uint32_t i = b + lane;
      const unsigned long long k = i < tot ? cand[i] : ~0ull;
      const bool ok = i < tot && !is_deleted(g, (uint32_t)k);
      const unsigned long long mk = __ballot(ok);
      wave_sync();   // chunk b has been read by every lane before its front part is overwritten (live <= b)
      if (ok) cand[live + __popcll(mk & ((1ull << lane) - 1ull))] = k;
      live += (uint32_t)__popcll(mk);
      wave_sync();
    }
    for (uint32_t i = lane; i < live; i += 64) {
      const unsigned long long k = cand[i];
      uint32_t rank = 0;
      for (uint32_t j = 0; j < live; j++) rank += cand[j] < k ? 1u : 0u;   // keys are distinct (a slot appears once in a row)
      sorted[rank] = k;
    }
    wave_sync();
    if (live <= W) {
      for (uint32_t i = lane; i < live; i += 64) sel[i] = sorted[i];
      ns = live;
    } else {
      uint32_t nsel = 0, np = 0;
      unsigned long long n_eval = 0;
      for (uint32_t ci = 0; ci < live && nsel < W; ci++) {
        lane = opaque_lane(lane_in);
        const int half = lane & 1, p = lane >> 1;
        const unsigned long long ce = sorted[ci];
        const uint32_t es = (uint32_t)ce;
        const float ed = __uint_as_float((uint32_t)(ce >> 32));
        bool bad = false;
        if (nsel) {
          const uint8_t* crow = g.rows + (size_t)es * g.stride;
          for (int t = lane; t < g.dim; t += 64) {
            if constexpr (R8) qs2[t] = load1<QUANT>(crow, r8_index<QUANT>(t)); else qs2[t] = load1<QUANT>(crow, t);
          }
          const float qn2 = METRIC == M_COS ? g.norms[es] : 0.f;
          wave_sync();
          for (uint32_t c0 = 0; c0 < nsel; c0 += 32) {
            const uint32_t idx = c0 + (uint32_t)p;
            const bool valid = idx < nsel;
            float dd = 0.f;
            if (valid) dd = eval_pair_q<METRIC, QUANT, PROF_BUILD, R8>(g, qs2, qn2, (uint32_t)sel[idx], half);
            bad = bad || (valid && half == 0 && dd < ed);
          }
          n_eval += nsel;
        }
        const bool rejected = __ballot(bad) != 0ull;
        wave_sync();
        if (!rejected) { if (lane == 0) sel[nsel] = ce; nsel++; }
        else if (np < 64u) { if (lane == 0) prn[np] = ce; np++; }
        wave_sync();
      }
      if (keep_pruned) {
        for (uint32_t i = 0; i < np && nsel < W; i++) { if (lane == 0) sel[nsel] = prn[i]; nsel++; }
      }
      if (lane == 0 && n_eval) atomicAdd(&stats[0], n_eval);   // the oracle's n_dist counts these evaluations
      ns = nsel;
    }
  }
  wave_sync();
  // ---- the new row, ascending by slot (ns <= W <= 64: one entry per lane, ranked by readlane broadcasts)
  lane = opaque_lane(lane_in);
  const unsigned long long mine = (uint32_t)lane < ns ? sel[lane] : ~0ull;
  const uint32_t myslot = (uint32_t)mine;
  uint32_t rank = 0;
  for (uint32_t j = 0; j < ns; j++) {
    const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)myslot, (int)j);
    rank += sj < myslot ? 1u : 0u;
  }
  wave_sync();
  float* nrow = (lvl0 && g.adj0_n) ? g.adj0_n + (size_t)rid * g.mMax0 : nullptr;
  float2* mrow = (lvl0 && g.adj0_m) ? g.adj0_m + (size_t)rid * g.mMax0 : nullptr;
  if ((uint32_t)lane < ns) {
    row[rank] = myslot; drow[rank] = __uint_as_float((uint32_t)(mine >> 32));
    if (nrow) nrow[rank] = g.norms[myslot];
    if (mrow) mrow[rank] = g.rows_m[myslot];
  }
  if ((uint32_t)lane >= ns && (uint32_t)lane < W) {
    row[lane] = NBR_NONE; drow[lane] = 0.f;
    if (nrow) nrow[lane] = 0.f;
    if (mrow) mrow[lane] = float2{0.f, 0.f};
  }
  if (lvl0 && dirty && lane == 0) { const uint32_t di = atomicAdd(&dirty[0], 1u); if (di < dirty_cap) dirty[2 + di] = rid; }   // as hnsw_link_kernel
}

// Before the diverse link pass: the longest request chain of the batch (+ the widest row) -> stats[5].  A row that would receive more candidates than the link
// kernel holds makes the host retry the batch in halves BEFORE anything was applied (insert_core): the index stays exactly as it was.
__global__ void hnsw_link_count_kernel(const BuildReq* __restrict__ req, uint32_t n_req, const uint32_t* __restrict__ head, uint64_t cap_slots,
                                       uint32_t mMax0, uint32_t mMax, unsigned long long* __restrict__ stats) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_req || req[r].next != NBR_NONE) return;
  const uint32_t rid = req[r].rid;
  uint32_t c = 0;
  for (uint32_t cur = head[rid]; cur != NBR_NONE; cur = req[cur].next) c++;
  atomicMax(&stats[5], (unsigned long long)(c + (rid < cap_slots ? mMax0 : mMax)));
}

// adj0_n[slot][j] = norms[adj0[slot][j]] (and adj0_m[slot][j] = rows_m[adj0[slot][j]]) for the level-0 rows of slots [first, first + n): after a bulk install of the topology
__global__ void adj_norms_kernel(GraphView g, uint64_t first, uint64_t n) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * g.mMax0) return;
  const uint64_t i = first * g.mMax0 + t;
  const uint32_t nb = g.adj0[i];
  g.adj0_n[i] = nb != NBR_NONE ? g.norms[nb] : 0.f;
  if (g.adj0_m) g.adj0_m[i] = nb != NBR_NONE ? g.rows_m[nb] : float2{0.f, 0.f};
}

__global__ void fill_u32_kernel(uint32_t* p, size_t n, uint32_t v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void add_base_kernel(uint64_t* ids, size_t n, uint64_t base) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ids[i] += base;
}


int prep_rows_any(Hnsw* x, const float* d_raw, uint64_t n, uint64_t slot_base, bool normalize) {
  if (n == 0) return COLTT_OK;
  int nrm = normalize ? 1 : 0;
  uint8_t* R = x->rows.as<uint8_t>();
  float* N = x->norms.as<float>();
  if (x->r8) {   // Normalize + Lower into a natural-order staging block, norms from it (AVX order), then the line transposition into the row array
    COLTT_TRY(x->w_stage.reserve(n * x->stride));
    uint8_t* S = x->w_stage.as<uint8_t>();
    const uint64_t chunks = (uint64_t)x->stride / 16;
    if (x->quant == COLTT_Q_NONE) {
      launch_prep_rows<Q_NONE>(x->stream, d_raw, n, (int)x->dim, nrm, nullptr, 0, S, x->stride);
      row_norms_kernel<Q_NONE><<<ceil_div(n * 2, 256), 256, 0, x->stream>>>(S, x->stride, nullptr, 0, n, (int)x->dim, N + slot_base);
      rows8_permute_kernel<Q_NONE><<<ceil_div(n * chunks, 256), 256, 0, x->stream>>>(S, R + slot_base * x->stride, x->stride, (int)x->dim, n);
      if (x->shadow) {   // the binary16 shadow of the same rows, from the same staging block
        const size_t hs = (size_t)x->dim * 2;
        if (x->rows_h.cap < (slot_base + n) * hs) x->drop_shadow();   // (reserve keeps it as large as `rows`: not reached)
        else rows_shadow_kernel<<<ceil_div(n * (x->dim / 8), 256), 256, 0, x->stream>>>(S, x->stride, x->rows_h.as<uint8_t>() + slot_base * hs, hs, (int)x->dim, n);
      }
      if (x->shadow8) {  // the 8-bit shadow and its (scale, error norm), from the same staging block
        const size_t bs = (size_t)x->dim;
        if (x->rows_b.cap < (slot_base + n) * bs || x->rows_m.cap < (slot_base + n) * 8) x->drop_shadow8();   // (not reached, as above)
        else rows_b_kernel<<<ceil_div(n, 4), 256, 0, x->stream>>>(S, x->stride, x->rows_b.as<uint8_t>() + slot_base * bs, bs, x->rows_m.as<RowMeta8>() + slot_base, (int)x->dim, n);
      }
    } else {
      launch_prep_rows<Q_F16>(x->stream, d_raw, n, (int)x->dim, nrm, nullptr, 0, S, x->stride);
      row_norms_kernel<Q_F16><<<ceil_div(n * 2, 256), 256, 0, x->stream>>>(S, x->stride, nullptr, 0, n, (int)x->dim, N + slot_base);
      rows8_permute_kernel<Q_F16><<<ceil_div(n * chunks, 256), 256, 0, x->stream>>>(S, R + slot_base * x->stride, x->stride, (int)x->dim, n);
    }
    COLTT_HIP(hipGetLastError());
    return COLTT_OK;
  }
#define COLTT_PREP(Q)                                                                                                  \
  do {                                                                                                                 \
    launch_prep_rows<Q>(x->stream, d_raw, n, (int)x->dim, nrm, nullptr, slot_base, R, x->stride);                     \
    row_norms_kernel<Q><<<ceil_div(n * 2, 256), 256, 0, x->stream>>>(R, x->stride, nullptr, slot_base, n, (int)x->dim, N);     \
  } while (0)
  COLTT_DISPATCH_QUANT(x->quant, COLTT_PREP)
#undef COLTT_PREP
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

// stored rows [first, first + m) -> the f32 values the index's distance sees (what the quantiser encodes), packed [m][dim]
template <int QUANT, bool R8>
__global__ void rows_to_f32_kernel(const uint8_t* __restrict__ rows, size_t stride, uint64_t first, uint64_t m, int dim, float* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * (uint64_t)dim) return;
  const uint64_t i = t / dim; const int e = (int)(t - i * dim);
  int pos = e;
  if constexpr (R8) pos = r8_index<QUANT>(e);
  out[t] = load1<QUANT>(rows + (first + i) * stride, pos);
}
// the stored codes of rows [first, first + m) in NATURAL element order, packed [m][dim * elem bytes] (read-backs of a line-transposed index)
template <int QUANT>
__global__ void rows_natural_kernel(const uint8_t* __restrict__ rows, size_t stride, uint64_t first, uint64_t m, int dim, uint8_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * (uint64_t)dim) return;
  const uint64_t i = t / dim; const int e = (int)(t - i * dim);
  const uint8_t* row = rows + (first + i) * stride;
  const int pos = r8_index<QUANT>(e);
  if constexpr (QUANT == Q_NONE) reinterpret_cast<uint32_t*>(out)[t] = reinterpret_cast<const uint32_t*>(row)[pos];
  else reinterpret_cast<unsigned short*>(out)[t] = reinterpret_cast<const unsigned short*>(row)[pos];
}
// codes of the slots added since the last call (hnsw_pq.hpp); completes on the device before it returns
int sync_pq(Hnsw* x) {
  if (!x->pq_on || x->pq_done >= x->n) { if (x->pq_done > x->n) x->pq_done = x->n; return COLTT_OK; }
  const size_t old = x->pq_codes.cap;
  COLTT_TRY(x->pq_codes.reserve(std::max<uint64_t>(x->cap, x->n) * x->pq_row, true, x->stream));
  if (x->pq_codes.cap > old) COLTT_HIP(hipMemsetAsync(x->pq_codes.as<uint8_t>() + old, 0, x->pq_codes.cap - old, x->stream));   // the bytes j >= m of a row read as code 0
  const uint64_t chunk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)x->dim * 4));
  COLTT_TRY(x->pq_stage.reserve(std::min<uint64_t>(chunk, x->n - x->pq_done) * x->dim * 4));
  for (uint64_t b = x->pq_done; b < x->n; b += chunk) {
    const uint64_t m = std::min<uint64_t>(chunk, x->n - b);
    if (x->quant == COLTT_Q_NONE) {
      if (x->r8) rows_to_f32_kernel<Q_NONE, true><<<ceil_div(m * x->dim, 256), 256, 0, x->stream>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, x->pq_stage.as<float>());
      else rows_to_f32_kernel<Q_NONE, false><<<ceil_div(m * x->dim, 256), 256, 0, x->stream>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, x->pq_stage.as<float>());
    } else {   // (attach refuses "f8" rows)
      if (x->r8) rows_to_f32_kernel<Q_F16, true><<<ceil_div(m * x->dim, 256), 256, 0, x->stream>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, x->pq_stage.as<float>());
      else rows_to_f32_kernel<Q_F16, false><<<ceil_div(m * x->dim, 256), 256, 0, x->stream>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, x->pq_stage.as<float>());
    }
    COLTT_HIP(hipGetLastError());
    COLTT_TRY(pq_encode_rowmajor(x->stream, x->pq_cb.as<float>(), x->pq_shape, x->pq_stage.as<float>(), m, x->pq_codes.as<uint8_t>() + b * x->pq_row, x->pq_row));
  }
  COLTT_HIP(hipStreamSynchronize(x->stream));
  x->pq_done = x->n;
  return COLTT_OK;
}
// does this shape have a rows8 copy (rows8.hpp: f32 / 2-byte rows whose byte length is a multiple of 128)?
bool rows8_shape(uint32_t dim, int quant) {
  const int pol = policy().rows8;
  if (quant == COLTT_Q_F8 || pol == 0) return false;
  // Short rows stay on the lane pairs: the eight-lane core pays a fixed LDS hand-off per chunk of neighbours, which a 128-element row does
  // not amortise (1 M x 128 f32, ef 20 — the reference's published point: 1.41 ms per 10 k queries against 1.17, one query 0.130 against
  // 0.103 ms; 2 M x 256 f16, ef 64: 4.24 against 5.17 ms, +22 % — profiles/r04h_ev8_short_rows.json).  COLTT_ROWS8=2 lifts the limit.
  if (pol == 1 && dim < 256) return false;
  return ((size_t)dim * quant_bytes(quant)) % 128 == 0;
}

}  // namespace

namespace coltt {
namespace hnsw {
int prep_queries_any(Hnsw* x, HCtx* c, const float* d_qraw, size_t nq, uint32_t* zero64) {
  COLTT_TRY(c->w_qeff.reserve(nq * x->dim * 4));
  COLTT_TRY(c->w_qn.reserve(nq * 4));
  int norm = x->metric == COLTT_COSINE;
  float* qe = c->w_qeff.as<float>();
#define COLTT_PQ(Q) launch_prep_queries<Q>(c->stream, d_qraw, nq, (int)x->dim, norm, qe, c->w_qn.as<float>(), zero64)
  COLTT_DISPATCH_QUANT(x->quant, COLTT_PQ)
#undef COLTT_PQ
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}
void add_base(hipStream_t stream, uint64_t* ids, size_t n, uint64_t base) { add_base_kernel<<<ceil_div(n, 256), 256, 0, stream>>>(ids, n, base); }
}  // namespace hnsw
}  // namespace coltt

namespace {
uint32_t next_pow2(uint32_t v) { uint32_t p = 1; while (p < v) p <<= 1; return p; }

#ifndef COLTT_VISG_MIN_EF
#define COLTT_VISG_MIN_EF 128
#endif
constexpr uint32_t VIS_MAX_REGIONS = 3072;  // 12 waves on each of 256 CUs: the product-quantised walk (3 per SIMD)
constexpr uint32_t VIS_ROW_REGIONS = 2048;  // 8 waves per CU: the row walks and the builder

}  // namespace

namespace coltt {
namespace hnsw {
// (Re)allocate the HBM visited set for the current slot capacity: one byte per slot and workgroup, zeroed, epochs reset.
// Sized against a quarter of the device memory; if that buys fewer than one region per CU the LDS hash is used instead.
int ensure_visg(Hnsw* x, const Policy& pol) {
  // Callers hold the index lock (shared or exclusive).  The slot capacity only changes under the exclusive lock, and every
  // search that wants the byte map passes through here first, so a re-allocation can never race a traversal that uses it.
  std::lock_guard<std::mutex> vg(x->vis_mu);
  const uint64_t stride = (std::max<uint64_t>(x->cap, 1) + 1023) & ~1023ull;
  // the row walks keep at most 8 traversals per CU (2048 regions); the product-quantised walk fits up to 12 (3072): only an index that carries a
  // quantiser pays for those (10 M slots x 3072 regions pinned 30 GB instead of 20 for everybody)
  const uint32_t want_max = x->pq_on ? VIS_MAX_REGIONS : VIS_ROW_REGIONS;
  if (x->vis_stride == stride && x->vis_want == want_max) return COLTT_OK;
  if (x->w_visg.p) { (void)hipFree(x->w_visg.p); x->w_visg.p = nullptr; x->w_visg.cap = 0; }
  size_t free_b = 0, total_b = 0;
  COLTT_HIP(hipMemGetInfo(&free_b, &total_b));
  uint64_t budget = std::min<uint64_t>(total_b / 4, free_b / 2);
  if (pol.visg_budget_mb >= 0) budget = std::min<uint64_t>(budget, (uint64_t)pol.visg_budget_mb << 20);  // test knob
  const uint64_t regions = std::min<uint64_t>(want_max, budget / stride);
  x->vis_stride = stride; x->vis_want = want_max;
  x->vis_regions = 0;
  x->vis_busy.clear();
  if (regions < 256) {
    fprintf(stderr, "[coltt_gpu] hnsw: HBM visited workspace would get only %llu regions of %llu B (budget %llu B) — using the LDS hash "
                    "visited set for ef > %d as well\n", (unsigned long long)regions, (unsigned long long)stride, (unsigned long long)budget, COLTT_VISG_MIN_EF);
    return COLTT_OK;
  }
  if (regions < want_max)
    fprintf(stderr, "[coltt_gpu] hnsw: HBM visited workspace capped at %llu of %u regions (%llu B each, budget %llu B): fewer resident "
                    "traversals per launch\n", (unsigned long long)regions, want_max, (unsigned long long)stride, (unsigned long long)budget);
  COLTT_TRY(x->w_visg.reserve(regions * stride));
  COLTT_TRY(x->w_vepoch.reserve(VIS_MAX_REGIONS * 4));
  COLTT_HIP(hipMemsetAsync(x->w_visg.p, 0, regions * stride, x->stream));
  COLTT_HIP(hipMemsetAsync(x->w_vepoch.p, 0, VIS_MAX_REGIONS * 4, x->stream));
  COLTT_HIP(hipStreamSynchronize(x->stream));  // searches run on other streams
  x->vis_regions = (uint32_t)regions;
  x->vis_busy.assign(regions, 0);
  return COLTT_OK;
}

void acquire_regions(Hnsw* x, uint32_t want, RegionLease& out) {
  std::unique_lock<std::mutex> lk(x->vis_mu);
  const uint32_t R = (uint32_t)x->vis_busy.size();
  if (want > R) want = R;
  for (;;) {
    uint32_t best_b = 0, best_l = 0;
    for (uint32_t i = 0; i < R;) {
      if (x->vis_busy[i]) { i++; continue; }
      uint32_t j = i; while (j < R && !x->vis_busy[j] && j - i < want) j++;
      if (j - i > best_l) { best_l = j - i; best_b = i; }
      if (best_l == want) break;
      i = j;
    }
    if (best_l > 0) {
      for (uint32_t i = 0; i < best_l; i++) x->vis_busy[best_b + i] = 1;
      out.x = x; out.base = best_b; out.count = best_l;
      return;
    }
    x->vis_cv.wait(lk);
  }
}
}  // namespace hnsw
}  // namespace coltt

// ---- The search plan: which kernel one coltt_hnsw_search call launches, and how.  Pure functions of (PlanFacts, Policy): no HIP call, no Hnsw, no
// environment.  search_common takes one policy() snapshot and calls plan_search once; coltt_hnsw_search_plan_host runs the same code with no device.
// DESIGN.md ("The search plan") has the decision table in one place.
namespace coltt {
namespace hnsw {
PlanFacts plan_facts(const Hnsw* x) {
  PlanFacts f{};
  f.dim = x->dim; f.metric = x->metric; f.quant = x->quant; f.m_max0 = (uint32_t)x->cfg.m_max0; f.stride = x->stride; f.slots = x->n;
  f.r8 = x->r8; f.shadow8 = x->has_shadow8(); f.shadow16 = x->has_shadow16();
  f.vis_ready = x->vis_stride != 0 && x->vis_regions > 0; f.vis_regions = x->vis_regions;
  return f;
}

// COLTT_VISG=0 / 1 forces the LDS hash / the HBM byte map (measurement and test knob, read at every call); default: the
// byte map above ef 128.  Measured on 10 M x 768 f16 (lowrank:32), queries/s LDS hash -> byte map: ef 128 728 k -> 724 k,
// ef 256 246 k -> 404 k, ef 512 62 k -> 212 k, ef 1024 25 k -> 105 k; build (efConstruction 200) 36 s -> 22 s.
bool wants_visg(const Policy& pol, uint32_t ef) { return pol.visg < 0 ? ef > COLTT_VISG_MIN_EF : pol.visg != 0; }

// The one-wave walk's LDS: query + `extra` bytes + result set (merged in place) + the visited set.
static SearchGeom row_walk_lds(const PlanFacts& f, const Policy& pol, uint32_t ef, size_t extra) {
  SearchGeom s;
  s.ef = ef;
  s.ef_pad = (ef + 63) & ~63u;
  const size_t fixed = (((size_t)f.dim * 4 + 15) & ~(size_t)15) + extra + (size_t)s.ef_pad * 8;
  // LDS visited set: sized so that a typical traversal (a few dozen evaluations per result slot) never resets
  s.hcap = std::min<uint32_t>(32768u, std::max<uint32_t>(8192u, next_pow2(ef * 48u)));
  // large ef x dim: shrink it until the wave's state fits the CU's 160 KiB (the reset-and-reseed path keeps results exact;
  // it needs 0.75 * hcap > ef + 64)
  while (fixed + (size_t)s.hcap * 4 > 160 * 1024 && s.hcap > 4096 && (s.hcap / 2) * 3 / 4 > ef + 64) s.hcap /= 2;
  s.visg = wants_visg(pol, ef) && f.vis_ready;
  if (s.visg) { s.hcap = 64; s.lds = fixed; s.max_grid = f.vis_regions; }
  else { s.lds = fixed + (size_t)s.hcap * 4; s.max_grid = 0xffffffffu; }
  return s;
}
SearchGeom walk_geom(const PlanFacts& f, const Policy& pol, uint32_t ef, uint32_t allowed) { return row_walk_lds(f, pol, ef, (size_t)((allowed + 63) & ~63u) * 8); }

// Resident waves per CU.  2-byte rows want all 8 (two per SIMD); f32 rows are faster with 4: eight 3-KB-per-row streams per
// CU measured slower both in search (ef 256: 160 k vs 197 k q/s) and in the 10 M build (61 s vs 50 s).  COLTT_WAVES_PER_CU
// overrides (measurement knob).
static size_t waves_per_cu_cap(const Policy& pol, int quant) { return pol.waves_per_cu > 0 ? (size_t)pol.waves_per_cu : (quant == Q_NONE ? 4 : 8); }
// The walk over the 16-bit visited set is compiled for two waves per SIMD and its LDS fits seven times: all seven (COLTT_WAVES_PER_CU overrides here too).
#ifndef COLTT_VIS16_WAVES_PER_CU
#define COLTT_VIS16_WAVES_PER_CU 7
#endif
uint32_t resident_waves(const Policy& pol, int quant, size_t lds, int w2, bool vis16) {
  const size_t cap = (w2 >= 0 && (w2 & 8)) ? 4 : (vis16 && pol.waves_per_cu <= 0) ? (size_t)COLTT_VIS16_WAVES_PER_CU : waves_per_cu_cap(pol, quant);
  return 256u * (uint32_t)std::max<size_t>(1, std::min<size_t>(cap, (160 * 1024) / lds));
}

// Non-temporal row loads for the eight-lane walks (exact.hpp: row_ld): worth it when the row array is far larger than L2 + MALL, costly when later queries
// would have found the rows there.  COLTT_ROWS_NT = 0 / 1 forces, COLTT_ROWS_NT_MIN_MB moves the threshold (default 12 GiB of rows: 768-d rows, same box — f16 0.5 M -24 %, 1 M -10 %,
// 2 M -2 %, 4 M +0.8 %, 10 M +-0; f32 1 M -4 %, 3 M +0.7 %, 10 M +4.5 %: profiles/r06ag_nt_rows_ab.md).
static bool rows_far_larger_than_caches(const PlanFacts& f, const Policy& pol) { return (unsigned long long)f.slots * (unsigned long long)f.stride >= ((unsigned long long)pol.rows_nt_min_mb << 20); }
static bool rows_nt(const PlanFacts& f, const Policy& pol) { return pol.rows_nt >= 0 ? pol.rows_nt != 0 : rows_far_larger_than_caches(f, pol); }
// The certified row filter of the eight-lane f32 cosine walks (hnsw_walk2.hpp: Group8FilterEval).  COLTT_ROW_FILTER = 0 / 1 forces (read per call: one index in
// one process runs both kernels, tools/row_filter_ab.py); unset: on for the LDS-hash walk (ef <= 128, the measured instance: 10 M x 768, ef 128, 1.41 x in one
// process, profiles/r07a_row_filter.md) where the row array is far larger than the caches: every row read is then an HBM read and the kernel sits at what the
// memory system delivers, so bytes are time.
// COLTT_ROW_FILTER_BITS = 8 / 16 / 8i picks the shadow a filtered launch reads; unset: the 8-bit one where the index keeps it.  An index keeps
// what COLTT_ROW_SHADOW_BITS said when it was created; the kind it does not keep is served by the one it does.  8i (ROW_FILTER_8I) reads the 8-bit shadow
// against the query quantised once per traversal: phase A is an integer sum (row_filter8i.hpp); it is what an unset knob takes over the 8-bit shadow
// (COLTT_ROW_FILTER8I_DEFAULT; the measurement behind it: profiles/r10a_row_filter8i.md).
#ifndef COLTT_ROW_FILTER8I_DEFAULT
#define COLTT_ROW_FILTER8I_DEFAULT 1
#endif
// the shadow an eight-lane f32 cosine launch filters through (16, 8, ROW_FILTER_8I), 0 = no filter
static int row_filter_kind(const PlanFacts& f, const Policy& pol, bool vis_hbm) {
  const bool h8 = f.shadow8 != 0, h16 = f.shadow16 != 0;
  if (!h8 && !h16) return 0;
  // unset and over the HBM map: off — the ef > 128 twins have not been timed against their unfiltered partners: COLTT_ROW_FILTER=1 only.  Unset otherwise:
  // the SIZE rule of the non-temporal hint (not its forcing knob COLTT_ROWS_NT: an A/B of the hint must not toggle the filter too).  The threshold is
  // inherited from that rule's measured crossover, the filter's own crossover on 1 M / 3 M has not been measured.
  if (!(pol.row_filter >= 0 ? pol.row_filter != 0 : (!vis_hbm && rows_far_larger_than_caches(f, pol)))) return 0;
  const int want = pol.row_filter_bits;
  if (want == 16) return h16 ? 16 : 8;
  if (want == 8) return h8 ? 8 : 16;
  if (want == ROW_FILTER_8I) return h8 ? ROW_FILTER_8I : 16;
  return h8 ? (COLTT_ROW_FILTER8I_DEFAULT ? ROW_FILTER_8I : 8) : 16;
}
// What the prologue of a row-filter launch does unless COLTT_DESCENT_NT / COLTT_ROW_FILTER_UPPER say otherwise.  Measured on 10 M x 768, ef 128, 10 000 queries
// per launch, four sides alternating in one process (tools/descent_filter_ab.py; profiles/r12a_descent_filter.md): cacheable descent loads 9.06 -> 8.76 ms
// (+3.4 %); the filtered descent on top of them 8.80 ms — it rejects 90 % of the 116 evaluations above level 0 and asks for a third of the bytes, but with the
// top of the graph served from cache those bytes were no longer HBM's, and a hop now waits for two dependent phases instead of one.
constexpr bool DESCENT_NT_DEFAULT = false;         // the entrypoint's and the descent's rows are loaded cacheable: every query of a launch reads them
constexpr bool ROW_FILTER_UPPER_DEFAULT = false;   // the greedy descent evaluates every listed neighbour exactly

// Which level-0 walk serves the HBM-visited searches.  COLTT_WALK2=off: hnsw_dev.hpp:search_level (the round-2 kernel);
// COLTT_WALK2=<n>: hnsw_walk2.hpp with OPT = n (1 Bloom, 2 delta result set, 4 adjacency-carried norms); the library carries 6 and 7.
// Measurement and test knob, read at every call.
#ifndef COLTT_WALK2_DEFAULT
#define COLTT_WALK2_DEFAULT 7
#endif
// The walk of the LDS-visited searches (ef <= 128 by default).  COLTT_WALK2_LDS=off: hnsw_dev.hpp:search_level; 2 / 4 / 6: hnsw_walk2.hpp
// with the delta result set / adjacency-carried norms / both.  A traversal that would overflow the hash table re-runs the call on
// search_level (which re-seeds the table from the result set) — never seen on the benchmark collections.
// 10 M x 768 f32, 10 000 queries, ms per launch (profiles/r03_walk_lds_f32_10m.json): ef 128 off 22.39, 2 22.25, 4 21.19, 6 21.28;
// ef 64 off 11.80, 2 11.77, 4 11.10, 6 11.25 — the norms riding with the adjacency rows are the gain; the delta set costs a little
// when the whole result set is two 64-entry chunks.  The library carries 4.
#ifndef COLTT_WALK2_LDS_DEFAULT
#define COLTT_WALK2_LDS_DEFAULT 4
#endif
// Batches of at most COLTT_LAT_MAX_NQ queries (default below; COLTT_MW_MAX_NQ is the round-2 name of the knob) take the
// 256-thread latency kernel (hnsw_lat.hpp).
// Measured at 10 M x 768 f32, ef 128 (profiles/r03_latency.json): 1 query 1.04 ms against 1.43 ms on the one-wave kernel, 128 queries
// 1.45 against 1.97 ms; beyond ~256 queries every CU already holds a workgroup and the one-wave kernel's 1024+ resident traversals win.
#ifndef COLTT_LAT_MAX_NQ_DEFAULT
#define COLTT_LAT_MAX_NQ_DEFAULT 256
#endif
#ifndef COLTT_LAT_MIN_STRIDE
#define COLTT_LAT_MIN_STRIDE 1024   // bytes per stored row below which a lane pair streams the whole row in one burst anyway
#endif

// force: 1 = not the latency kernel, 2 = not the walk2 LDS-hash kernel (both after an err 8).  ef: the call's or the index's; the plan's is max(ef, k).
int plan_search(const PlanFacts& f, const Policy& pol, size_t nq, uint32_t k, uint32_t ef, int force, SearchPlan& s) {
  s = SearchPlan{};
  if (k == 0) return fail(COLTT_E_INVALID, "hnsw_search: k must be >= 1");
  ef = std::max(ef, k);  // gomath.MaxInt(ef, k), hnsw.go:258
  if (ef > 4096) return fail(COLTT_E_UNSUPPORTED, "hnsw_search: ef=%u > 4096", ef);
  const bool hbm = wants_visg(pol, ef) && f.vis_ready;
  // The walk: hnsw_walk2.hpp over the HBM map (COLTT_WALK2) or over the LDS hash (small ef: delta result set, adjacency-carried norms; no Bloom filter —
  // the hash is on chip), else the one-wave walk.
  int w2 = -1;
  if (f.m_max0 <= 1024) {
    if (hbm) w2 = pol.walk2 == 7 ? COLTT_WALK2_DEFAULT : pol.walk2;
    else if (!(force & 2)) w2 = pol.walk2_lds == 4 ? COLTT_WALK2_LDS_DEFAULT : pol.walk2_lds;
  }
  // eight lanes per row (rows8.hpp): a second, permuted copy of the query and 96 words of scratch per wave.  Served by the shipped
  // walk2 variants only (LDS hash: 4; HBM map: 6 / 7).  COLTT_EV8=0: level-0 distances from the pair-owned rows even when the index carries the
  // line-transposed copy (A/B and test knob)
  const bool ev8 = f.r8 && f.slots > 0 && pol.ev8 && walk2_shipped(hbm, w2);
  const int filter = ev8 && f.metric == COLTT_COSINE && f.quant == COLTT_Q_NONE ? row_filter_kind(f, pol, hbm) : 0;
  // the row filter over the quantised query (row_filter8i.hpp): two planes of dim signed bytes per wave behind the scratch (hnsw_kernels.hpp:
  // hnsw_search2_rowfilter_kernel).  768-d, ef 128: 4 x (37 248 + 1 536) = 155 136 bytes per CU, four traversals still fit.
  const SearchGeom g = w2 < 0 ? walk_geom(f, pol, ef) : row_walk_lds(f, pol, ef, (ev8 ? 96 * 4 : 0) + (filter == ROW_FILTER_8I ? (size_t)f.dim * 2 : 0));
  s.family = w2 >= 0 ? COLTT_PLAN_WALK2 : COLTT_PLAN_ONE_WAVE;
  s.ef = g.ef; s.ef_pad = g.ef_pad; s.hcap = g.hcap; s.lds = g.lds; s.vis_kind = hbm ? 0 : 32; s.w2 = w2; s.r8 = f.r8 && f.quant != COLTT_Q_F8;
  s.ev8 = ev8; s.filter = filter;
  if (hbm && w2 >= 0 && (w2 & 1)) {
    // Bloom filter: the largest power of two that keeps the profile's resident waves (>= 2 KiB, <= 32 KiB), else none
    const size_t budget = (160 * 1024) / ((w2 & 8) ? 4 : waves_per_cu_cap(pol, f.quant));
    size_t kb = 32;
    if (pol.bloom_kb > 0) kb = (size_t)pol.bloom_kb;
    else while (kb >= 2 && g.lds + kb * 1024 > budget) kb >>= 1;
    size_t p2 = 1; while (p2 * 2 <= kb) p2 *= 2;   // power of two
    if (kb >= 2 && g.lds + p2 * 1024 <= 160 * 1024) { s.bloom_words = (uint32_t)(p2 * 256); s.lds = g.lds + p2 * 1024; }
    else s.w2 &= ~1;
  }
  // The headline walk (LDS variant 4, eight-lane core, row filter over the quantised query) keeps its visited set at 16 bits per entry (vis16.hpp) where every
  // slot is representable: query + scratch + digit planes + result set + 16 KiB + the stash = 22 464 bytes at 768-d, ef 128 — SEVEN traversals per CU where the
  // 32-bit table (38 784 bytes) held four.  The capacity rule is the 32-bit table's: 3/4 of 8 192 entries.  COLTT_VIS16=0 keeps the 32-bit table (per call).
  // COLTT_VIS16_BUCKET_BITS (test knob) shrinks the table to 2^bits buckets and lifts the capacity rule, so that a small walk fills buckets, uses the stash and
  // overflows it.
  if (filter == ROW_FILTER_8I && !hbm && pol.vis16 && ef <= 128) {   // (a filter over the LDS hash: variant 4 with the eight-lane core)
    const uint32_t bits = pol.vis16_bucket_bits > 0 ? (uint32_t)pol.vis16_bucket_bits : VIS16_BUCKET_BITS;
    if (f.slots <= ((uint64_t)1 << (VIS16_TAG_BITS + bits))) {
      s.vis_kind = 16; s.v16_bits = bits;
      s.v16_limit = pol.vis16_bucket_bits > 0 ? 0xffffffu : ((8u << bits) >> 2) * 3;
      s.lds = g.lds - (size_t)g.hcap * 4 + (size_t)vis16_table_words(bits) * 4 + VIS16_STASH * 4;
    }
  }
  if (s.lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "hnsw_search: dim/ef need %zu B of LDS (> 160 KiB)", (size_t)s.lds);
  // latency kernel for small batches.  Its LDS hash must never need the reset path, so it gets the largest table that fits beside the
  // staging area (one workgroup per CU); if even that is too small for this ef the one-wave kernel (or the walk above) serves the call.
  if (nq <= (pol.lat_knob_set ? pol.lat_max_nq : (uint32_t)COLTT_LAT_MAX_NQ_DEFAULT) && !(force & 1) &&
      f.stride <= LAT_MAX_STRIDE /* else: rows too long to hold (or stage) 32 at a time */ &&
      (f.stride >= COLTT_LAT_MIN_STRIDE || pol.lat_knob_set) /* short rows: not the latency kernel (unless asked for) */) {
    // LDS: query + result set + exchange words + the staging area (32 padded rows) + the visited hash
    // (line-transposed rows are evaluated out of the registers they land in: no staging area — hnsw_lat.hpp: lat_eval_chunk, TP != 0)
    const size_t fixed = ((lat_q_floats((int)f.dim) * 4 + 15) & ~(size_t)15) + (size_t)s.ef_pad * 8 + sizeof(LatShared) + (s.r8 ? (size_t)0 : (size_t)LAT_ROWS * (f.stride + LAT_PAD));
    uint32_t hcap = 32768; while (fixed + (size_t)hcap * 4 > 160 * 1024 && hcap > 1024) hcap /= 2;
    if (fixed + (size_t)hcap * 4 <= 160 * 1024 && (hcap / 4) * 3 >= ef * 34u + 64u) {   // else: table too small to be sure
      SearchPlan m{};
      m.family = COLTT_PLAN_LATENCY; m.ef = s.ef; m.ef_pad = s.ef_pad; m.hcap = hcap; m.lds = fixed + (size_t)hcap * 4; m.vis_kind = 32; m.w2 = -1; m.r8 = s.r8;
      m.rows8_launch = s.r8;   // the latency kernel reads the index's ONE row array in the layout it has: COLTT_EV8 does not choose here
      // COLTT_LAT_SEQ=1: the sequential walk (search_level2 + LatEval) also for one-chunk rows — the A/B partner of the pipelined one.  COLTT_LAT_HELPERS =
      // 1 .. 3 helper workgroups per walking one; OFF by default — exact, but 3-5 % slower than no helpers at all (profiles/r06f_latency_helpers_ab.md); not
      // with the sequential walk.
      m.lat_seq = pol.lat_seq || f.m_max0 > 32;
      m.lat_helpers = m.lat_seq ? 0 : std::min(pol.lat_helpers, LAT_HELPERS_MAX);
      m.per_cu = 1; m.grid = std::min<uint32_t>((uint32_t)nq, 256u);
      s = m;
      return COLTT_OK;
    }
  }
  if (s.family == COLTT_PLAN_WALK2) {
    s.nt = ev8 && rows_nt(f, pol);
    if (filter) {   // (the binary16 kind has no per-slot (scale, error norm): its descent stays exact)
      if (filter != 16 && (pol.row_filter_upper >= 0 ? pol.row_filter_upper != 0 : ROW_FILTER_UPPER_DEFAULT)) s.upper |= ROWF_UPPER_FILTER;
      if (s.nt && (pol.descent_nt >= 0 ? pol.descent_nt == 0 : !DESCENT_NT_DEFAULT)) s.upper |= ROWF_UPPER_CACHED;
    }
    s.rows8_launch = ev8;
    if (!walk2_shipped(hbm, s.w2)) return fail(COLTT_E_UNSUPPORTED, "hnsw_search: walk variant %d is not compiled into this build (COLTT_WALK2)", s.w2);
  }
  const uint32_t waves = resident_waves(pol, f.quant, s.lds, s.w2, s.vis_kind == 16);
  s.per_cu = waves / 256u;
  s.grid = std::min<uint32_t>((uint32_t)std::min<size_t>(nq, 0xffffffffu), waves);
  return COLTT_OK;
}
}  // namespace hnsw
}  // namespace coltt

namespace {
// hnsw_walk2.hpp kernels: hnsw_search2.hip (launch_search2).

template <int METRIC, int QUANT>
int launch_search(Hnsw* x, HCtx* c, const SearchPlan& sp, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                  uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  const bool visg = sp.vis_kind == 0;
  auto kern = visg ? hnsw_search_kernel<METRIC, QUANT, true> : hnsw_search_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (sp.r8) kern = visg ? hnsw_search_kernel<METRIC, QUANT, true, true> : hnsw_search_kernel<METRIC, QUANT, false, true>; }
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.lds));
  kern<<<grid, 64, sp.lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                        k, sp.ef, sp.ef_pad, sp.hcap, counter, oi, os, oc, stats,
                                        x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                        x->w_vepoch.as<uint32_t>() + region_base);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

// latency launch: one 4-wave workgroup per query in flight, at most one per CU
template <int METRIC, int QUANT>
int launch_search_lat(Hnsw* x, HCtx* c, const SearchPlan& sp, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                      uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  (void)region_base;
  const bool seq = sp.lat_seq != 0;   // the sequential walk (search_level2 + LatEval): plan_search
  // the latency kernel reads the index's ONE row array in the layout it has (line-transposed: lines evaluated out of their registers; natural:
  // staged and transposed through LDS).  COLTT_EV8 chooses between distance cores over the same bytes in the THROUGHPUT kernels; here the layout
  // alone decides (the A/B partner is an index created with COLTT_ROWS8=0).  One kernel instance per (layout, walk): TP = the row's 128-byte lines
  // as a compile-time constant for the common shapes (24: 768 x f32; 12: 768 x 2 bytes, 384 x f32), -1 any line-transposed row, 0 natural order.
  GraphView gv = x->view();
  typedef void (*lat_kern_t)(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*,
                             unsigned long long*, int);
  lat_kern_t kern;
  if constexpr (QUANT == Q_F8) kern = seq ? (lat_kern_t)hnsw_search_lat_kernel<METRIC, QUANT, LAT_TP_STAGED, true> : (lat_kern_t)hnsw_search_lat_kernel<METRIC, QUANT, LAT_TP_STAGED, false>;
  else {
    const int lines = gv.rows8 ? (int)(x->stride >> 7) : 0;
    if (!gv.rows8) kern = seq ? (lat_kern_t)hnsw_search_lat_kernel<METRIC, QUANT, LAT_TP_STAGED, true> : (lat_kern_t)hnsw_search_lat_kernel<METRIC, QUANT, LAT_TP_STAGED, false>;
    else if (seq) kern = hnsw_search_lat_kernel<METRIC, QUANT, LAT_TP_R8_ANY, true>;
    else if (lines == 24) kern = hnsw_search_lat_kernel<METRIC, QUANT, 24, false>;
    else if (lines == 12) kern = hnsw_search_lat_kernel<METRIC, QUANT, 12, false>;
    else kern = hnsw_search_lat_kernel<METRIC, QUANT, LAT_TP_R8_ANY, false>;
  }
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.lds));
  // Batches of at most LAT_MASTERS queries (the reference's one-query RPC above all) get helper workgroups that warm the XCD's L2 with the rows the walk
  // will want next (hnsw_lat.hpp; COLTT_LAT_HELPERS: plan_search).
  unsigned long long* mbox = nullptr;
  const int helpers = sp.lat_helpers;
  if (helpers > 0 && nq <= (uint32_t)LAT_MASTERS) {
    const size_t mb = (size_t)LAT_MASTERS * (LAT_HELPERS_MAX + 1) * 8;
    COLTT_TRY(c->w_mbox.reserve(mb));
    COLTT_HIP(hipMemsetAsync(c->w_mbox.p, 0, mb, c->stream));
    mbox = c->w_mbox.as<unsigned long long>();
    grid = (uint32_t)LAT_MASTERS * (uint32_t)(helpers + 1);
  }
  kern<<<grid, 256, sp.lds, c->stream>>>(gv, x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                         k, sp.ef, sp.ef_pad, sp.hcap, counter, oi, os, oc, stats, mbox, helpers);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

int search_common(Hnsw* x, HCtx* c, const float* queries, bool on_device, size_t nq, uint32_t k, uint32_t ef_override,
                  uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, int force = 0) {
  // argument checks, plan, lease, upload, launch by plan, read-back, counters by plan.  force: plan_search (a call re-run after an err 8)
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (nq == 0) return COLTT_OK;
  if (k == 0) return fail(COLTT_E_INVALID, "hnsw_search: k must be >= 1");
  const Policy pol = policy();   // the ONE snapshot this call decides by
  uint64_t* d_oi = out_ids; float* d_os = out_scores; uint32_t* d_oc = out_counts;
  // small host-buffer calls: the work counter, the traversal counters and the three answer arrays live in ONE device block that
  // comes back in one copy through page-locked staging (layout: 256 B counter + stats | ids | scores | counts)
  const size_t pack_bytes = 256 + nq * k * 12 + nq * 4;
  const bool packed = !on_device && pack_bytes <= SMALL_CALL_BYTES && nq * x->dim * 4 <= SMALL_CALL_BYTES && pol.staging;
  if (packed) {
    COLTT_TRY(c->w_pack.reserve(SMALL_CALL_BYTES + 256));
    COLTT_TRY(c->h_out.reserve(SMALL_CALL_BYTES + 256));
    COLTT_TRY(c->h_in.reserve(SMALL_CALL_BYTES));
    uint8_t* b = c->w_pack.as<uint8_t>();
    d_oi = reinterpret_cast<uint64_t*>(b + 256); d_os = reinterpret_cast<float*>(b + 256 + nq * k * 8); d_oc = reinterpret_cast<uint32_t*>(b + 256 + nq * k * 12);
  } else if (!on_device) {
    COLTT_TRY(c->w_out_ids.reserve(nq * k * 8));
    COLTT_TRY(c->w_out_sc.reserve(nq * k * 4));
    COLTT_TRY(c->w_out_cnt.reserve(nq * 4));
    d_oi = c->w_out_ids.as<uint64_t>(); d_os = c->w_out_sc.as<float>(); d_oc = c->w_out_cnt.as<uint32_t>();
  }
  if (x->entry < 0) {  // empty index => empty result, not an error (hnsw.go:249-251)
    COLTT_HIP(hipMemsetAsync(d_oc, 0, nq * 4, c->stream));
    if (!on_device) COLTT_HIP(hipMemcpyAsync(out_counts, d_oc, nq * 4, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipStreamSynchronize(c->stream));
    return COLTT_OK;
  }
  const uint32_t ef = std::max<uint32_t>(ef_override ? ef_override : (uint32_t)x->cfg.ef, k);
  if (ef <= 4096 && wants_visg(pol, ef)) COLTT_TRY(ensure_visg(x, pol));  // lazily: N bytes x <= 2048 regions are only worth having for ef > 128
  const PlanFacts facts = plan_facts(x);
  SearchPlan sp;
  const int plan_rc = plan_search(facts, pol, nq, k, ef, force, sp);
  const bool mw = sp.family == COLTT_PLAN_LATENCY, w2 = sp.family == COLTT_PLAN_WALK2, v16 = sp.vis_kind == 16;
  static const bool dbg_nt = [] { const char* e = getenv("COLTT_DEBUG_ROWS_NT"); return e && *e == '1'; }();   // diagnostics: which twin a walk2 launch takes, and why
  if (dbg_nt && w2) {
    const unsigned long long bytes = (unsigned long long)facts.slots * (unsigned long long)facts.stride, least = (unsigned long long)pol.rows_nt_min_mb << 20;
    fprintf(stderr, "[rows_nt] slots=%llu stride=%zu row bytes=%llu threshold=%llu knob=%d -> %s\n", (unsigned long long)facts.slots, (size_t)facts.stride, bytes, least, pol.rows_nt,
            rows_nt(facts, pol) ? "nt" : "default");
  }
  COLTT_TRY(plan_rc);
  uint32_t grid = sp.grid;
  RegionLease lease;
  if (sp.vis_kind == 0) { acquire_regions(x, grid, lease); grid = lease.count; }
  const float* d_q = queries;
  if (!on_device) {
    COLTT_TRY(c->w_qraw.reserve(nq * x->dim * 4));
    const void* src = queries;
    if (packed) { std::memcpy(c->h_in.p, queries, nq * x->dim * 4); src = c->h_in.p; }
    COLTT_HIP(hipMemcpyAsync(c->w_qraw.p, src, nq * x->dim * 4, hipMemcpyHostToDevice, c->stream));
    d_q = c->w_qraw.as<float>();
  }
  COLTT_TRY(c->w_misc.reserve(256));
  if (!packed) COLTT_TRY(c->h_out.reserve(256));   // the traversal counters come back through page-locked memory (a pageable target makes the copy a blocking, staged one)
  uint8_t* misc = packed ? c->w_pack.as<uint8_t>() : c->w_misc.as<uint8_t>();
  uint32_t* counter = reinterpret_cast<uint32_t*>(misc);
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(misc + 16);
  COLTT_TRY(prep_queries_any(x, c, d_q, nq, reinterpret_cast<uint32_t*>(misc)));   // ... which also clears the 256 bytes of counters (no memset of their own)
  COLTT_HIP(hipEventRecord(c->ev0, c->stream));
  if (sp.rows8_launch) x->ev8_launches.fetch_add(1);
  int rc;
#define COLTT_LS_ARGS x, c, sp, grid, lease.base, (uint32_t)nq, k, counter, d_oi, d_os, d_oc, d_stats
#define COLTT_LS(Q) rc = mw ? (x->metric == COLTT_COSINE ? launch_search_lat<M_COS, Q>(COLTT_LS_ARGS) : launch_search_lat<M_L2, Q>(COLTT_LS_ARGS)) \
                     : w2 ? launch_search2(COLTT_LS_ARGS) /* hnsw_search2.hip: the same dispatch over its own kernels */ \
                            : (x->metric == COLTT_COSINE ? launch_search<M_COS, Q>(COLTT_LS_ARGS) : launch_search<M_L2, Q>(COLTT_LS_ARGS))
  COLTT_DISPATCH_QUANT(x->quant, COLTT_LS)
#undef COLTT_LS
#undef COLTT_LS_ARGS
  COLTT_TRY(rc);
  COLTT_HIP(hipEventRecord(c->ev1, c->stream));
  if (x->dense && x->dense_base) add_base_kernel<<<ceil_div(nq * k, 256), 256, 0, c->stream>>>(d_oi, nq * k, x->dense_base);
  unsigned long long h_stats[21] = {0};   // [18 .. 20]: the filtered descent's (shadow rows, rejected, f32 rows above level 0); [6], [7]: the row filter's counters; [16], [17]: the 16-bit visited set's maxima (hnsw_kernels.hpp: hnsw_search2_rowfilter_kernel; [8, 16) is the phase clock's)
  if (packed) COLTT_HIP(hipMemcpyAsync(c->h_out.p, c->w_pack.p, pack_bytes, hipMemcpyDeviceToHost, c->stream));
  else {
    if (!on_device) {
      COLTT_HIP(hipMemcpyAsync(out_ids, d_oi, nq * k * 8, hipMemcpyDeviceToHost, c->stream));
      COLTT_HIP(hipMemcpyAsync(out_scores, d_os, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
      COLTT_HIP(hipMemcpyAsync(out_counts, d_oc, nq * 4, hipMemcpyDeviceToHost, c->stream));
    }
    COLTT_HIP(hipMemcpyAsync(c->h_out.p, d_stats, sizeof(h_stats), hipMemcpyDeviceToHost, c->stream));
  }
#ifdef COLTT_PHASE_TIMING
  unsigned long long h_pt[8] = {0};
  COLTT_HIP(hipMemcpyAsync(h_pt, d_stats + 8, 64, hipMemcpyDeviceToHost, c->stream));
#endif
  COLTT_HIP(hipStreamSynchronize(c->stream));  // the lease (destructor) outlives the kernel
  if (!packed) std::memcpy(h_stats, c->h_out.p, sizeof(h_stats));
  if (packed) {
    const uint8_t* hb = c->h_out.as<uint8_t>();
    std::memcpy(h_stats, hb + 16, sizeof(h_stats));
    std::memcpy(out_ids, hb + 256, nq * k * 8);
    std::memcpy(out_scores, hb + 256 + nq * k * 8, nq * k * 4);
    std::memcpy(out_counts, hb + 256 + nq * k * 12, nq * 4);
  }
#ifdef COLTT_PHASE_TIMING
  {
    static const char* nm_w[8] = {"pop", "adjacency", "visited", "rows+dist", "merge", "prologue(upper levels)", "writeout", "shadow rows (row filter, phase A)"};
    static const char* nm_l[8] = {"pop+publish", "adjacency", "visited+fetch+stage", "eval", "barrier2+admission", "-", "prologue(upper levels)", "-"};
    const char* const* nm = mw ? nm_l : nm_w;
    double tot = 0; for (int i = 0; i < 8; i++) tot += (double)h_pt[i];
    fprintf(stderr, "[phase] nq=%zu ef=%u visg=%d:", nq, sp.ef, (int)(sp.vis_kind == 0));
    for (int i = 0; i < 8; i++) fprintf(stderr, " %s %.1f%%", nm[i], 100.0 * (double)h_pt[i] / tot);
    fprintf(stderr, "  | ticks/query %.0f\n", tot / (double)nq);
  }
#endif
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  x->last_ms.store(ms);
  {   // what this launch kept its visited set in, and how many traversals per CU it kept resident (the grid rule's figure; the 16-bit launches: the runtime's too)
    uint32_t per_cu = sp.per_cu;
    if (v16 && c->occ_per_cu > 0) per_cu = std::min<uint32_t>(per_cu, (uint32_t)c->occ_per_cu);
    x->last_vis_kind.store(sp.vis_kind); x->last_per_cu.store(per_cu); x->last_grid.store(grid);
    x->last_stash_max.store(v16 ? h_stats[16] : 0); x->last_visited_max.store(v16 ? h_stats[17] : 0);
    if (v16) x->v16_launches.fetch_add(1);
  }
  if (mw && (h_stats[4] & 8ull))  // the multi-wave kernel's visited table would have needed a reset: same call on the single-wave kernel
    return search_common(x, c, queries, on_device, nq, k, ef_override, out_ids, out_scores, out_counts, stats, force | 1);
  if (w2 && sp.vis_kind != 0 && (h_stats[4] & 8ull))  // same for the walk2 kernel with the LDS hash: hnsw_dev.hpp:search_level has the reset-and-reseed path
    return search_common(x, c, queries, on_device, nq, k, ef_override, out_ids, out_scores, out_counts, stats, force | 3);
  if (h_stats[4]) return fail(COLTT_E_DEVICE, "hnsw_search: traversal watchdog tripped (code %llu)", h_stats[4]);
  if (stats) { stats->n_dist = h_stats[0]; stats->n_exp = h_stats[1]; stats->n_hops = h_stats[2]; stats->n_visit_resets = h_stats[3]; }
  if (sp.filter) { x->flt_launches.fetch_add(1); x->flt_rejected.fetch_add(h_stats[6]); x->flt_f32_rows.fetch_add(h_stats[7]); x->flt_shadow_rows.fetch_add(h_stats[5]); }
  if (sp.filter && (sp.upper & ROWF_UPPER_FILTER)) { x->flt_up_launches.fetch_add(1); x->flt_up_shadow_rows.fetch_add(h_stats[18]); x->flt_up_rejected.fetch_add(h_stats[19]); x->flt_up_f32_rows.fetch_add(h_stats[20]); }   // (a call re-run after err 8 returned above: only the launch that answered counts)
  return COLTT_OK;
}


// ---- Hnsw.Search over product-quantiser codes + exact re-rank (hnsw_pq.hpp) --------------------------------------------------------
// neighbourhood blocks: one thread per 16-byte piece of nbr[slot][p][row_bytes]
__global__ void pq_nbr_build_kernel(const uint32_t* __restrict__ adj0, const uint8_t* __restrict__ codes, uint8_t* __restrict__ nbr, uint64_t total, uint32_t row_bytes) {
  const uint32_t pieces = row_bytes >> 4;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint64_t e = t / pieces; const uint32_t pc = (uint32_t)(t - e * pieces);   // e = slot * width + p
  const uint32_t nb = adj0[e];
  u32x4v v = {0u, 0u, 0u, 0u};
  if (nb != NBR_NONE) v = *reinterpret_cast<const u32x4v*>(codes + (size_t)nb * row_bytes + (size_t)pc * 16);
  *reinterpret_cast<u32x4v*>(nbr + e * row_bytes + (size_t)pc * 16) = v;
}
}  // namespace

namespace coltt {
namespace hnsw {
// Called by a search (shared lock held).  *use: the blocks are there and current.  They cost n x mMax0 x pq_row bytes (20.5 GB at 10 M x 32 x 64): an index
// that cannot afford them (less than twice that free) keeps gathering by neighbour slot.
int ensure_pq_nbr(Hnsw* x, hipStream_t stream, bool* use) {
  *use = false;
  if (!policy().pq_nbr || !x->pq_on || x->n == 0) return COLTT_OK;
  std::lock_guard<std::mutex> g(x->pq_nbr_mu);
  if (!x->pq_nbr_stale.load()) { *use = x->pq_nbr_ok; return COLTT_OK; }
  const uint32_t W = (uint32_t)x->cfg.m_max0;
  const size_t bytes = (size_t)std::max<uint64_t>(x->cap, x->n) * W * x->pq_row;
  x->pq_nbr_ok = false;
  if (x->pq_nbr.cap < bytes) {
    size_t free_b = 0, total_b = 0;
    COLTT_HIP(hipMemGetInfo(&free_b, &total_b));
    if (bytes > free_b / 2 || x->pq_nbr.reserve(bytes) != COLTT_OK) { (void)hipGetLastError(); x->pq_nbr_stale.store(false); return COLTT_OK; }
  }
  const uint64_t pieces = x->n * W * (x->pq_row >> 4);
  const uint64_t step = 840ull << 20;   // a multiple of every pieces-per-row (1 .. 8); grid.x stays under 2^31
  for (uint64_t b = 0; b < pieces; b += step) {
    const uint64_t m = std::min<uint64_t>(step, pieces - b);
    const uint64_t e0 = b / (x->pq_row >> 4);
    pq_nbr_build_kernel<<<(unsigned)ceil_div(m, 256), 256, 0, stream>>>(x->adj0.as<uint32_t>() + e0, x->pq_codes.as<uint8_t>(), x->pq_nbr.as<uint8_t>() + e0 * x->pq_row, m, x->pq_row);
  }
  COLTT_HIP(hipGetLastError());
  COLTT_HIP(hipStreamSynchronize(stream));
  x->pq_nbr_ok = true; x->pq_nbr_built = true; x->pq_nbr_stale.store(false);
  x->pq_nbr_builds.fetch_add(1);
  *use = true;
  return COLTT_OK;
}
}  // namespace hnsw
}  // namespace coltt

namespace {
// ---- the writers' side of the neighbourhood blocks: re-gather the blocks of the level-0 rows a mutation rewrote -------------------------------------
// the blocks of the listed slots, as pq_nbr_build_kernel writes them: one thread per 16-byte piece of nbr[slots[i]][p][row_bytes].  count (may be NULL: all
// `cap` entries) = the device counter the link kernels appended under; a slot or a neighbour outside [0, n_slots) is skipped (never the case).
__global__ void pq_nbr_patch_kernel(const uint32_t* __restrict__ adj0, const uint8_t* __restrict__ codes, uint8_t* __restrict__ nbr, const uint32_t* __restrict__ slots,
                                    const uint32_t* __restrict__ count, uint32_t cap, uint32_t W, uint32_t row_bytes, uint32_t n_slots) {
  const uint32_t pieces = row_bytes >> 4, per = W * pieces;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t i = t / per;
  uint32_t n = cap;
  if (count) { const uint32_t c = *count; n = c < cap ? c : cap; }
  if (i >= n) return;
  const uint32_t slot = slots[i];
  if (slot >= n_slots) return;
  const uint32_t r = (uint32_t)(t - i * per);
  const uint32_t p = r / pieces, pc = r - p * pieces;
  const uint64_t e = (uint64_t)slot * W + p;
  const uint32_t nb = adj0[e];
  u32x4v v = {0u, 0u, 0u, 0u};
  if (nb < n_slots) v = *reinterpret_cast<const u32x4v*>(codes + (size_t)nb * row_bytes + (size_t)pc * 16);   // (NBR_NONE is not below n_slots)
  *reinterpret_cast<u32x4v*>(nbr + e * row_bytes + (size_t)pc * 16) = v;
}
// One mutation's bookkeeping.  begin: called under the exclusive lock once the call can no longer be refused and before its first device write — the blocks are
// stale from here on; if they were current (and the knobs allow) the call tracks: d_dirty is the list its link kernels append to.  end: called when every
// kernel of the mutation has been launched and the new slots' codes are written (sync_pq) — re-gathers the blocks of the new slots [first_new, first_new +
// n_new), of the listed rows (the link kernels' list, or d_slots[n_slots_listed] the host put together: Remove) and only then calls the blocks current again.
// A call that returns early never reaches end: the blocks stay stale and the next walk rebuilds them.
constexpr uint64_t PQ_PATCH_MAX_LIST = 1ull << 20;   // entries (4 MiB): a call that could rewrite more rows than this leaves the blocks to the whole rebuild
struct PqNbrPatch { bool on = false; uint32_t* d_dirty = nullptr; uint32_t cap = 0; };
PqNbrPatch pq_nbr_patch_begin(Hnsw* x, uint64_t max_listed) {
  PqNbrPatch t;
  const bool current = !x->pq_nbr_stale.load() && x->pq_nbr_ok;
  x->pq_nbr_stale.store(true);
  if (!current || !x->pq_on || max_listed > PQ_PATCH_MAX_LIST) return t;   // an index that keeps no blocks pays this line and nothing else
  const Policy pol = policy();
  if (!pol.pq_nbr || !pol.pq_nbr_patch) return t;
  if (max_listed) {
    if (x->pq_dirty.reserve((2 + max_listed) * 4) != COLTT_OK) { (void)hipGetLastError(); return t; }
    if (hipMemsetAsync(x->pq_dirty.p, 0, 8, x->stream) != hipSuccess) { (void)hipGetLastError(); return t; }
    t.d_dirty = x->pq_dirty.as<uint32_t>(); t.cap = (uint32_t)max_listed;
  }
  t.on = true;
  return t;
}
int pq_nbr_patch_end(Hnsw* x, const PqNbrPatch& t, uint64_t first_new, uint64_t n_new, const uint32_t* d_slots, uint32_t n_slots_listed) {
  if (!t.on) return COLTT_OK;
  const uint32_t W = (uint32_t)x->cfg.m_max0, pieces = x->pq_row >> 4;
  if (x->pq_nbr.cap < (size_t)std::max<uint64_t>(x->cap, x->n) * W * x->pq_row || x->pq_done < x->n) return COLTT_OK;   // the slot capacity grew past the array: stale, rebuilt whole
  const uint32_t* adj0 = x->adj0.as<uint32_t>(); const uint8_t* codes = x->pq_codes.as<uint8_t>(); uint8_t* nbr = x->pq_nbr.as<uint8_t>();
  if (n_new) {   // a run of consecutive slots: the whole build's kernel over that run
    const uint64_t total = n_new * W * pieces, e0 = first_new * W;
    pq_nbr_build_kernel<<<(unsigned)ceil_div(total, 256), 256, 0, x->stream>>>(adj0 + e0, codes, nbr + e0 * x->pq_row, total, x->pq_row);
  }
  const uint32_t* list = t.d_dirty ? t.d_dirty + 2 : d_slots;
  const uint32_t lcap = t.d_dirty ? t.cap : n_slots_listed;
  if (lcap) pq_nbr_patch_kernel<<<(unsigned)ceil_div((uint64_t)lcap * W * pieces, 256), 256, 0, x->stream>>>(adj0, codes, nbr, list, t.d_dirty, lcap, W, x->pq_row, (uint32_t)x->n);
  COLTT_HIP(hipGetLastError());
  uint32_t listed = n_slots_listed;
  if (t.d_dirty) COLTT_HIP(hipMemcpyAsync(&listed, t.d_dirty, 4, hipMemcpyDeviceToHost, x->stream));
  COLTT_HIP(hipStreamSynchronize(x->stream));
  if (listed > lcap) return COLTT_OK;   // (the list is sized by the request bound: not reached) rows were dropped — stale
  x->pq_nbr_patches.fetch_add(1); x->pq_nbr_patched_rows.fetch_add(n_new + listed);
  x->pq_nbr_stale.store(false);
  return COLTT_OK;
}
// Resident traversals per CU of the product-quantised walk (120 VGPRs: four waves per SIMD would fit; the LDS decides below that — 16 instead of 12
// measured nothing, profiles/r05s_pq_ab.md).
// The walk over the byte map carries NO Bloom filter (the row walks do, hnsw_walk2.hpp): the probe of the byte map is one wave-wide load that is
// issued whenever ANY lane's filter bits are set — and some ~10 of an expansion's 32 neighbours have been visited, so it is issued practically
// always; what the filter saves is probing lanes (HBM sectors), which this walk has to spare, and what it costs is an LDS atomic round trip in
// front of every probe plus 2-4 KiB of LDS per traversal (one resident wave per CU at ef 1 408).  Same box, 10 M x 768 f16, 64 x 32 quantiser
// (profiles/r05s_pq_ab.md): ef 1 024 410 -> 440 k queries/s, ef 1 408 277 -> 316 k.
constexpr size_t PQ_WAVES_CAP = 12;
// filt_cap: the capacity of the allowed set R of a filtered walk (coltt_hnsw_pq_search_filtered), 0 = no filter
bool pq_geom(Hnsw* x, uint32_t ef, bool force_hbm, PqGeom& out, uint32_t filt_cap = 0) {
  PqGeom s{};
  s.ef = ef; s.ef_pad = (ef + 63) & ~63u;
  const size_t fixed = (size_t)s.ef_pad * 8 + ((size_t)pq_walk_table_rows(x->pq_row >> 4) << pq_lut_shift(x)) * 2   // result set | binary16 table, pair-interleaved (the query stays in HBM: only the re-rank reads it)
                     + (filt_cap ? (size_t)((filt_cap + 63u) & ~63u) * 8 : 0);                                         // | R
  if (fixed > 160 * 1024) return false;
  const bool hbm_ok = x->vis_stride != 0 && x->vis_regions > 0;
  // LDS hash: as walk_geom sizes it; it must never need the reset path (err 8 -> the call is re-run over the byte map)
  uint32_t hcap = std::min<uint32_t>(32768u, std::max<uint32_t>(8192u, next_pow2(ef * 48u)));
  const bool lds_fits = fixed + (size_t)hcap * 4 <= 160 * 1024;
  if (!force_hbm && !(wants_visg(policy(), ef) && hbm_ok) && lds_fits) { s.variant = 0; s.vis_words = hcap; s.lds = fixed + (size_t)hcap * 4; }
  else {
    if (!hbm_ok) return false;
    s.variant = 2; s.vis_words = 0; s.lds = fixed;
  }
  {
    const Policy pol = policy();
    const size_t cap = pol.pq_waves > 0 ? (size_t)pol.pq_waves : PQ_WAVES_CAP;
    s.per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(cap, (160 * 1024) / s.lds));
  }
  out = s;
  return true;
}

}  // namespace

namespace coltt {
namespace hnsw {
int launch_pq_walk(Hnsw* x, HCtx* c, const PqGeom& sg, bool nbr, uint32_t grid, uint32_t region_base, const unsigned short* lut, uint32_t nq, uint32_t k,
                   uint32_t rerank, uint32_t* counter, uint32_t* surv, uint32_t* surv_cnt, unsigned long long* stats, const FilterView* fv, uint32_t fcap,
                   const PqFiltQuery* pd) {
  const uint32_t sh = pq_lut_shift(x);
  // table row length x code-row pieces as compile-time constants for the common quantisers: 64 sub-vectors x 16 / 32 centroids (LS 4 / 5, 4 pieces),
  // 32 x 256 — the reference's shape, playground/hnswpq_verification.go:69-73 — (LS 8, 2 pieces), 96 x 256 (LS 8, 6 pieces); anything else runs the
  // forms that read the shape at run time.  Byte map (variant 2) with or without the neighbourhood blocks; the LDS-hash variant gathers.
  const uint32_t np = x->pq_row >> 4;
  typedef void (*pq_kern_t)(GraphView, int32_t, int32_t, const unsigned short*, const uint8_t*, const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                            uint32_t*, uint32_t*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*, FilterView, uint32_t);
  pq_kern_t kern;
  // fv (coltt_hnsw_pq_search_filtered): the same dispatch over the FILTER instances — one filter takes the same kernel form through either entry point
  // pd (coltt_hnsw_pq_search_filtered_batch): the same dispatch once more over the PERQ instances — nq descriptors, one per query of the launch; sg then
  // carries the launch's variant, its largest query's LDS and the survivors' stride (ef_pad)
#define COLTT_PQKF(LS, NP, F, P) (sg.variant == 0 ? (pq_kern_t)hnsw_pq_search_kernel<0, VIS_LDS, LS, NP, false, F, P> : nbr ? (pq_kern_t)hnsw_pq_search_kernel<2, VIS_HBM, LS, NP, true, F, P> : (pq_kern_t)hnsw_pq_search_kernel<2, VIS_HBM, LS, NP, false, F, P>)
#define COLTT_PQK(LS, NP) (pd ? COLTT_PQKF(LS, NP, true, true) : fv ? COLTT_PQKF(LS, NP, true, false) : COLTT_PQKF(LS, NP, false, false))
  if (sh == 5 && np == 4) kern = COLTT_PQK(5, 4);
  else if (sh == 4 && np == 4) kern = COLTT_PQK(4, 4);
  else if (sh == 8 && np == 2) kern = COLTT_PQK(8, 2);
  else if (sh == 8 && np == 6) kern = COLTT_PQK(8, 6);
  else if (sh == 4) kern = COLTT_PQK(4, 0);
  else if (sh == 5) kern = COLTT_PQK(5, 0);
  else if (sh == 8) kern = COLTT_PQK(8, 0);
  else kern = COLTT_PQK(0, 0);
#undef COLTT_PQK
#undef COLTT_PQKF
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sg.lds));
  kern<<<grid, 64, sg.lds, c->stream>>>(x->view(), x->entry, x->entry_level, lut, x->pq_codes.as<uint8_t>(), nbr ? x->pq_nbr.as<uint8_t>() : nullptr, x->pq_row, sh, nq, k, sg.ef, sg.ef_pad, rerank,
                                        sg.vis_words, counter, surv, surv_cnt, stats, x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride,
                                        (size_t)x->vis_stride, x->w_vepoch.as<uint32_t>() + region_base,
                                        pd ? FilterView{reinterpret_cast<const uint32_t*>(pd), 0u} : fv ? *fv : FilterView{nullptr, 0u}, fcap);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}
}  // namespace hnsw
}  // namespace coltt

namespace {
}  // namespace

// (not a template: it stands in the one translation unit that launches it)
namespace coltt {
namespace kern {
// step 2: the k smallest keys of a query — (exact score bits, slot) order — by k rounds of a wave minimum over the keys staged in LDS
__global__ __launch_bounds__(64) void hnsw_pq_select_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ surv_cnt, uint32_t ef_pad, uint32_t k,
                                                            const uint64_t* __restrict__ ids, uint64_t* __restrict__ out_ids, float* __restrict__ out_scores,
                                                            uint32_t* __restrict__ out_counts, const PqFiltQuery* __restrict__ pd = nullptr) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  unsigned long long* const res = reinterpret_cast<unsigned long long*>(smem);
  const uint32_t qi = blockIdx.x, r = surv_cnt[qi];
  const uint32_t row = pd ? pd[qi].row : qi;   // pd (coltt_hnsw_pq_search_filtered_batch): query qi of the launch answers batch row pd[qi].row
  const int lane_in = threadIdx.x;
  for (uint32_t i = (uint32_t)lane_in; i < r; i += 64) res[i] = keys[(size_t)qi * ef_pad + i];
  wave_sync();
  const uint32_t n = r < k ? r : k;
  for (uint32_t t = 0; t < n; t++) {
    const int lane = opaque_lane(lane_in);
    unsigned long long best = ~0ull; uint32_t bi = 0;
    for (uint32_t i = (uint32_t)lane; i < r; i += 64) { const unsigned long long e = res[i]; if (e < best) { best = e; bi = i; } }
    const unsigned long long km = wave_min_u64(best);
    if (best == km && km != ~0ull) {   // keys are distinct (a slot appears once): exactly one lane
      const uint32_t slot = (uint32_t)km >> 1;
      out_ids[(size_t)row * k + t] = ids ? ids[slot] : (uint64_t)slot;
      out_scores[(size_t)row * k + t] = __uint_as_float((uint32_t)(km >> 32));
      res[bi] = ~0ull;
    }
    wave_sync();
  }
  if (lane_in == 0) out_counts[row] = n;
}
}  // namespace kern
}  // namespace coltt

namespace {
template <int METRIC, int QUANT>
int launch_pq_rerank_for(Hnsw* x, HCtx* c, const PqGeom& sg, uint32_t q0, uint32_t nq, uint32_t k, const uint32_t* surv, const uint32_t* surv_cnt,
                     unsigned long long* keys, uint64_t* oi, float* os, uint32_t* oc, const PqFiltQuery* pd = nullptr, const float* pd_qe = nullptr,
                     const float* pd_qn = nullptr) {
  const dim3 grid(ceil_div(sg.ef_pad, 32), nq);
  const GraphView g = x->view();
  const float* qe = c->w_qeff.as<float>() + (size_t)q0 * x->dim; const float* qn = c->w_qn.as<float>() + q0;
  if (pd) { qe = pd_qe; qn = pd_qn; q0 = 0; }   // a compacted sub-batch (coltt_hnsw_pq_search_filtered_batch): its own queries; the select answers row pd[i].row
  if (x->r8) hnsw_pq_rerank_kernel<METRIC, QUANT, true><<<grid, 64, 0, c->stream>>>(g, qe, qn, surv, surv_cnt, sg.ef_pad, keys);
  else hnsw_pq_rerank_kernel<METRIC, QUANT, false><<<grid, 64, 0, c->stream>>>(g, qe, qn, surv, surv_cnt, sg.ef_pad, keys);
  const size_t lds = (size_t)sg.ef_pad * 8;
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_pq_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hnsw_pq_select_kernel<<<nq, 64, lds, c->stream>>>(keys, surv_cnt, sg.ef_pad, k, g.ids, oi + (size_t)q0 * k, os + (size_t)q0 * k, oc + q0, pd);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}
}  // namespace

namespace coltt {
namespace hnsw {
// the re-rank for the index's metric and row format (attach refuses "f8" rows)
int launch_pq_rerank(Hnsw* x, HCtx* c, const PqGeom& sg, uint32_t q0, uint32_t nq, uint32_t k, const uint32_t* surv, const uint32_t* surv_cnt,
                     unsigned long long* keys, uint64_t* oi, float* os, uint32_t* oc, const PqFiltQuery* pd, const float* pd_qe, const float* pd_qn) {
  int rc;
#define COLTT_LP_ARGS x, c, sg, q0, nq, k, surv, surv_cnt, keys, oi, os, oc, pd, pd_qe, pd_qn
#define COLTT_LP(Q) rc = x->metric == COLTT_COSINE ? launch_pq_rerank_for<M_COS, Q>(COLTT_LP_ARGS) : launch_pq_rerank_for<M_L2, Q>(COLTT_LP_ARGS)
  if (x->quant == COLTT_Q_NONE) { COLTT_LP(Q_NONE); } else { COLTT_LP(Q_F16); }
#undef COLTT_LP
#undef COLTT_LP_ARGS
  return rc;
}

// the geometry of one walk at ef, as every entry point decides it: the LDS hash unless the policy, the caller (force_hbm) or the table's size says the byte map
int pq_walk_geom(Hnsw* x, uint32_t ef, bool force_hbm, uint32_t fcap, PqGeom& sg) {
  const Policy pol = policy();
  if (wants_visg(pol, ef) || force_hbm) COLTT_TRY(ensure_visg(x, pol));
  bool have = pq_geom(x, ef, force_hbm, sg, fcap);
  if (!have && !force_hbm) { COLTT_TRY(ensure_visg(x, pol)); have = pq_geom(x, ef, true, sg, fcap); }   // no room for the LDS hash beside the table: the byte map
  if (!have) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_search: dim %u / ef %u / %u sub-vectors need more than the CU's 160 KiB of LDS", x->dim, ef, x->pq_shape.m);
  return COLTT_OK;
}
}  // namespace hnsw
}  // namespace coltt

namespace {

// one attempt; *retry_hbm: the LDS hash would have needed its reset path — the caller runs the same call over the byte map
// fv (coltt_hnsw_pq_search_filtered, WALK): the walk also keeps the allowed set R and the re-rank is over R; ef_override is then ef_walk (>= k)
int pq_search_once(Hnsw* x, HCtx* c, const float* queries, bool on_device, size_t nq, uint32_t k, uint32_t ef_override, uint32_t rerank,
                   uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact, bool force_hbm, bool* retry_hbm,
                   const FilterView* fv = nullptr) {
  *retry_hbm = false;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (out_n_exact) *out_n_exact = 0;
  if (nq == 0) return COLTT_OK;
  if (k == 0) return fail(COLTT_E_INVALID, "hnsw_pq_search: k must be >= 1");
  if (!x->pq_on) return fail(COLTT_E_INVALID, "hnsw_pq_search: the index carries no product-quantiser codes (coltt_hnsw_pq_attach)");
  if (x->pq_done != x->n) return fail(COLTT_E_DEVICE, "hnsw_pq_search: codes cover %llu of %llu slots", (unsigned long long)x->pq_done, (unsigned long long)x->n);
  uint64_t* d_oi = out_ids; float* d_os = out_scores; uint32_t* d_oc = out_counts;
  if (!on_device) {
    COLTT_TRY(c->w_out_ids.reserve(nq * k * 8)); COLTT_TRY(c->w_out_sc.reserve(nq * k * 4)); COLTT_TRY(c->w_out_cnt.reserve(nq * 4));
    d_oi = c->w_out_ids.as<uint64_t>(); d_os = c->w_out_sc.as<float>(); d_oc = c->w_out_cnt.as<uint32_t>();
  }
  if (x->entry < 0) {  // empty index => empty result, not an error (hnsw.go:249-251)
    COLTT_HIP(hipMemsetAsync(d_oc, 0, nq * 4, c->stream));
    if (!on_device) COLTT_HIP(hipMemcpyAsync(out_counts, d_oc, nq * 4, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipStreamSynchronize(c->stream));
    return COLTT_OK;
  }
  const uint32_t ef = std::max<uint32_t>(ef_override ? ef_override : (uint32_t)x->cfg.ef, k);  // gomath.MaxInt(ef, k), hnsw.go:258
  if (ef > 4096) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_search: ef=%u > 4096", ef);
  PqGeom sg;
  const uint32_t fcap = fv ? pq_filt_cap(ef, k, rerank) : 0u;   // |R| <= cap
  COLTT_TRY(pq_walk_geom(x, ef, force_hbm, fcap, sg));
  uint32_t grid = (uint32_t)std::min<size_t>(nq, (size_t)256 * sg.per_cu);
  RegionLease lease;
  if (sg.variant != 0) { acquire_regions(x, grid, lease); grid = lease.count; }
  const float* d_q = queries;
  if (!on_device) {
    COLTT_TRY(c->w_qraw.reserve(nq * x->dim * 4));
    COLTT_HIP(hipMemcpyAsync(c->w_qraw.p, queries, nq * x->dim * 4, hipMemcpyHostToDevice, c->stream));
    d_q = c->w_qraw.as<float>();
  }
  COLTT_TRY(prep_queries_any(x, c, d_q, nq));
  bool nbr = false;
  if (sg.variant != 0) COLTT_TRY(ensure_pq_nbr(x, c->stream, &nbr));
  // tables for a group of queries at a time: [group][row_bytes][1 << shift] binary16 (4 KiB per query for 64 x 32), up to 256 MiB of them — a launch should
  // hold several queries per resident wave so that the work counter balances the tail (a 10 000-query call once ran as five 2 048-query launches on
  // 2 048 waves: every launch as long as its slowest traversal, profiles/r05i_bench_kernel_stats_by_grid.csv); at most 32 768 queries (the re-rank's grid.y)
  const uint32_t lsh = pq_lut_shift(x);
  const size_t lut_q = ((size_t)x->pq_row << lsh) * 2;
  // ... and the survivors' slots + exact keys (12 bytes per result-set entry and query) stay under 256 MiB as well (1.5 GB per pooled context at ef 4096)
  const size_t group = std::max<size_t>(1, std::min<size_t>({nq, (256ull << 20) / lut_q, (256ull << 20) / ((size_t)sg.ef_pad * 12), (size_t)32768}));
  COLTT_TRY(c->w_pack.reserve(group * lut_q + group * 4));   // the tables, then one word per query: its table's maximum (pq.hip: table scale)
  COLTT_TRY(c->w_surv.reserve(group * sg.ef_pad * 4)); COLTT_TRY(c->w_scnt.reserve(group * 4)); COLTT_TRY(c->w_keys.reserve(group * sg.ef_pad * 8));
  COLTT_TRY(c->w_misc.reserve(256));
  uint8_t* misc = c->w_misc.as<uint8_t>();
  uint32_t* counter = reinterpret_cast<uint32_t*>(misc);
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(misc + 16);
  COLTT_HIP(hipMemsetAsync(misc, 0, 256, c->stream));
  COLTT_HIP(hipEventRecord(c->ev0, c->stream));
  for (size_t q0 = 0; q0 < nq; q0 += group) {
    const size_t gn = std::min(group, nq - q0);
    COLTT_TRY(pq_lut16_batch(c->stream, x->pq_cb.as<float>(), x->pq_shape, c->w_qeff.as<float>() + q0 * x->dim, gn, x->pq_row, lsh,
                             reinterpret_cast<uint32_t*>(c->w_pack.as<uint8_t>() + group * lut_q), c->w_pack.as<unsigned short>()));
    if (q0) COLTT_HIP(hipMemsetAsync(counter, 0, 4, c->stream));
    COLTT_TRY(launch_pq_walk(x, c, sg, nbr, (uint32_t)std::min<size_t>(grid, gn), lease.base, c->w_pack.as<unsigned short>(), (uint32_t)gn, k, rerank, counter, c->w_surv.as<uint32_t>(),
                             c->w_scnt.as<uint32_t>(), d_stats, fv, fcap));
    COLTT_TRY(launch_pq_rerank(x, c, sg, (uint32_t)q0, (uint32_t)gn, k, c->w_surv.as<uint32_t>(), c->w_scnt.as<uint32_t>(), c->w_keys.as<unsigned long long>(), d_oi, d_os, d_oc));
  }
  COLTT_HIP(hipEventRecord(c->ev1, c->stream));
  if (x->dense && x->dense_base) add_base_kernel<<<ceil_div(nq * k, 256), 256, 0, c->stream>>>(d_oi, nq * k, x->dense_base);
  unsigned long long h_stats[5] = {0, 0, 0, 0, 0};
  if (!on_device) {
    COLTT_HIP(hipMemcpyAsync(out_ids, d_oi, nq * k * 8, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipMemcpyAsync(out_scores, d_os, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipMemcpyAsync(out_counts, d_oc, nq * 4, hipMemcpyDeviceToHost, c->stream));
  }
  COLTT_HIP(hipMemcpyAsync(h_stats, d_stats, 40, hipMemcpyDeviceToHost, c->stream));
#ifdef COLTT_PHASE_TIMING
  unsigned long long h_pt[8] = {0};
  COLTT_HIP(hipMemcpyAsync(h_pt, d_stats + 8, 64, hipMemcpyDeviceToHost, c->stream));
#endif
  COLTT_HIP(hipStreamSynchronize(c->stream));  // the lease (destructor) outlives the kernel
#ifdef COLTT_PHASE_TIMING
  {
    static const char* nm[8] = {"pop", "adjacency", "visited", "codes+table sum", "admission/evict/flush", "prologue(table, upper levels)", "flush+re-rank+writeout", "-"};
    double tot = 0; for (int i = 0; i < 7; i++) tot += (double)h_pt[i];
    fprintf(stderr, "[phase pq] nq=%zu ef=%u variant=%d per_cu=%u:", nq, sg.ef, sg.variant, sg.per_cu);
    for (int i = 0; i < 7; i++) fprintf(stderr, " %s %.1f%%", nm[i], 100.0 * (double)h_pt[i] / tot);
    fprintf(stderr, "  | ticks/query %.0f, per expansion %.0f\n", tot / (double)nq, tot / (double)std::max<unsigned long long>(1, h_stats[1]));
  }
#endif
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  x->last_ms.store(ms);
  if (sg.variant == 0 && (h_stats[4] & 8ull)) { *retry_hbm = true; return COLTT_OK; }
  if (h_stats[4]) return fail(COLTT_E_DEVICE, "hnsw_pq_search: traversal watchdog tripped (code %llu)", h_stats[4]);
  if (stats) { stats->n_dist = h_stats[0]; stats->n_exp = h_stats[1]; stats->n_hops = h_stats[2]; stats->n_visit_resets = 0; }
  if (out_n_exact) *out_n_exact = h_stats[3];
  return COLTT_OK;
}
int pq_search_common(Hnsw* x, HCtx* c, const float* queries, bool on_device, size_t nq, uint32_t k, uint32_t ef_override, uint32_t rerank,
                     uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact) {
  bool retry = false;
  COLTT_TRY(pq_search_once(x, c, queries, on_device, nq, k, ef_override, rerank, out_ids, out_scores, out_counts, stats, out_n_exact, false, &retry));
  if (retry) COLTT_TRY(pq_search_once(x, c, queries, on_device, nq, k, ef_override, rerank, out_ids, out_scores, out_counts, stats, out_n_exact, true, &retry));
  return COLTT_OK;
}
}  // namespace

namespace coltt {
namespace hnsw {
// coltt_hnsw_pq_search_filtered, WALK: pq_search_common at ef_walk with the allowed set
int pq_search_filtered_walk(Hnsw* x, HCtx* c, const FilterView& fv, const float* queries, size_t nq, uint32_t k, uint32_t ef_walk, uint32_t rerank,
                            uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact) {
  bool retry = false;
  COLTT_TRY(pq_search_once(x, c, queries, false, nq, k, ef_walk, rerank, out_ids, out_scores, out_counts, stats, out_n_exact, false, &retry, &fv));
  if (retry) COLTT_TRY(pq_search_once(x, c, queries, false, nq, k, ef_walk, rerank, out_ids, out_scores, out_counts, stats, out_n_exact, true, &retry, &fv));
  return COLTT_OK;
}
}  // namespace hnsw
}  // namespace coltt

namespace {

// pruneNeighbors as Remove calls it (hnsw.go:234-236): rebuild the row from its non-deleted entries (<= width, so
// nothing is trimmed).  One thread per (neighbour, level) row.
__global__ void hnsw_unlink_kernel(GraphView g, const uint32_t* __restrict__ nbs, const int32_t* __restrict__ lvl, uint32_t n) {
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t W;
  uint32_t* row = const_cast<uint32_t*>(adj_row(g, nbs[t], lvl[t], W));
  float* drow = lvl[t] == 0 ? g.adj0_d + (size_t)nbs[t] * g.mMax0 : g.adjU_d + ((size_t)g.upper_off[nbs[t]] + (uint32_t)(lvl[t] - 1)) * g.mMax;
  float* nrow = (lvl[t] == 0 && g.adj0_n) ? g.adj0_n + (size_t)nbs[t] * g.mMax0 : nullptr;
  float2* mrow = (lvl[t] == 0 && g.adj0_m) ? g.adj0_m + (size_t)nbs[t] * g.mMax0 : nullptr;
  uint32_t m = 0;
  for (uint32_t i = 0; i < W && row[i] != NBR_NONE; i++) {
    uint32_t sl = row[i]; float dd = drow[i];
    if (!is_deleted(g, sl)) { row[m] = sl; drow[m] = dd; if (nrow) nrow[m] = nrow[i]; if (mrow) mrow[m] = mrow[i]; m++; }
  }
  for (; m < W; m++) { row[m] = NBR_NONE; drow[m] = 0.f; if (nrow) nrow[m] = 0.f; if (mrow) mrow[m] = float2{0.f, 0.f}; }
}

int hnsw_undense(Hnsw* x) {
  if (!x->dense) return COLTT_OK;
  x->h_ids.resize(x->n);
  x->id2slot.reserve(x->n * 2);
  for (uint64_t s = 0; s < x->n; s++) {
    x->h_ids[s] = x->dense_base + s;
    if (!(x->h_del.size() > (s >> 5) && ((x->h_del[s >> 5] >> (s & 31)) & 1u))) x->id2slot[x->dense_base + s] = (uint32_t)s;
  }
  x->dense = false;
  COLTT_TRY(x->ids.reserve(std::max<uint64_t>(x->cap, 1024) * 8, false, x->stream));
  if (x->n) COLTT_HIP(hipMemcpyAsync(x->ids.p, x->h_ids.data(), x->n * 8, hipMemcpyHostToDevice, x->stream));
  COLTT_HIP(hipStreamSynchronize(x->stream));
  return COLTT_OK;
}

template <int METRIC, int QUANT>
int launch_build(Hnsw* x, const SearchGeom& sg, uint32_t base, uint32_t count, const int32_t* d_levels, uint32_t* counter,
                 uint32_t* req_count, BuildReq* req, uint32_t* head, unsigned long long* stats) {
  auto kern = sg.visg ? hnsw_build_search_kernel<METRIC, QUANT, true> : hnsw_build_search_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (x->r8) kern = sg.visg ? hnsw_build_search_kernel<METRIC, QUANT, true, true> : hnsw_build_search_kernel<METRIC, QUANT, false, true>; }
  // algo 2 (diverse selection): a second query buffer + the chosen / rejected keys behind the walk's LDS
  const uint32_t diverse = x->cfg.algo == 2 ? (x->cfg.keep_pruned ? 3u : 1u) : 0u;
  const size_t ext_off = (sg.lds + 15) & ~(size_t)15;
  const size_t lds = diverse ? ext_off + (((size_t)x->dim * 4 + 15) & ~(size_t)15) + 2 * 64 * 8 : sg.lds;
  if (lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "hnsw insert: dim/efConstruction need %zu B of LDS", lds);
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const uint32_t per_cu = resident_waves(policy(), QUANT, lds) / 256u;
  uint32_t grid = std::min<uint32_t>({count, 256u * per_cu, sg.max_grid});
  kern<<<grid, 64, lds, x->stream>>>(x->view(), x->entry, x->entry_level, base, count, d_levels, (uint32_t)x->cfg.m,
                                     sg.ef, sg.ef_pad, sg.hcap, x->cap, counter, req_count, req, head, stats,
                                     x->w_visg.as<uint8_t>(), (size_t)x->vis_stride, x->w_vepoch.as<uint32_t>(), diverse, (uint32_t)ext_off);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

template <int METRIC, int QUANT>
int launch_link_diverse(Hnsw* x, const BuildReq* req, uint32_t n_req, uint32_t* head, unsigned long long* stats, uint32_t* dirty, uint32_t dirty_cap) {
  auto kern = hnsw_link_diverse_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (x->r8) kern = hnsw_link_diverse_kernel<METRIC, QUANT, true>; }
  const size_t lds = (((size_t)x->dim * 4 + 15) & ~(size_t)15) + (size_t)(2 * LINKD_CAND + 128) * 8;
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<n_req, 64, lds, x->stream>>>(x->view(), x->cap, req, n_req, head, (uint32_t)(x->cfg.keep_pruned ? 1 : 0), stats, dirty, dirty_cap);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

// n Inserts (hnsw.go:104-167) in order, `batch` at a time against a frozen graph.  d_vecs: raw vectors in HBM.
int insert_core(Hnsw* x, const uint64_t* ids, uint64_t first_id, const float* d_vecs, const int32_t* levels, size_t n,
                uint32_t batch) {
  if (n == 0) return COLTT_OK;
  if (batch == 0) batch = 1;
  if (x->cfg.m_max > LINK_W || x->cfg.m_max0 > LINK_W) return fail(COLTT_E_UNSUPPORTED, "hnsw insert: builder supports mMax, mMax0 <= %d", LINK_W);
  if (x->cfg.m > 64) return fail(COLTT_E_UNSUPPORTED, "hnsw insert: builder supports m <= 64");
  if (x->n + n >= 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw insert: more than 2^31-1 slots");
  for (size_t i = 0; i < n; i++) if (levels[i] < 0 || levels[i] > 60) return fail(COLTT_E_INVALID, "hnsw insert: level %d out of range", levels[i]);
  bool dense_ok = !ids && x->dense && (x->n == 0 || first_id == x->dense_base + x->n);
  if (dense_ok) { if (x->n == 0) x->dense_base = first_id; }
  else {
    COLTT_TRY(hnsw_undense(x));
    std::unordered_map<uint64_t, int> seen;
    for (size_t i = 0; i < n; i++) {  // storeVertex: ItemAlreadyExistsError (hnsw.go:293-295), checked before any mutation
      uint64_t id = ids ? ids[i] : first_id + i;
      if (x->id2slot.count(id) || !seen.emplace(id, 1).second) return fail(COLTT_E_EXISTS, "Item already exists");
    }
  }
  // The neighbourhood blocks are stale from here on; a call that found them current lists the level-0 rows its link kernels rewrite (every new vertex queues at
  // most cfg.m level-0 requests, and a listed row is owned by one of them) and re-gathers their blocks at its end.
  const uint64_t first_new = x->n;
  const PqNbrPatch patch = pq_nbr_patch_begin(x, (uint64_t)n * (uint64_t)x->cfg.m);
  const uint32_t efc = (uint32_t)x->cfg.ef_construction;
  const Policy pol = policy();
  COLTT_TRY(x->w_misc.reserve(64));
  uint32_t* counter = x->w_misc.as<uint32_t>();
  uint32_t* req_count = counter + 1;
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(x->w_misc.as<uint8_t>() + 16);
  size_t i = 0;
  uint32_t shrink = 0;   // diverse mode: a batch that would overflow a row's candidate list is retried at half the size (nothing was applied)
  while (i < n) {
    // nil entrypoint (empty index, or Remove left no successor: hnsw.go:197-217 may CAS the entrypoint to nil): the vertex is
    // stored at level 0 and becomes the entrypoint, nothing is linked (hnsw.go:108-116)
    const bool first = x->entry < 0;
    uint32_t b = first ? 1u : (uint32_t)std::min<size_t>(batch, n - i);
    if (shrink) b = std::min(b, shrink);
    uint64_t up = 0;
    for (uint32_t j = 0; j < b; j++) up += first ? 0 : (uint64_t)levels[i + j];
    const uint64_t base = x->n;
    COLTT_TRY(x->reserve(base + b, x->n_upper + up));
    if (wants_visg(pol, efc)) COLTT_TRY(ensure_visg(x, pol));  // (re)sized here: the slot capacity may just have grown
    const SearchGeom sg = walk_geom(plan_facts(x), pol, efc);
    if (sg.lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "hnsw insert: dim/efConstruction need %zu B of LDS", sg.lds);
    // per-slot tables of the batch.  Host mirrors (h_levels, h_upper_off, h_ids, id2slot, h_del) are committed only after
    // the device work of the batch has succeeded: a failed batch leaves the index exactly as it was (slots >= n unreferenced).
    std::vector<uint32_t> uo(b);
    std::vector<int32_t> lv(b);
    std::vector<uint64_t> nid(x->dense ? 0 : b);
    uint64_t u = x->n_upper;
    for (uint32_t j = 0; j < b; j++) {
      lv[j] = first ? 0 : levels[i + j];
      uo[j] = lv[j] > 0 ? (uint32_t)u : NBR_NONE;
      u += (uint64_t)lv[j];
      if (!x->dense) nid[j] = ids ? ids[i + j] : first_id + i + j;
    }
    auto commit_host = [&]() {
      for (uint32_t j = 0; j < b; j++) {
        x->h_levels.push_back(lv[j]);
        x->h_upper_off.push_back(uo[j]);
        if (!x->dense) { x->h_ids.push_back(nid[j]); x->id2slot[nid[j]] = (uint32_t)(base + j); }
      }
      x->h_del.resize((base + b + 31) / 32, 0u);
    };
    COLTT_HIP(hipMemcpyAsync(x->upper_off.as<uint32_t>() + base, uo.data(), (size_t)b * 4, hipMemcpyHostToDevice, x->stream));
    if (!x->dense) COLTT_HIP(hipMemcpyAsync(x->ids.as<uint64_t>() + base, nid.data(), (size_t)b * 8, hipMemcpyHostToDevice, x->stream));
    COLTT_HIP(hipMemsetAsync(x->adj0.as<uint32_t>() + base * x->cfg.m_max0, 0xff, (size_t)b * x->cfg.m_max0 * 4, x->stream));
    COLTT_HIP(hipMemsetAsync(x->adj0_d.as<float>() + base * x->cfg.m_max0, 0, (size_t)b * x->cfg.m_max0 * 4, x->stream));
    if (x->metric == COLTT_COSINE) COLTT_HIP(hipMemsetAsync(x->adj0_n.as<float>() + base * x->cfg.m_max0, 0, (size_t)b * x->cfg.m_max0 * 4, x->stream));
    if (x->shadow8) COLTT_HIP(hipMemsetAsync(x->adj0_m.as<float2>() + base * x->cfg.m_max0, 0, (size_t)b * x->cfg.m_max0 * 8, x->stream));
    if (up) {
      COLTT_HIP(hipMemsetAsync(x->adjU.as<uint32_t>() + x->n_upper * x->cfg.m_max, 0xff, (size_t)up * x->cfg.m_max * 4, x->stream));
      COLTT_HIP(hipMemsetAsync(x->adjU_d.as<float>() + x->n_upper * x->cfg.m_max, 0, (size_t)up * x->cfg.m_max * 4, x->stream));
    }
    COLTT_TRY(prep_rows_any(x, d_vecs + i * x->dim, b, base, x->metric == COLTT_COSINE));
    if (first) {
      COLTT_HIP(hipStreamSynchronize(x->stream));
      commit_host();
      x->entry = (int32_t)base; x->entry_level = 0;
      x->n += 1; x->live += 1; i += 1;
      continue;
    }
    // builder scratch: head[] over every adjacency row, request queue sized for the worst case
    uint64_t need_head = x->cap + x->ucap;
    if (need_head > x->head_cap) {
      COLTT_TRY(x->b_head.reserve(need_head * 4));
      fill_u32_kernel<<<ceil_div(need_head, 256), 256, 0, x->stream>>>(x->b_head.as<uint32_t>(), need_head, NBR_NONE);
      x->head_cap = need_head;
    }
    uint64_t max_req = 0;
    for (uint32_t j = 0; j < b; j++) max_req += (uint64_t)(std::min<int32_t>(lv[j], x->entry_level) + 1) * (uint64_t)x->cfg.m;
    COLTT_TRY(x->b_req.reserve(std::max<uint64_t>(max_req, 1) * sizeof(BuildReq)));
    COLTT_TRY(x->b_levels.reserve((size_t)b * 4));
    COLTT_HIP(hipMemcpyAsync(x->b_levels.p, lv.data(), (size_t)b * 4, hipMemcpyHostToDevice, x->stream));
    COLTT_HIP(hipMemsetAsync(x->w_misc.p, 0, 64, x->stream));
    int rc;
#define COLTT_LB_ARGS x, sg, (uint32_t)base, b, x->b_levels.as<int32_t>(), counter, req_count, x->b_req.as<BuildReq>(), x->b_head.as<uint32_t>(), d_stats
#define COLTT_LB(Q) rc = x->metric == COLTT_COSINE ? launch_build<M_COS, Q>(COLTT_LB_ARGS) : launch_build<M_L2, Q>(COLTT_LB_ARGS)
    COLTT_DISPATCH_QUANT(x->quant, COLTT_LB)
#undef COLTT_LB
#undef COLTT_LB_ARGS
    COLTT_TRY(rc);
    struct { uint32_t counter, n_req, pad0, pad1; unsigned long long st[6]; } hm;
    COLTT_HIP(hipMemcpyAsync(&hm, x->w_misc.p, sizeof(hm), hipMemcpyDeviceToHost, x->stream));
    COLTT_HIP(hipStreamSynchronize(x->stream));
    if (hm.st[4]) {  // phase A queued link requests on head[] before tripping: drop them so the next batch starts clean
      fill_u32_kernel<<<ceil_div(x->head_cap, 256), 256, 0, x->stream>>>(x->b_head.as<uint32_t>(), x->head_cap, NBR_NONE);
      (void)hipStreamSynchronize(x->stream);
      return fail(COLTT_E_DEVICE, "hnsw insert: traversal watchdog tripped (code %llu)", hm.st[4]);
    }
    if (hm.n_req && x->cfg.algo == 2) {
      // diverse mode: one wave per touched row; its evaluations are counted.  A row that would receive more candidates than the link kernel holds (a hub
      // chosen by > ~1 000 vertices of ONE batch) is found BEFORE anything is applied, and the batch is retried in halves: a smaller batch is another
      // legal schedule of the same Inserts, and the index is untouched by the attempt (the new slots' own rows are rewritten by the retry)
      hnsw_link_count_kernel<<<ceil_div(hm.n_req, 256), 256, 0, x->stream>>>(x->b_req.as<BuildReq>(), hm.n_req, x->b_head.as<uint32_t>(), x->cap, (uint32_t)x->cfg.m_max0,
                                                                            (uint32_t)x->cfg.m_max, d_stats);
      COLTT_HIP(hipMemcpyAsync(&hm, x->w_misc.p, sizeof(hm), hipMemcpyDeviceToHost, x->stream));
      COLTT_HIP(hipStreamSynchronize(x->stream));
      if (hm.st[5] > LINKD_CAND && b > 1) {
        fill_u32_kernel<<<ceil_div(x->head_cap, 256), 256, 0, x->stream>>>(x->b_head.as<uint32_t>(), x->head_cap, NBR_NONE);
        COLTT_HIP(hipStreamSynchronize(x->stream));
        shrink = std::max(1u, b / 2);
        continue;
      }
#define COLTT_LD_ARGS x, x->b_req.as<BuildReq>(), hm.n_req, x->b_head.as<uint32_t>(), d_stats, patch.d_dirty, patch.cap
#define COLTT_LD(Q) rc = x->metric == COLTT_COSINE ? launch_link_diverse<M_COS, Q>(COLTT_LD_ARGS) : launch_link_diverse<M_L2, Q>(COLTT_LD_ARGS)
      COLTT_DISPATCH_QUANT(x->quant, COLTT_LD)
#undef COLTT_LD
#undef COLTT_LD_ARGS
      COLTT_TRY(rc);
      COLTT_HIP(hipMemcpyAsync(&hm, x->w_misc.p, sizeof(hm), hipMemcpyDeviceToHost, x->stream));
      COLTT_HIP(hipStreamSynchronize(x->stream));
      if (hm.st[4]) {
        fill_u32_kernel<<<ceil_div(x->head_cap, 256), 256, 0, x->stream>>>(x->b_head.as<uint32_t>(), x->head_cap, NBR_NONE);
        (void)hipStreamSynchronize(x->stream);
        return fail(COLTT_E_DEVICE, "hnsw insert (diverse selection): a row overflowed the link kernel's %u candidates behind the pre-check", LINKD_CAND);   // (cannot happen)
      }
      shrink = 0;
    } else if (hm.n_req) {
      hnsw_link_kernel<<<ceil_div(hm.n_req, 64), 64, 0, x->stream>>>(x->view(), x->cap, x->b_req.as<BuildReq>(), hm.n_req, x->b_head.as<uint32_t>(), patch.d_dirty, patch.cap);
      COLTT_HIP(hipGetLastError());
    }
    commit_host();
    x->build_stats.n_dist += hm.st[0]; x->build_stats.n_exp += hm.st[1]; x->build_stats.n_hops += hm.st[2]; x->build_stats.n_visit_resets += hm.st[3];
    for (uint32_t j = 0; j < b; j++)  // entrypoint CAS in insertion order (hnsw.go:161-164)
      if (lv[j] > x->entry_level) { x->entry = (int32_t)(base + j); x->entry_level = lv[j]; }
    x->n += b; x->live += b; x->n_upper += up; i += b;
  }
  COLTT_HIP(hipStreamSynchronize(x->stream));
  COLTT_TRY(sync_pq(x));   // the new slots' codes: the blocks below gather them
  return pq_nbr_patch_end(x, patch, first_new, x->n - first_new, nullptr, 0);
}

// the derived neighbour-norm rows of every slot (bulk installs; Insert / Remove maintain them incrementally in their kernels)
int fill_adj_norms(Hnsw* x) {
  if (x->metric != COLTT_COSINE || x->n == 0) return COLTT_OK;
  adj_norms_kernel<<<ceil_div(x->n * x->cfg.m_max0, 256), 256, 0, x->stream>>>(x->view(), 0, x->n);
  COLTT_HIP(hipGetLastError());
  COLTT_HIP(hipStreamSynchronize(x->stream));
  return COLTT_OK;
}

// A failed (re)load must not leave a half-installed index behind: fall back to the empty index (memory-safe, searchable).
void make_empty(Hnsw* x) {
  x->gen++;
  x->n = 0; x->live = 0; x->n_upper = 0; x->entry = -1; x->entry_level = 0; x->any_deleted = false; x->pq_done = 0;
  x->h_levels.clear(); x->h_upper_off.clear(); x->h_del.clear(); x->h_ids.clear(); x->id2slot.clear();
  x->dense = true; x->dense_base = 0;
}

// Installs graph topology + id tables (everything of a bulk load except the vectors) under configuration `c`.
// Transactional: the stream is validated and laid out on the host FIRST; the object (cfg included) is only touched once
// nothing but a device failure can go wrong, and a device failure leaves an EMPTY index, never a half-installed one.
int graph_install(Hnsw* x, const coltt_hnsw_cfg& c, uint64_t n, const uint64_t* ids, const int32_t* levels, const uint8_t* deleted,
                  const int64_t* row_offsets, const int32_t* nbr, const float* nbr_dist, int32_t entry_slot) {
  x->gen++;   // the slots are about to be renumbered
  if (n >= 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_bulk_load: more than 2^31-1 slots");
  if (n && (entry_slot < -1 || entry_slot >= (int64_t)n)) return fail(COLTT_E_INVALID, "hnsw_bulk_load: entry slot out of range");
  const uint32_t W0 = (uint32_t)c.m_max0, WU = (uint32_t)c.m_max;
  uint64_t n_upper = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (levels[i] < 0 || levels[i] > 60) return fail(COLTT_E_INVALID, "hnsw_bulk_load: level %d out of range", levels[i]);
    n_upper += (uint64_t)levels[i];
  }
  std::vector<uint32_t> a0((size_t)n * W0, NBR_NONE), aU((size_t)n_upper * WU, NBR_NONE), uo(n, NBR_NONE);
  std::vector<float> d0((size_t)n * W0, 0.f), dU((size_t)n_upper * WU, 0.f);
  std::vector<uint32_t> h_del((n + 31) / 32, 0u);
  bool any_deleted = false; uint64_t live = 0;
  uint64_t row = 0, up = 0;
  std::vector<std::pair<uint32_t, float>> tmp;
  for (uint64_t i = 0; i < n; i++) {
    bool del = deleted && deleted[i];
    if (del) { h_del[i >> 5] |= 1u << (i & 31); any_deleted = true; } else live++;
    if (levels[i] > 0) { uo[i] = (uint32_t)up; }
    for (int l = 0; l <= levels[i]; l++, row++) {
      int64_t b = row_offsets[row], e = row_offsets[row + 1];
      uint32_t W = l == 0 ? W0 : WU;
      if (e < b || e - b > (int64_t)W) return fail(COLTT_E_INVALID, "hnsw_bulk_load: slot %llu level %d has %lld edges > width %u", (unsigned long long)i, l, (long long)(e - b), W);
      tmp.clear();
      for (int64_t j = b; j < e; j++) {
        if (nbr[j] < 0 || (uint64_t)nbr[j] >= n) return fail(COLTT_E_INVALID, "hnsw_bulk_load: neighbour slot out of range");
        if (levels[nbr[j]] < l) return fail(COLTT_E_INVALID, "hnsw_bulk_load: slot %llu level %d lists a neighbour of lower level", (unsigned long long)i, l);
        tmp.push_back({(uint32_t)nbr[j], nbr_dist ? nbr_dist[j] : 0.f});
      }
      std::sort(tmp.begin(), tmp.end());
      uint32_t* ar = l == 0 ? &a0[(size_t)i * W0] : &aU[(size_t)(up + l - 1) * WU];
      float* dr = l == 0 ? &d0[(size_t)i * W0] : &dU[(size_t)(up + l - 1) * WU];
      for (size_t j = 0; j < tmp.size(); j++) { ar[j] = tmp[j].first; dr[j] = tmp[j].second; }
    }
    up += (uint64_t)levels[i];
  }
  std::unordered_map<uint64_t, uint32_t> id2slot;
  if (ids) {
    id2slot.reserve(n * 2);
    for (uint64_t i = 0; i < n; i++)
      if (!(deleted && deleted[i]) && !id2slot.emplace(ids[i], (uint32_t)i).second) return fail(COLTT_E_INVALID, "hnsw_bulk_load: duplicate id");
  }
  // ---- from here on the object changes.  Buffers only grow; capacities are re-derived under the new row widths.
  const coltt_hnsw_cfg old_cfg = x->cfg;
  const uint64_t old_cap = x->cap, old_ucap = x->ucap;
  const bool old_dense = x->dense;
  x->cfg = c; x->cap = 0; x->ucap = 0; x->dense = (ids == nullptr);
  x->vis_stride = 0;  // the HBM visited workspace is sized by the slot capacity: re-made lazily
  int rc = x->reserve(n, n_upper);
  if (rc != COLTT_OK) { x->cfg = old_cfg; x->cap = old_cap; x->ucap = old_ucap; x->dense = old_dense; return rc; }  // nothing was written
  auto upload = [&]() -> int {
    if (!x->dense) COLTT_HIP(hipMemcpyAsync(x->ids.p, ids, n * 8, hipMemcpyHostToDevice, x->stream));
    if (n) {
      COLTT_HIP(hipMemcpyAsync(x->adj0.p, a0.data(), a0.size() * 4, hipMemcpyHostToDevice, x->stream));
      COLTT_HIP(hipMemcpyAsync(x->adj0_d.p, d0.data(), d0.size() * 4, hipMemcpyHostToDevice, x->stream));
      COLTT_HIP(hipMemcpyAsync(x->upper_off.p, uo.data(), n * 4, hipMemcpyHostToDevice, x->stream));
      COLTT_HIP(hipMemcpyAsync(x->del_bits.p, h_del.data(), h_del.size() * 4, hipMemcpyHostToDevice, x->stream));
      if (n_upper) {
        COLTT_HIP(hipMemcpyAsync(x->adjU.p, aU.data(), aU.size() * 4, hipMemcpyHostToDevice, x->stream));
        COLTT_HIP(hipMemcpyAsync(x->adjU_d.p, dU.data(), dU.size() * 4, hipMemcpyHostToDevice, x->stream));
      }
    }
    COLTT_HIP(hipStreamSynchronize(x->stream));
    return COLTT_OK;
  };
  rc = upload();
  x->id2slot.clear(); x->h_ids.clear(); x->dense_base = 0;
  if (rc != COLTT_OK) { make_empty(x); return rc; }  // device failure mid-install: leave an empty (safe) index
  x->h_levels.assign(levels, levels + n);
  x->h_upper_off = std::move(uo);
  x->h_del = std::move(h_del);
  x->any_deleted = any_deleted; x->live = live;
  if (!x->dense) { x->h_ids.assign(ids, ids + n); x->id2slot = std::move(id2slot); }
  x->n = n; x->n_upper = n_upper; x->pq_done = 0;   // every row is about to be rewritten (the callers upload the vectors next)
  x->entry = n ? entry_slot : -1;
  x->entry_level = x->entry >= 0 ? levels[x->entry] : 0;
  return COLTT_OK;
}

}  // namespace

extern "C" {

int coltt_hnsw_create(uint32_t dim, int metric, int quant, const coltt_hnsw_cfg* cfg, coltt_handle_t* out) {
  return coltt::hnsw_create_on(-1 /* the process default device, selected after the arguments have been validated */, dim, metric, quant, cfg, out);
}

}  // extern "C"

// NewHnsw on an explicit device (collection groups place one shard per GPU)
int coltt::hnsw_create_on(int device, uint32_t dim, int metric, int quant, const coltt_hnsw_cfg* cfg, coltt_handle_t* out) {
  if (!out) return fail(COLTT_E_INVALID, "hnsw_create: out is NULL");
  if (dim == 0 || dim > 8192) return fail(COLTT_E_INVALID, "hnsw_create: dim %u outside [1,8192]", dim);
  if (metric != COLTT_COSINE && metric != COLTT_EUCLIDEAN) return fail(COLTT_E_INVALID, "hnsw_create: bad metric %d", metric);
  if (quant < COLTT_Q_NONE || quant > COLTT_Q_BF16) return fail(COLTT_E_UNSUPPORTED, "not support quantization type");
  auto x = std::make_shared<Hnsw>();
  x->dim = dim; x->metric = metric; x->quant = quant;
  x->stride = ((size_t)dim * quant_bytes(quant) + 15) & ~(size_t)15;
  coltt_hnsw_cfg c = cfg ? *cfg : coltt_hnsw_cfg{16, -1, -1, 20, 200, 0, -1.f, 0, 1};
  if (c.m <= 0) return fail(COLTT_E_INVALID, "hnsw_create: m must be > 0");
  // newHnswConfig defaults (hnsw_config.go:150-160)
  if (c.level_multiplier == -1.f) c.level_multiplier = 1.0f / (float)std::log((double)(float)c.m);
  if (c.m_max == -1) c.m_max = c.m;
  if (c.m_max0 == -1) c.m_max0 = 2 * c.m;
  if (c.algo != 0 && c.algo != 1 && c.algo != COLTT_HNSW_DIVERSE) return fail(COLTT_E_INVALID, "hnsw_create: unknown search algorithm %d", c.algo);
  if (c.algo != 0 && c.extend_candidates)
    return fail(COLTT_E_UNSUPPORTED, "hnsw_create: HeuristicExtendCandidates is undefined behaviour in the reference "
                                     "(priority_queue.go:109-122 aliases the heap array); rejected");
  if (c.m_max < c.m || c.m_max0 < c.m || c.m_max0 > 1024) return fail(COLTT_E_INVALID, "hnsw_create: need m <= mMax, m <= mMax0 <= 1024");
  if (c.ef <= 0 || c.ef_construction <= 0) return fail(COLTT_E_INVALID, "hnsw_create: ef and efConstruction must be > 0");
  x->cfg = c;
  x->r8 = rows8_shape(dim, quant);
  const bool shadow_ok = x->r8 && quant == COLTT_Q_NONE && metric == COLTT_COSINE && rows_h_shape((int)dim) && policy().row_shadow;
  x->shadow = shadow_ok && (policy().row_shadow_bits & 16) != 0;
  x->shadow8 = shadow_ok && (policy().row_shadow_bits & 8) != 0;
  COLTT_DEVICE(device); device = coltt_dev_scope_.device();
  x->device = device;
  COLTT_HIP(hipStreamCreateWithFlags(&x->stream, hipStreamNonBlocking));
  *out = Registry::get().add(x);
  return COLTT_OK;
}

extern "C" {

int coltt_hnsw_destroy(coltt_handle_t h) {
  if (!Registry::get().erase(h)) return fail(COLTT_E_NOT_FOUND, "hnsw_destroy: unknown handle");
  return COLTT_OK;
}

int coltt_hnsw_get_cfg(coltt_handle_t h, coltt_hnsw_cfg* out) {
  auto x = lookup<Hnsw>(h);
  if (!x || !out) return fail(COLTT_E_NOT_FOUND, "hnsw_get_cfg: unknown handle");
  ReadLock g(x->rw);
  *out = x->cfg;
  return COLTT_OK;
}

int coltt_hnsw_random_level(coltt_handle_t h, float u, int32_t* out_level) {
  auto x = lookup<Hnsw>(h);
  if (!x || !out_level) return fail(COLTT_E_NOT_FOUND, "hnsw_random_level: unknown handle");
  ReadLock g(x->rw);
  if (!(u > 0.f && u < 1.f)) return fail(COLTT_E_INVALID, "hnsw_random_level: u must be in (0,1)");
  const float lg = (float)std::log((double)u);       // gomath.Log
  const float v = -lg * x->cfg.level_multiplier;      // RandomExponential (f32 multiply)
  *out_level = (int32_t)std::floor((double)v);        // gomath.Floor
  return COLTT_OK;
}

int coltt_hnsw_len(coltt_handle_t h, uint64_t* out) {
  auto x = lookup<Hnsw>(h);
  if (!x || !out) return fail(COLTT_E_NOT_FOUND, "hnsw_len: unknown handle");
  ReadLock g(x->rw);
  *out = x->live;
  return COLTT_OK;
}

int coltt_hnsw_bulk_load(coltt_handle_t h, uint64_t n, const uint64_t* ids, const int32_t* levels, const uint8_t* deleted,
                         const float* vectors, const int64_t* row_offsets, const int32_t* nbr, const float* nbr_dist,
                         int32_t entry_slot) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_bulk_load: unknown handle");
  if (n && (!levels || !vectors || !row_offsets)) return fail(COLTT_E_INVALID, "hnsw_bulk_load: NULL input");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  x->pq_nbr_stale.store(true);
  COLTT_TRY(graph_install(x.get(), x->cfg, n, ids, levels, deleted, row_offsets, nbr, nbr_dist, entry_slot));
  auto upload_vectors = [&]() -> int {
    // vectors in chunks through a staging buffer: Normalize (cosine) + Lower, as Insert does (hnsw.go:105-107)
    const uint64_t chunk = std::max<uint64_t>(1, (256ull << 20) / ((uint64_t)x->dim * 4));
    COLTT_TRY(x->w_raw.reserve(std::min<uint64_t>(chunk, n) * x->dim * 4));
    for (uint64_t b = 0; b < n; b += chunk) {
      uint64_t m = std::min<uint64_t>(chunk, n - b);
      COLTT_HIP(hipMemcpyAsync(x->w_raw.p, vectors + b * x->dim, m * x->dim * 4, hipMemcpyHostToDevice, x->stream));
      COLTT_TRY(prep_rows_any(x.get(), x->w_raw.as<float>(), m, b, x->metric == COLTT_COSINE));
      COLTT_HIP(hipStreamSynchronize(x->stream));
    }
    return COLTT_OK;
  };
  if (n) { int rc = upload_vectors(); if (rc == COLTT_OK) rc = fill_adj_norms(x.get()); if (rc == COLTT_OK) rc = sync_pq(x.get()); if (rc != COLTT_OK) { make_empty(x.get()); return rc; } }
  return COLTT_OK;
}

// ---- Hnsw.Commit / Hnsw.Load (core/vectorindex/hnsw_commit.go:69-278) ------------------------------------------------
namespace {
struct BEW {
  uint8_t* p; uint64_t cap, n = 0;
  void put(const void* s, size_t k) { if (p && n + k <= cap) std::memcpy(p + n, s, k); n += k; }
  void u8(uint8_t v) { put(&v, 1); }
  void u16(uint16_t v) { uint8_t b[2] = {(uint8_t)(v >> 8), (uint8_t)v}; put(b, 2); }
  void u32(uint32_t v) { uint8_t b[4]; for (int i = 0; i < 4; i++) b[i] = (uint8_t)(v >> (8 * (3 - i))); put(b, 4); }
  void u64(uint64_t v) { uint8_t b[8]; for (int i = 0; i < 8; i++) b[i] = (uint8_t)(v >> (8 * (7 - i))); put(b, 8); }
  void f32(float f) { uint32_t u; std::memcpy(&u, &f, 4); u32(u); }
};
struct BER {
  const uint8_t* p; uint64_t n, i = 0; bool ok = true;
  bool need(uint64_t k) { if (i + k > n) { ok = false; return false; } return true; }
  uint8_t u8() { if (!need(1)) return 0; return p[i++]; }
  uint16_t u16() { if (!need(2)) return 0; uint16_t v = (uint16_t)((p[i] << 8) | p[i + 1]); i += 2; return v; }
  uint32_t u32() { if (!need(4)) return 0; uint32_t v = 0; for (int k = 0; k < 4; k++) v = (v << 8) | p[i + k]; i += 4; return v; }
  uint64_t u64() { if (!need(8)) return 0; uint64_t v = 0; for (int k = 0; k < 8; k++) v = (v << 8) | p[i + k]; i += 8; return v; }
  float f32() { uint32_t u = u32(); float f; std::memcpy(&f, &u, 4); return f; }
};
// big-endian f32 vectors at arbitrary byte offsets of the uploaded stream chunk -> f32 staging rows (Vector.Load, edge/constants.go:115-122)
__global__ void be_rows_kernel(const uint8_t* __restrict__ chunk, const uint64_t* __restrict__ offs, uint64_t m, int dim, float* __restrict__ out) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * (uint64_t)dim) return;
  uint64_t i = t / dim; int e = (int)(t - i * dim);
  const uint8_t* s = chunk + offs[i] + (size_t)e * 4;
  uint32_t u = ((uint32_t)s[0] << 24) | ((uint32_t)s[1] << 16) | ((uint32_t)s[2] << 8) | s[3];
  out[t] = __uint_as_float(u);
}
// stored 2-byte codes -> the f32 values they stand for (exact), for the f32 vertex section of Commit
__global__ void decode_rows16_kernel(const uint8_t* __restrict__ rows, size_t stride, uint64_t first, uint64_t m, int dim, float* __restrict__ out) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * (uint64_t)dim) return;
  uint64_t i = t / dim; int e = (int)(t - i * dim);
  out[t] = dev::f16bits_to_f32(*reinterpret_cast<const unsigned short*>(rows + (first + i) * stride + (size_t)e * 2));
}
}  // namespace

int coltt_hnsw_load(coltt_handle_t h, int header, const uint8_t* buf, uint64_t len, uint64_t* out_n, uint64_t* out_ids,
                    uint64_t* out_meta_off, uint32_t* out_meta_len, uint64_t cap_n) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_load: unknown handle");
  if (!buf && len) return fail(COLTT_E_INVALID, "hnsw_load: NULL buffer");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  x->pq_nbr_stale.store(true);
  BER r{buf, len};
  coltt_hnsw_cfg c = x->cfg;  // committed by graph_install only after the whole stream has been parsed and validated
  if (header) {  // hnswConfig.load (hnsw_config.go:205-245), dim, distIdx (hnsw_commit.go:165-183)
    c.algo = (int32_t)r.u32(); c.level_multiplier = r.f32(); c.ef = (int32_t)r.u32(); c.ef_construction = (int32_t)r.u32();
    c.m = (int32_t)r.u32(); c.m_max = (int32_t)r.u32(); c.m_max0 = (int32_t)r.u32();
    uint32_t dim = r.u32(); uint8_t di = r.u8();
    if (!r.ok) return fail(COLTT_E_INVALID, "hnsw_load: truncated header");
    if (di != 1 && di != 2) return fail(COLTT_E_INVALID, "Invalid space type");  // InvalidSpaceTypeErr
    if (dim != x->dim) return fail(COLTT_E_INVALID, "hnsw_load: stream dim %u != index dim %u", dim, x->dim);
    if ((di == 1) != (x->metric == COLTT_COSINE)) return fail(COLTT_E_INVALID, "hnsw_load: stream distance differs from the index's");
    if (c.m <= 0 || c.m_max < c.m || c.m_max0 < c.m || c.m_max0 > 1024 || c.ef <= 0 || c.ef_construction <= 0 || (c.algo != 0 && c.algo != 1 && c.algo != COLTT_HNSW_DIVERSE))
      return fail(COLTT_E_INVALID, "hnsw_load: invalid config in stream");
  }
  std::vector<uint64_t> ids, voff, moff; std::vector<int32_t> levels; std::vector<uint32_t> mlen;
  uint64_t entry_id = 0; bool empty = r.i >= len;
  if (!empty) {
    entry_id = r.u64();
    for (int s = 0; s < 16 && r.ok; s++) {
      uint32_t cnt = r.u32();
      for (uint32_t i = 0; i < cnt && r.ok; i++) {
        ids.push_back(r.u64()); levels.push_back((int32_t)r.u32());
        voff.push_back(r.i); r.need((uint64_t)x->dim * 4); r.i += (uint64_t)x->dim * 4;
        uint64_t m0 = r.i; uint16_t pairs = r.u16();
        for (uint16_t p = 0; p < pairs && r.ok; p++) { uint8_t kl = r.u8(); r.need(kl); r.i += kl; uint16_t vl = r.u16(); r.need(vl); r.i += vl; }
        moff.push_back(m0); mlen.push_back((uint32_t)(r.i - m0));
        if (levels.back() < 0 || levels.back() > 60) return fail(COLTT_E_INVALID, "hnsw_load: bad level in stream");
      }
    }
  }
  if (!r.ok) return fail(COLTT_E_INVALID, "hnsw_load: truncated vertex section");
  const uint64_t n = ids.size();
  std::unordered_map<uint64_t, int32_t> slot; slot.reserve(n * 2);
  for (uint64_t i = 0; i < n; i++) if (!slot.emplace(ids[i], (int32_t)i).second) return fail(COLTT_E_INVALID, "hnsw_load: duplicate id in stream");
  int32_t entry = -1;
  if (n) { auto it = slot.find(entry_id); if (it == slot.end()) return fail(COLTT_E_INVALID, "hnsw_load: entrypoint id not in stream"); entry = it->second; }
  // edges -> per (slot, level) lists, then CSR in slot-major / level-minor order
  std::vector<int64_t> row_of(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) row_of[i + 1] = row_of[i] + levels[i] + 1;
  std::vector<std::vector<std::pair<int32_t, float>>> rows((size_t)row_of[n]);
  for (uint64_t k = 0; k < n && r.ok; k++) {
    uint64_t id = r.u64();
    auto it = slot.find(id);
    if (!r.ok || it == slot.end()) return fail(COLTT_E_INVALID, "hnsw_load: edge record for an unknown vertex");
    int32_t s = it->second;
    for (int l = levels[s]; l >= 0; l--) {
      uint32_t c = r.u32();
      auto& lst = rows[(size_t)row_of[s] + l];
      for (uint32_t j = 0; j < c && r.ok; j++) {
        uint64_t nid = r.u64(); float d = r.f32();
        auto nit = slot.find(nid);
        if (nit == slot.end()) return fail(COLTT_E_INVALID, "hnsw_load: edge to an unknown vertex");
        lst.push_back({nit->second, d});
      }
    }
  }
  if (!r.ok) return fail(COLTT_E_INVALID, "hnsw_load: truncated edge section");
  std::vector<int64_t> offs(rows.size() + 1, 0);
  for (size_t i = 0; i < rows.size(); i++) offs[i + 1] = offs[i] + (int64_t)rows[i].size();
  std::vector<int32_t> nbr((size_t)offs.back()); std::vector<float> nd((size_t)offs.back());
  for (size_t i = 0; i < rows.size(); i++)
    for (size_t j = 0; j < rows[i].size(); j++) { nbr[(size_t)offs[i] + j] = rows[i][j].first; nd[(size_t)offs[i] + j] = rows[i][j].second; }
  COLTT_TRY(graph_install(x.get(), c, n, n ? ids.data() : nullptr, levels.data(), nullptr, offs.data(), nbr.data(), nd.data(), entry));
  // vectors: upload the stream in chunks, byte-swap on the device; stored vectors are NOT re-normalised (hnsw_commit.go:217-220)
  auto upload_vectors = [&]() -> int {
    const uint64_t rows_per = std::max<uint64_t>(1, (128ull << 20) / ((uint64_t)x->dim * 4));
    DevBuf d_chunk, d_offs;
    for (uint64_t b = 0; b < n; b += rows_per) {
      uint64_t m = std::min<uint64_t>(rows_per, n - b);
      uint64_t lo = voff[b], hi = voff[b + m - 1] + (uint64_t)x->dim * 4;
      std::vector<uint64_t> rel(m);
      for (uint64_t i = 0; i < m; i++) rel[i] = voff[b + i] - lo;
      COLTT_TRY(d_chunk.reserve(hi - lo)); COLTT_TRY(d_offs.reserve(m * 8)); COLTT_TRY(x->w_raw.reserve(m * x->dim * 4));
      COLTT_HIP(hipMemcpyAsync(d_chunk.p, buf + lo, hi - lo, hipMemcpyHostToDevice, x->stream));
      COLTT_HIP(hipMemcpyAsync(d_offs.p, rel.data(), m * 8, hipMemcpyHostToDevice, x->stream));
      be_rows_kernel<<<ceil_div(m * x->dim, 256), 256, 0, x->stream>>>(d_chunk.as<uint8_t>(), d_offs.as<uint64_t>(), m, (int)x->dim, x->w_raw.as<float>());
      COLTT_TRY(prep_rows_any(x.get(), x->w_raw.as<float>(), m, b, false));
      COLTT_HIP(hipStreamSynchronize(x->stream));
    }
    return COLTT_OK;
  };
  if (n) { int rc = upload_vectors(); if (rc == COLTT_OK) rc = fill_adj_norms(x.get()); if (rc == COLTT_OK) rc = sync_pq(x.get()); if (rc != COLTT_OK) { make_empty(x.get()); return rc; } }
  if (out_n) *out_n = n;
  for (uint64_t i = 0; i < n && i < cap_n; i++) {
    if (out_ids) out_ids[i] = ids[i];
    if (out_meta_off) out_meta_off[i] = moff[i];
    if (out_meta_len) out_meta_len[i] = mlen[i];
  }
  return COLTT_OK;
}

int coltt_hnsw_entry_level(coltt_handle_t h, int32_t* out_level) {
  auto x = lookup<Hnsw>(h);
  if (!x || !out_level) return fail(COLTT_E_NOT_FOUND, "hnsw_entry_level: unknown handle");
  ReadLock g(x->rw);
  *out_level = x->entry >= 0 ? x->entry_level : -1;
  return COLTT_OK;
}

int coltt_hnsw_commit(coltt_handle_t h, int header, const uint8_t* const* meta_blobs, const uint32_t* meta_lens, uint64_t n_meta,
                      uint8_t* out, uint64_t cap, uint64_t* out_len) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_commit: unknown handle");
  if (!out_len) return fail(COLTT_E_INVALID, "hnsw_commit: out_len is NULL");
  // The reference stream stores f32 vectors (hnsw_commit.go:100-112).  A binary16 ("f16" / "bf16") index writes the values its codes stand
  // for — exact — and Load into an index of the same quantisation encodes them back to the same codes (encode(decode(c)) == c for every
  // non-NaN binary16 code; tests/test_oracle.py checks all 65 536), so the round trip is bit-identical and the stream stays readable by
  // the reference.  The "f8" codec is not idempotent (decode -> encode -> decode changes 128 of its 256 codes): no stream can carry it.
  if (x->quant == COLTT_Q_F8) return fail(COLTT_E_UNSUPPORTED, "hnsw_commit: the reference stream stores f32 vectors and the f8 codec does not round-trip through them; f8 indexes are not committable");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  BEW w{out, out ? cap : 0};
  if (header) {  // hnswConfig.save (hnsw_config.go:179-203) + dim + distIdx (hnsw_commit.go:70-80)
    w.u32((uint32_t)x->cfg.algo); w.f32(x->cfg.level_multiplier); w.u32((uint32_t)x->cfg.ef); w.u32((uint32_t)x->cfg.ef_construction);
    w.u32((uint32_t)x->cfg.m); w.u32((uint32_t)x->cfg.m_max); w.u32((uint32_t)x->cfg.m_max0);
    w.u32(x->dim); w.u8(x->metric == COLTT_COSINE ? 1 : 2);
  }
  if (x->live == 0) { *out_len = w.n; return (out && w.n > cap) ? fail(COLTT_E_INVALID, "hnsw_commit: buffer too small") : COLTT_OK; }
  if (x->entry < 0) return fail(COLTT_E_INVALID, "hnsw_commit: no entrypoint");  // NoEntrypointErr
  const uint64_t n = x->n;
  const uint32_t W0 = (uint32_t)x->cfg.m_max0, WU = (uint32_t)x->cfg.m_max;
  auto id_of = [&](uint64_t s) { return x->dense ? x->dense_base + s : x->h_ids[s]; };
  auto dead = [&](uint64_t s) { return (x->h_del[s >> 5] >> (s & 31)) & 1u; };
  std::vector<std::vector<uint32_t>> shards(16);
  for (uint64_t s = 0; s < n; s++) if (!dead(s)) shards[shard_vertex(id_of(s), 16)].push_back((uint32_t)s);
  w.u64(id_of((uint64_t)x->entry));
  // section 1: vertices (rows fetched from HBM in blocks)
  std::vector<float> rowbuf;
  const uint64_t blk = std::max<uint64_t>(1, (64ull << 20) / ((uint64_t)x->dim * 4));
  std::vector<float> all;  // sized only when actually writing
  if (out) { all.resize(n * (size_t)x->dim);
    DevBuf d_dec;
    for (uint64_t b = 0; b < n; b += blk) { uint64_t m = std::min<uint64_t>(blk, n - b);
      if (x->quant == COLTT_Q_NONE && !x->r8)
        COLTT_HIP(hipMemcpy2D(all.data() + b * x->dim, (size_t)x->dim * 4, x->rows.as<uint8_t>() + b * x->stride, x->stride, (size_t)x->dim * 4, m, hipMemcpyDeviceToHost));
      else {
        COLTT_TRY(d_dec.reserve(m * x->dim * 4));
        if (x->quant == COLTT_Q_NONE) rows_to_f32_kernel<Q_NONE, true><<<ceil_div(m * x->dim, 256), 256, 0, nullptr>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, d_dec.as<float>());
        else if (x->r8) rows_to_f32_kernel<Q_F16, true><<<ceil_div(m * x->dim, 256), 256, 0, nullptr>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, d_dec.as<float>());
        else decode_rows16_kernel<<<ceil_div(m * x->dim, 256), 256, 0, nullptr>>>(x->rows.as<uint8_t>(), x->stride, b, m, (int)x->dim, d_dec.as<float>());
        COLTT_HIP(hipGetLastError());
        COLTT_HIP(hipMemcpy(all.data() + b * x->dim, d_dec.p, m * x->dim * 4, hipMemcpyDeviceToHost));
      } } }
  for (auto& sh : shards) {
    w.u32((uint32_t)sh.size());
    for (uint32_t s : sh) {
      w.u64(id_of(s)); w.u32((uint32_t)x->h_levels[s]);
      if (out) for (uint32_t e = 0; e < x->dim; e++) w.f32(all[(size_t)s * x->dim + e]); else w.n += (uint64_t)x->dim * 4;
      if (meta_blobs && meta_lens && s < n_meta && meta_blobs[s] && meta_lens[s] >= 2) w.put(meta_blobs[s], meta_lens[s]); else w.u16(0);
    }
  }
  // section 2: edges, highest level first, tombstoned neighbours skipped (hnsw_commit.go:133-157)
  std::vector<uint32_t> a0((size_t)n * W0), aU((size_t)x->n_upper * WU); std::vector<float> d0(a0.size()), dU(aU.size());
  if (n) { COLTT_HIP(hipMemcpy(a0.data(), x->adj0.p, a0.size() * 4, hipMemcpyDeviceToHost)); COLTT_HIP(hipMemcpy(d0.data(), x->adj0_d.p, d0.size() * 4, hipMemcpyDeviceToHost)); }
  if (x->n_upper) { COLTT_HIP(hipMemcpy(aU.data(), x->adjU.p, aU.size() * 4, hipMemcpyDeviceToHost)); COLTT_HIP(hipMemcpy(dU.data(), x->adjU_d.p, dU.size() * 4, hipMemcpyDeviceToHost)); }
  for (auto& sh : shards)
    for (uint32_t s : sh) {
      w.u64(id_of(s));
      for (int l = x->h_levels[s]; l >= 0; l--) {
        uint32_t W = l == 0 ? W0 : WU;
        const uint32_t* row = l == 0 ? &a0[(size_t)s * W0] : &aU[((size_t)x->h_upper_off[s] + l - 1) * WU];
        const float* dr = l == 0 ? &d0[(size_t)s * W0] : &dU[((size_t)x->h_upper_off[s] + l - 1) * WU];
        uint32_t c = 0;
        for (uint32_t j = 0; j < W && row[j] != NBR_NONE; j++) if (!dead(row[j])) c++;
        w.u32(c);
        for (uint32_t j = 0; j < W && row[j] != NBR_NONE; j++) { if (dead(row[j])) continue; w.u64(id_of(row[j])); w.f32(dr[j]); }
      }
    }
  *out_len = w.n;
  if (out && w.n > cap) return fail(COLTT_E_INVALID, "hnsw_commit: buffer of %llu bytes is too small for %llu", (unsigned long long)cap, (unsigned long long)w.n);
  return COLTT_OK;
}

int coltt_hnsw_search(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, uint32_t ef_override,
                      uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_search: unknown handle");
  if (nq && (!queries || !out_ids || !out_scores || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_search: NULL buffer");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return search_common(x.get(), ctx.c, queries, false, nq, k, ef_override, out_ids, out_scores, out_counts, stats);
}

int coltt_hnsw_search_device(coltt_handle_t h, const float* d_queries, size_t nq, uint32_t k, uint32_t ef_override,
                             uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_counts, coltt_hnsw_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_search_device: unknown handle");
  if (nq && (!d_queries || !d_out_ids || !d_out_scores || !d_out_counts)) return fail(COLTT_E_INVALID, "hnsw_search_device: NULL buffer");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return search_common(x.get(), ctx.c, d_queries, true, nq, k, ef_override, d_out_ids, d_out_scores, d_out_counts, stats);
}


int coltt_hnsw_insert(coltt_handle_t h, uint64_t id, const float* vec, int32_t level) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_insert: unknown handle");
  if (!vec) return fail(COLTT_E_INVALID, "hnsw_insert: NULL vector");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  COLTT_TRY(x->w_raw.reserve((size_t)x->dim * 4));
  COLTT_HIP(hipMemcpyAsync(x->w_raw.p, vec, (size_t)x->dim * 4, hipMemcpyHostToDevice, x->stream));
  return insert_core(x.get(), &id, 0, x->w_raw.as<float>(), &level, 1, 1);
}

int coltt_hnsw_insert_batch_device(coltt_handle_t h, const uint64_t* ids, uint64_t first_id, const float* d_vecs,
                                   const int32_t* levels, size_t n, uint32_t batch) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_insert_batch_device: unknown handle");
  if (n && (!d_vecs || !levels)) return fail(COLTT_E_INVALID, "hnsw_insert_batch_device: NULL input");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  return insert_core(x.get(), ids, first_id, d_vecs, levels, n, batch);
}

int coltt_hnsw_remove(coltt_handle_t h, uint64_t id) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_remove: unknown handle");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  uint32_t vi;
  if (x->dense) {
    if (id < x->dense_base || id >= x->dense_base + x->n) return fail(COLTT_E_NOT_FOUND, "Item not found");
    vi = (uint32_t)(id - x->dense_base);
    if ((x->h_del[vi >> 5] >> (vi & 31)) & 1u) return fail(COLTT_E_NOT_FOUND, "Item not found");
  } else {
    auto it = x->id2slot.find(id);
    if (it == x->id2slot.end()) return fail(COLTT_E_NOT_FOUND, "Item not found");  // ItemNotFoundError (hnsw.go:317)
    vi = it->second;
    x->id2slot.erase(it);
  }
  const PqNbrPatch patch = pq_nbr_patch_begin(x.get(), 0);   // the neighbours' level-0 rows are about to be re-pruned: stale until their blocks are re-gathered below
  // removeVertex: delete from the map, set the deleted flag (hnsw.go:304-318)
  x->h_del[vi >> 5] |= 1u << (vi & 31);
  x->any_deleted = true; x->live--;
  COLTT_HIP(hipMemcpyAsync(x->del_bits.as<uint32_t>() + (vi >> 5), &x->h_del[vi >> 5], 4, hipMemcpyHostToDevice, x->stream));
  // the removed vertex's own rows
  const int L = x->h_levels[vi];
  const uint32_t W0 = (uint32_t)x->cfg.m_max0, WU = (uint32_t)x->cfg.m_max;
  std::vector<std::vector<uint32_t>> nb(L + 1);
  std::vector<std::vector<float>> nd(L + 1);
  for (int l = 0; l <= L; l++) {
    uint32_t W = l == 0 ? W0 : WU;
    nb[l].resize(W); nd[l].resize(W);
    const uint32_t* src = l == 0 ? x->adj0.as<uint32_t>() + (size_t)vi * W0 : x->adjU.as<uint32_t>() + ((size_t)x->h_upper_off[vi] + l - 1) * WU;
    const float* dsrc = l == 0 ? x->adj0_d.as<float>() + (size_t)vi * W0 : x->adjU_d.as<float>() + ((size_t)x->h_upper_off[vi] + l - 1) * WU;
    COLTT_HIP(hipMemcpyAsync(nb[l].data(), src, W * 4, hipMemcpyDeviceToHost, x->stream));
    COLTT_HIP(hipMemcpyAsync(nd[l].data(), dsrc, W * 4, hipMemcpyDeviceToHost, x->stream));
  }
  COLTT_HIP(hipStreamSynchronize(x->stream));
  if (x->entry == (int32_t)vi) {  // new entrypoint: closest neighbour on the highest level that has any (hnsw.go:197-217)
    float minD = 3.40282346638528859811704183484516925440e+38f;
    int32_t closest = -1;
    for (int l = L; l >= 0; l--) {
      for (size_t j = 0; j < nb[l].size() && nb[l][j] != NBR_NONE; j++)
        if (nd[l][j] < minD) { minD = nd[l][j]; closest = (int32_t)nb[l][j]; }
      if (closest >= 0) break;
    }
    x->entry = closest;
    x->entry_level = closest >= 0 ? x->h_levels[closest] : 0;
  }
  // every neighbour drops the back-edge and is re-pruned (hnsw.go:219-238)
  std::vector<uint32_t> t_nb; std::vector<int32_t> t_lv;
  for (int l = L; l >= 0; l--)
    for (size_t j = 0; j < nb[l].size() && nb[l][j] != NBR_NONE; j++) { t_nb.push_back(nb[l][j]); t_lv.push_back(l); }
  if (!t_nb.empty()) {
    COLTT_TRY(x->b_req.reserve(t_nb.size() * 8));
    uint32_t* d_nb = x->b_req.as<uint32_t>();
    int32_t* d_lv = reinterpret_cast<int32_t*>(d_nb + t_nb.size());
    COLTT_HIP(hipMemcpyAsync(d_nb, t_nb.data(), t_nb.size() * 4, hipMemcpyHostToDevice, x->stream));
    COLTT_HIP(hipMemcpyAsync(d_lv, t_lv.data(), t_lv.size() * 4, hipMemcpyHostToDevice, x->stream));
    hnsw_unlink_kernel<<<ceil_div(t_nb.size(), 64), 64, 0, x->stream>>>(x->view(), d_nb, d_lv, (uint32_t)t_nb.size());
    COLTT_HIP(hipGetLastError());
  }
  COLTT_HIP(hipStreamSynchronize(x->stream));
  // the rows the kernel compacted at level 0 are the removed vertex's level-0 neighbours: the tail of t_nb (levels descend), already on the device
  uint32_t n_l0 = 0;
  while (n_l0 < t_lv.size() && t_lv[t_lv.size() - 1 - n_l0] == 0) n_l0++;
  return pq_nbr_patch_end(x.get(), patch, 0, 0, n_l0 ? x->b_req.as<uint32_t>() + (t_nb.size() - n_l0) : nullptr, n_l0);
}

// ---- HNSW compaction (include/coltt_gpu.h, "HNSW compaction"; kernels and the hazard argument: hnsw_compact.hpp) --------------------------
int coltt_hnsw_compact_map_host(const uint32_t* del_bits, uint64_t n_slots, const int32_t* levels, uint32_t* out_new_of_old,
                                uint32_t* out_new_upper_off, uint64_t* out_live, uint64_t* out_upper_rows) {
  if (n_slots >= 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_compact_map_host: more than 2^31-1 slots");
  if (n_slots && !levels && (out_new_upper_off || out_upper_rows)) return fail(COLTT_E_INVALID, "hnsw_compact_map_host: the upper-row outputs need levels");
  compact::map_host(del_bits, n_slots, levels, out_new_of_old, out_new_upper_off, out_live, out_upper_rows);
  return COLTT_OK;
}

}  // extern "C"

namespace {

// what coltt_hnsw_compact_carry adds to a compaction: the listed filters and columns come out valid at the new generation
struct CarryReq {
  const coltt_handle_t* filters; size_t n_filters; uint64_t* out_allowed;
  const coltt_handle_t* columns; size_t n_columns; uint64_t* out_set;
  coltt_hnsw_carry_stats* stats;
};

// a carried filter takes its new bitmap and list (slices of `slab`; nullptr: the empty filter) and lets go of what it had
void filter_install(HnswFilter* f, const std::shared_ptr<FilterSlab>& slab, uint32_t* bits, uint32_t* list, uint32_t slots, uint64_t allowed, uint64_t gen) {
  if (f->slab) { f->bits.p = nullptr; f->list.p = nullptr; }   // slices of a shared slab: its siblings keep it
  else { if (f->bits.p) (void)hipFree(f->bits.p); if (f->list.p) (void)hipFree(f->list.p); }
  f->slab = slab;
  f->bits.p = bits; f->bits.cap = bits ? ((size_t)slots + 31) / 32 * 4 : 0;
  f->list.p = allowed ? list : nullptr; f->list.cap = (size_t)allowed * 4;
  f->slots = slots; f->allowed = allowed; f->gen = gen;
}

// coltt_hnsw_compact and coltt_hnsw_compact_carry (cr != nullptr): one compaction
int compact_common(coltt_handle_t h, const char* who, uint64_t stage_bytes_or_0, const CarryReq* cr, uint32_t* out_new_of_old, uint64_t cap_map,
                   coltt_hnsw_compact_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "%s: unknown handle", who);
  // ---- the objects to carry: handles first, each distinct object once
  std::vector<std::shared_ptr<HnswFilter>> cf;
  std::vector<std::shared_ptr<HnswAttr>> cc;
  std::vector<size_t> f_at, c_at;   // list position -> its object in cf / cc
  if (cr) {
    if (cr->n_filters && !cr->filters) return fail(COLTT_E_INVALID, "%s: filters is NULL with n_filters = %zu", who, cr->n_filters);
    if (cr->n_columns && !cr->columns) return fail(COLTT_E_INVALID, "%s: columns is NULL with n_columns = %zu", who, cr->n_columns);
    std::unordered_map<coltt_handle_t, size_t> seen;
    f_at.resize(cr->n_filters); c_at.resize(cr->n_columns);
    for (size_t i = 0; i < cr->n_filters; i++) {
      auto it = seen.find(cr->filters[i]);
      if (it == seen.end()) {
        auto f = lookup<HnswFilter>(cr->filters[i]);
        if (!f) return fail(COLTT_E_NOT_FOUND, "%s: unknown filter handle at filters[%zu]", who, i);
        if (f->index != h) return fail(COLTT_E_INVALID, "%s: the filter at filters[%zu] was built for another index", who, i);
        it = seen.emplace(cr->filters[i], cf.size()).first;
        cf.push_back(std::move(f));
      }
      f_at[i] = it->second;
    }
    seen.clear();
    for (size_t i = 0; i < cr->n_columns; i++) {
      auto it = seen.find(cr->columns[i]);
      if (it == seen.end()) {
        auto a = lookup<HnswAttr>(cr->columns[i]);
        if (!a) return fail(COLTT_E_NOT_FOUND, "%s: unknown column handle at columns[%zu]", who, i);
        if (a->index != h) return fail(COLTT_E_INVALID, "%s: the column at columns[%zu] belongs to another index", who, i);
        it = seen.emplace(cr->columns[i], cc.size()).first;
        cc.push_back(std::move(a));
      }
      c_at[i] = it->second;
    }
  }
  WriteLock g(x->rw);
  std::vector<WriteLock> clocks;   // index before column: the order of attr_set
  clocks.reserve(cc.size());
  for (auto& a : cc) clocks.emplace_back(a->rw);
  for (size_t i = 0; i < f_at.size(); i++)
    if (cf[f_at[i]]->gen != x->gen) return fail(COLTT_E_INVALID, "%s: the filter at filters[%zu] is stale (the index was renumbered since it was built)", who, i);
  for (size_t i = 0; i < c_at.size(); i++)
    if (cc[c_at[i]]->gen != x->gen) return fail(COLTT_E_INVALID, "%s: the column at columns[%zu] is stale (the index was renumbered since it was created)", who, i);
  COLTT_DEVICE(x->device);
  const uint64_t n = x->n;
  if (out_new_of_old && cap_map < n) return fail(COLTT_E_INVALID, "%s: the map holds %llu entries, the index has %llu slots", who, (unsigned long long)cap_map, (unsigned long long)n);
  coltt_hnsw_compact_stats st{};
  coltt_hnsw_carry_stats cst{};
  cst.filters = cf.size(); cst.columns = cc.size();
  st.slots_before = st.slots_after = n; st.upper_rows_before = st.upper_rows_after = x->n_upper;
  auto report = [&]() {   // the carried objects as they are now
    if (!cr) return;
    if (cr->out_allowed) for (size_t i = 0; i < f_at.size(); i++) cr->out_allowed[i] = cf[f_at[i]]->allowed;
    if (cr->out_set) for (size_t i = 0; i < c_at.size(); i++) cr->out_set[i] = cc[c_at[i]]->n_set;
    if (cr->stats) *cr->stats = cst;
  };
  if (x->live == n) {   // no tombstone: nothing is launched, nothing is renumbered
    if (out_new_of_old) for (uint64_t s = 0; s < n; s++) out_new_of_old[s] = (uint32_t)s;
    if (stats) *stats = st;
    report();
    return COLTT_OK;
  }
  // ---- the plan, from the host mirrors
  std::vector<uint32_t> nmap(n), nuo(x->live);
  uint64_t live = 0, up_after = 0;
  compact::map_host(x->h_del.data(), n, x->h_levels.data(), nmap.data(), nuo.data(), &live, &up_after);
  // Remove elects the removed entrypoint's closest listed neighbour without asking whether it is alive (hnsw.go:197-217): a walk can start from a
  // tombstone, a compacted index cannot — refused before anything changes rather than answered differently
  if (live && x->entry >= 0 && nmap[(size_t)x->entry] == NBR_NONE)
    return fail(COLTT_E_UNSUPPORTED, "%s: the entrypoint (slot %d) is a tombstone; dropping it would change the answers", who, x->entry);
  const size_t words = (size_t)((n + 31) / 32);
  uint64_t first = 0;                                   // the first tombstone: the slots below it keep their numbers
  while (nmap[first] != NBR_NONE) first++;
  std::vector<uint32_t> old_of_new(live), rank(words, 0u), uold(up_after);
  for (uint64_t s = 0; s < n; s++) if (nmap[s] != NBR_NONE) old_of_new[nmap[s]] = (uint32_t)s;
  { uint32_t c = 0; for (size_t w = 0; w < words; w++) { rank[w] = c; const uint64_t in_word = std::min<uint64_t>(32, n - (uint64_t)w * 32);
      const uint32_t mask = in_word == 32 ? 0xffffffffu : ((1u << in_word) - 1u); c += (uint32_t)__builtin_popcount(~x->h_del[w] & mask); } }
  for (uint64_t j = 0; j < live; j++) {
    const uint32_t s = old_of_new[j];
    for (int32_t l = 0; l < x->h_levels[s]; l++) uold[(size_t)nuo[j] + l] = x->h_upper_off[s] + (uint32_t)l;
  }
  uint64_t ufirst = 0;                                  // the first upper row that moves
  while (ufirst < up_after && uold[ufirst] == ufirst) ufirst++;
  st.slots_after = live; st.upper_rows_after = up_after; st.rows_moved = live - first;
  x->pq_nbr_stale.store(true);   // the slots are about to be renumbered: the next walk over the blocks rebuilds them, as after Load
  // new(s) for any s <= n, tombstoned or not: the live slots below s.  Reads the OLD h_del: every use is before the mirrors are rebuilt
  auto new_below = [&](uint64_t s) -> uint64_t {
    if (s >= n) return live;
    return (uint64_t)rank[s >> 5] + (uint64_t)__builtin_popcount(~x->h_del[s >> 5] & ((1u << (s & 31)) - 1u));
  };
  if (live == 0) {               // every vertex is dead: the empty index
    hipError_t e = hipMemsetAsync(x->del_bits.p, 0, words * 4, x->stream);
    for (auto& a : cc)           // a carried column covers no slot; no word of its bitmap past the coverage is set
      if (e == hipSuccess && a->set.p) e = hipMemsetAsync(a->set.p, 0, ((size_t)a->cap + 31) / 32 * 4, x->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(x->stream);
    make_empty(x.get());
    if (e != hipSuccess) return fail(COLTT_E_DEVICE, "%s: %s", who, hipGetErrorString(e));
    for (auto& f : cf) filter_install(f.get(), nullptr, nullptr, nullptr, 0, 0, x->gen);
    for (auto& a : cc) { a->slots = 0; a->n_set = 0; std::fill(a->h_set.begin(), a->h_set.end(), 0u); a->gen = x->gen; }
    if (out_new_of_old) std::copy(nmap.begin(), nmap.end(), out_new_of_old);
    if (stats) *stats = st;
    report();
    return COLTT_OK;
  }
  // ---- what moves.  Per-slot arrays: rows of rb bytes; every allocation is made before the first kernel, so a refused one leaves the index as it was
  struct Move { uint8_t* p; size_t rb; uint64_t end; };   // the new slots [first, end) of this array move
  std::vector<Move> moves;
  moves.push_back({x->rows.as<uint8_t>(), x->stride, live});
  if (x->has_shadow16()) moves.push_back({x->rows_h.as<uint8_t>(), (size_t)x->dim * 2, live});
  if (x->has_shadow8()) { moves.push_back({x->rows_b.as<uint8_t>(), (size_t)x->dim, live}); moves.push_back({x->rows_m.as<uint8_t>(), 8, live}); }
  moves.push_back({x->norms.as<uint8_t>(), 4, live});
  if (!x->dense) moves.push_back({x->ids.as<uint8_t>(), 8, live});
  const bool pq_move = x->pq_on && x->pq_done == n && x->pq_codes.p;   // (writers leave every slot coded; otherwise the codes are made again below)
  if (pq_move) moves.push_back({x->pq_codes.as<uint8_t>(), (size_t)x->pq_row, live});
  // a carried column's values: the new slots below new(covered), whose sources lie below the coverage (new() is monotone)
  // every carried object's new coverage, once, from the old mirrors: new(F.slots), new(covered)
  std::vector<uint32_t> f_cov(cf.size()), c_cov(cc.size());
  for (size_t i = 0; i < cf.size(); i++) f_cov[i] = (uint32_t)new_below(cf[i]->slots);
  for (size_t i = 0; i < cc.size(); i++) c_cov[i] = (uint32_t)new_below(cc[i]->slots);
  for (size_t i = 0; i < cc.size(); i++) {
    HnswAttr* a = cc[i].get();
    const uint64_t end = c_cov[i];
    if (a->vals.p && end > first) { moves.push_back({a->vals.as<uint8_t>(), 8, end}); cst.column_values += end - first; }
  }
  const uint32_t W0 = (uint32_t)x->cfg.m_max0, WU = (uint32_t)x->cfg.m_max;
  const bool with_n = x->metric == COLTT_COSINE, with_m = x->has_shadow8();
  auto region = [](uint64_t rows, uint32_t W, size_t elem) { return ((size_t)rows * W * elem + 255) & ~(size_t)255; };   // one array's share of the staging block
  auto adj_stage = [&](uint64_t rows, uint32_t W, bool level0) {
    return 2 * region(rows, W, 4) + (level0 && with_n ? region(rows, W, 4) : 0) + (level0 && with_m ? region(rows, W, 8) : 0);
  };
  const uint64_t budget = stage_bytes_or_0 ? stage_bytes_or_0 : (64ull << 20);
  // destinations per chunk: max(64, budget / row bytes), no more than there are rows to move, the launch's pieces within a 32-bit grid
  auto chunk_of = [&](size_t rb, uint64_t count) { return std::min<uint64_t>({std::max<uint64_t>(64, budget / rb), std::max<uint64_t>(count, 1), (1ull << 34) / rb}); };
  const uint64_t ch0 = chunk_of((size_t)W0 * 20, live - first), chU = chunk_of((size_t)WU * 8, up_after - ufirst);
  size_t stage_need = 0;
  if (live > first) {
    for (const Move& m : moves) stage_need = std::max(stage_need, (size_t)chunk_of(m.rb, live - first) * m.rb);
    stage_need = std::max(stage_need, adj_stage(ch0, W0, true));
  }
  if (up_after > ufirst) stage_need = std::max(stage_need, adj_stage(chU, WU, false));
  DevBuf d_stage, d_plan;
  const size_t off_rank = ((size_t)live * 4 + 255) & ~(size_t)255, off_uold = off_rank + ((words * 4 + 255) & ~(size_t)255),
               off_cnt = off_uold + (((size_t)up_after * 4 + 255) & ~(size_t)255);
  COLTT_TRY(d_plan.reserve(off_cnt + 256));
  if (stage_need) COLTT_TRY(d_stage.reserve(stage_need));
  if (x->dense) COLTT_TRY(x->ids.reserve(std::max<uint64_t>(x->cap, 1024) * 8, false, x->stream));
  // ---- the carry (filter_carry.hpp): the filters' bitmaps first, then the columns' set bitmaps, in one launch.  The filters' new bitmaps and
  // lists are slices of one slab (lists sized by the OLD allowed counts: no round trip decides an allocation), the columns' new bitmaps go to
  // scratch and are copied over the old ones in stream order.  Everything is allocated here, before the first kernel.
  const size_t nF = cf.size(), nC = cc.size(), nP = nF + nC;
  const uint32_t nw_new = (uint32_t)((live + 31) / 32), c_wg = carry_n_wg(live);
  const size_t c_stride = carry_stride(live);
  if (nP * (uint64_t)c_wg > 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "%s: %zu bitmaps over %llu slots exceed one launch", who, nP, (unsigned long long)live);
  std::shared_ptr<FilterSlab> slab;
  DevBuf d_carry;
  std::vector<CarryMap> h_maps(nP);
  std::vector<uint64_t> h_loff(nF);
  // read-back targets (pageable: the copies are staged and the stream is synchronised before they are read; a column's whole new set bitmap
  // comes back only to refill its h_set mirror — small at present column counts, pinned staging if they grow)
  std::vector<uint32_t> h_cnt(nP * (size_t)c_wg), h_cset(nC * (size_t)nw_new);
  uint64_t list_total = 0;
  const size_t o_loff = ((nP * sizeof(CarryMap)) + 255) & ~(size_t)255, o_cnt = o_loff + ((nF * 8 + 255) & ~(size_t)255),
               o_cbits = o_cnt + ((h_cnt.size() * 4 + 255) & ~(size_t)255);
  if (nP) {
    for (size_t i = 0; i < nF; i++) { h_loff[i] = list_total; list_total += (cf[i]->allowed + 63) & ~63ull; }
    COLTT_TRY(d_carry.reserve(o_cbits + nC * c_stride * 4));
    if (nF) {
      slab = std::make_shared<FilterSlab>();
      slab->device = x->device;
      COLTT_TRY(slab->bits.reserve(nF * c_stride * 4));
      if (list_total) COLTT_TRY(slab->lists.reserve((size_t)list_total * 4));
    }
    for (size_t i = 0; i < nF; i++)
      h_maps[i] = CarryMap{cf[i]->bits.as<uint32_t>(), slab->bits.as<uint32_t>() + i * c_stride, (uint32_t)std::min<uint64_t>(((uint64_t)cf[i]->slots + 31) / 32, words), 0u};
    for (size_t i = 0; i < nC; i++)
      h_maps[nF + i] = CarryMap{cc[i]->set.as<uint32_t>(), reinterpret_cast<uint32_t*>(d_carry.as<uint8_t>() + o_cbits) + i * c_stride,
                                cc[i]->set.p ? (uint32_t)std::min<uint64_t>(((uint64_t)cc[i]->slots + 31) / 32, words) : 0u, 0u};
  }
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  COLTT_HIP(hipEventCreate(&ev0));
  if (hipEventCreate(&ev1) != hipSuccess) { (void)hipEventDestroy(ev0); return fail(COLTT_E_DEVICE, "%s: hipEventCreate", who); }
  if (nP && (hipEventCreate(&ev2) != hipSuccess || hipEventCreate(&ev3) != hipSuccess)) {
    (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1); if (ev2) (void)hipEventDestroy(ev2);
    return fail(COLTT_E_DEVICE, "%s: hipEventCreate", who);
  }
  uint8_t* const plan = d_plan.as<uint8_t>(); uint8_t* const stage = d_stage.as<uint8_t>();
  const uint32_t* d_oon = reinterpret_cast<const uint32_t*>(plan); const uint32_t* d_rank = reinterpret_cast<const uint32_t*>(plan + off_rank);
  const uint32_t* d_uold = reinterpret_cast<const uint32_t*>(plan + off_uold);
  unsigned long long* d_cnt = reinterpret_cast<unsigned long long*>(plan + off_cnt);
  unsigned long long dropped = 0;
  uint64_t bytes = 0;
  // ---- from here on the index changes: a device failure leaves the EMPTY index
  auto run = [&]() -> int {
    hipStream_t s = x->stream;
    COLTT_HIP(hipMemcpyAsync(plan, old_of_new.data(), live * 4, hipMemcpyHostToDevice, s));
    COLTT_HIP(hipMemcpyAsync(plan + off_rank, rank.data(), words * 4, hipMemcpyHostToDevice, s));
    if (up_after) COLTT_HIP(hipMemcpyAsync(plan + off_uold, uold.data(), up_after * 4, hipMemcpyHostToDevice, s));
    COLTT_HIP(hipMemsetAsync(d_cnt, 0, 8, s));
    COLTT_HIP(hipEventRecord(ev0, s));
    // adjacency rows of one level class: rows [0, fst) are rewritten in place, rows [fst, cnt) go through the staging block chunk by chunk
    auto adjacency = [&](uint32_t* ids, float* d, float* nn, float2* mm, uint32_t W, const uint32_t* list, uint64_t fst, uint64_t cnt, uint64_t ch) -> int {
      compact::AdjJob j{};
      j.src_ids = ids; j.src_d = d; j.src_n = nn; j.src_m = mm; j.W = W;
      j.del_bits = x->del_bits.as<uint32_t>(); j.rank = d_rank; j.n_slots = (uint32_t)n; j.dropped = d_cnt;
      const size_t row_b = (size_t)W * (8 + (nn ? 4 : 0) + (mm ? 8 : 0));
      for (uint64_t b = 0; b < fst; b += 1u << 24) {
        j.dst_ids = ids; j.dst_d = d; j.dst_n = nn; j.dst_m = mm; j.src_list = list + b; j.dst_row0 = b; j.m = (uint32_t)std::min<uint64_t>(1u << 24, fst - b);
        compact::compact_adj_kernel<<<compact::adj_grid(j.m), 256, 0, s>>>(j);
        bytes += (uint64_t)j.m * row_b;
      }
      const int vb4 = compact::width_of((size_t)W * 4), vb8 = compact::width_of((size_t)W * 8);
      for (uint64_t b = fst; b < cnt; b += ch) {
        const uint64_t m = std::min<uint64_t>(ch, cnt - b);
        uint8_t* s_ids = stage; uint8_t* s_d = s_ids + region(m, W, 4); uint8_t* s_n = s_d + region(m, W, 4); uint8_t* s_m = s_n + (nn ? region(m, W, 4) : 0);
        j.dst_ids = reinterpret_cast<uint32_t*>(s_ids); j.dst_d = reinterpret_cast<float*>(s_d);
        j.dst_n = nn ? reinterpret_cast<float*>(s_n) : nullptr; j.dst_m = mm ? reinterpret_cast<float2*>(s_m) : nullptr;
        j.src_list = list + b; j.dst_row0 = 0; j.m = (uint32_t)m;
        compact::compact_adj_kernel<<<compact::adj_grid(m), 256, 0, s>>>(j);
        compact::launch_copy(s, s_ids, reinterpret_cast<uint8_t*>(ids + b * W), m * W * 4, vb4);
        compact::launch_copy(s, s_d, reinterpret_cast<uint8_t*>(d + b * W), m * W * 4, vb4);
        if (nn) compact::launch_copy(s, s_n, reinterpret_cast<uint8_t*>(nn + b * W), m * W * 4, vb4);
        if (mm) compact::launch_copy(s, s_m, reinterpret_cast<uint8_t*>(mm + b * W), m * W * 8, vb8);
        bytes += 2 * m * row_b;
      }
      COLTT_HIP(hipGetLastError());
      return COLTT_OK;
    };
    COLTT_TRY(adjacency(x->adj0.as<uint32_t>(), x->adj0_d.as<float>(), with_n ? x->adj0_n.as<float>() : nullptr, with_m ? x->adj0_m.as<float2>() : nullptr,
                        W0, d_oon, first, live, ch0));
    if (up_after) COLTT_TRY(adjacency(x->adjU.as<uint32_t>(), x->adjU_d.as<float>(), nullptr, nullptr, WU, d_uold, ufirst, up_after, chU));
    for (const Move& mv : moves) {
      const uint64_t ch = chunk_of(mv.rb, live - first);
      const int vb = compact::width_of(mv.rb);
      for (uint64_t b = first; b < mv.end; b += ch) {
        const uint64_t m = std::min<uint64_t>(ch, mv.end - b);
        compact::launch_gather(s, mv.p, mv.rb, d_oon + b, m, stage);
        compact::launch_copy(s, stage, mv.p + b * mv.rb, m * mv.rb, vb);
        bytes += 2 * m * mv.rb;
      }
      COLTT_HIP(hipGetLastError());
    }
    if (x->dense) {
      compact::compact_dense_ids_kernel<<<ceil_div(live, 256), 256, 0, s>>>(x->ids.as<uint64_t>(), d_oon, live, x->dense_base);
      COLTT_HIP(hipGetLastError());
      bytes += live * 8;
    }
    if (nP) {   // the carry: reads the old tombstones, the rank table, old_of_new and the old bitmaps; writes the slab and the scratch only
      uint8_t* const cb = d_carry.as<uint8_t>();
      uint32_t* const d_ccnt = reinterpret_cast<uint32_t*>(cb + o_cnt);
      COLTT_HIP(hipMemcpyAsync(cb, h_maps.data(), nP * sizeof(CarryMap), hipMemcpyHostToDevice, s));
      if (nF) COLTT_HIP(hipMemcpyAsync(cb + o_loff, h_loff.data(), nF * 8, hipMemcpyHostToDevice, s));
      COLTT_HIP(hipEventRecord(ev2, s));
      launch_carry(s, reinterpret_cast<const CarryMap*>(cb), (uint32_t)nP, x->del_bits.as<uint32_t>(), (uint32_t)n, d_rank, d_oon, (uint32_t)live, d_ccnt);
      if (list_total)
        filter_compact_kernel<<<(uint32_t)(nF * c_wg), FEX_THREADS, 0, s>>>(slab->bits.as<uint32_t>(), c_stride, nw_new, c_wg, d_ccnt,
                                                                            reinterpret_cast<const uint64_t*>(cb + o_loff), slab->lists.as<uint32_t>());
      COLTT_HIP(hipGetLastError());
      COLTT_HIP(hipEventRecord(ev3, s));
      for (size_t i = 0; i < nC; i++) {   // a column keeps its own bitmap array: the new words over the old, 0 past them
        HnswAttr* a = cc[i].get();
        if (!a->set.p) continue;
        const size_t cap_words = ((size_t)a->cap + 31) / 32;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(cb + o_cbits) + i * c_stride;
        const size_t cw = std::min<size_t>(nw_new, cap_words);   // (the new words past the column's coverage, hence past its capacity, are 0)
        COLTT_HIP(hipMemcpyAsync(a->set.p, src, cw * 4, hipMemcpyDeviceToDevice, s));
        if (cap_words > cw) COLTT_HIP(hipMemsetAsync(a->set.as<uint32_t>() + cw, 0, (cap_words - cw) * 4, s));
        COLTT_HIP(hipMemcpyAsync(h_cset.data() + i * (size_t)nw_new, src, cw * 4, hipMemcpyDeviceToHost, s));
      }
      COLTT_HIP(hipMemcpyAsync(h_cnt.data(), d_ccnt, h_cnt.size() * 4, hipMemcpyDeviceToHost, s));
    }
    COLTT_HIP(hipMemcpyAsync(x->upper_off.p, nuo.data(), live * 4, hipMemcpyHostToDevice, s));
    COLTT_HIP(hipMemsetAsync(x->del_bits.p, 0, words * 4, s));   // last: every launch above read the old tombstones
    COLTT_HIP(hipEventRecord(ev1, s));
    COLTT_HIP(hipMemcpyAsync(&dropped, d_cnt, 8, hipMemcpyDeviceToHost, s));
    COLTT_HIP(hipStreamSynchronize(s));
    COLTT_HIP(hipEventElapsedTime(&st.ms, ev0, ev1));
    if (nP) COLTT_HIP(hipEventElapsedTime(&cst.ms, ev2, ev3));
    return COLTT_OK;
  };
  int rc = run();
  (void)hipEventDestroy(ev0); (void)hipEventDestroy(ev1);
  if (ev2) (void)hipEventDestroy(ev2);
  if (ev3) (void)hipEventDestroy(ev3);
  if (rc != COLTT_OK) { (void)hipStreamSynchronize(x->stream); make_empty(x.get()); return rc; }
  // ---- the host mirrors, from the plan
  std::vector<int32_t> lv(live);
  std::vector<uint64_t> nids(live);
  for (uint64_t j = 0; j < live; j++) { const uint32_t s = old_of_new[j]; lv[j] = x->h_levels[s]; nids[j] = x->dense ? x->dense_base + s : x->h_ids[s]; }
  x->h_levels = std::move(lv); x->h_ids = std::move(nids); x->h_upper_off = std::move(nuo);
  x->h_del.assign((size_t)((live + 31) / 32), 0u);
  x->id2slot.clear(); x->id2slot.reserve(live * 2);
  for (uint64_t j = 0; j < live; j++) x->id2slot[x->h_ids[j]] = (uint32_t)j;
  x->dense = false; x->dense_base = 0;
  x->n = live; x->live = live; x->n_upper = up_after; x->any_deleted = false;
  if (x->entry >= 0) x->entry = (int32_t)nmap[(size_t)x->entry];   // (alive: checked above)
  x->pq_done = pq_move ? live : 0;
  x->gen++;                      // the slots were renumbered: filters built before are stale
  rc = sync_pq(x.get());
  if (rc != COLTT_OK) { make_empty(x.get()); return rc; }
  st.edges_dropped = dropped; st.bytes_moved = bytes;
  // ---- the stream has synchronised: the carried objects take their new data under the same handles (an object that was not listed keeps the
  // old generation and is stale)
  auto count_of = [&](size_t p) { uint64_t a = 0; for (uint32_t t = 0; t < c_wg; t++) a += h_cnt[p * c_wg + t]; return a; };
  for (size_t i = 0; i < nF; i++) {
    const uint64_t a = count_of(i);
    filter_install(cf[i].get(), slab, slab->bits.as<uint32_t>() + i * c_stride, list_total ? slab->lists.as<uint32_t>() + h_loff[i] : nullptr,
                   f_cov[i], a, x->gen);
    cst.list_entries += a;
  }
  for (size_t i = 0; i < nC; i++) {
    HnswAttr* a = cc[i].get();
    a->slots = c_cov[i]; a->n_set = count_of(nF + i); a->gen = x->gen;
    std::fill(a->h_set.begin(), a->h_set.end(), 0u);
    if (a->set.p) std::copy_n(h_cset.begin() + i * (size_t)nw_new, std::min<size_t>(nw_new, a->h_set.size()), a->h_set.begin());
  }
  cst.bitmap_words = (uint64_t)nP * nw_new;
  if (out_new_of_old) std::copy(nmap.begin(), nmap.end(), out_new_of_old);
  if (stats) *stats = st;
  report();
  return COLTT_OK;
}

}  // namespace

extern "C" {

int coltt_hnsw_compact(coltt_handle_t h, uint64_t stage_bytes_or_0, uint32_t* out_new_of_old, uint64_t cap_map, coltt_hnsw_compact_stats* stats) {
  return compact_common(h, "hnsw_compact", stage_bytes_or_0, nullptr, out_new_of_old, cap_map, stats);
}

int coltt_hnsw_compact_carry(coltt_handle_t h, uint64_t stage_bytes_or_0, const coltt_handle_t* filters, size_t n_filters, uint64_t* out_allowed,
                             const coltt_handle_t* columns, size_t n_columns, uint64_t* out_set, uint32_t* out_new_of_old, uint64_t cap_map,
                             coltt_hnsw_compact_stats* stats, coltt_hnsw_carry_stats* carry) {
  const CarryReq cr{filters, n_filters, out_allowed, columns, n_columns, out_set, carry};
  return compact_common(h, "hnsw_compact_carry", stage_bytes_or_0, &cr, out_new_of_old, cap_map, stats);
}

int coltt_hnsw_carry_bits_host(const uint32_t* bits, uint64_t n_words, const uint32_t* del_bits, uint64_t n_slots, uint32_t* out_bits,
                               uint64_t* out_allowed, uint64_t* out_live) {
  if (n_slots >= 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_carry_bits_host: more than 2^31-1 slots");
  if (n_words && !bits) return fail(COLTT_E_INVALID, "hnsw_carry_bits_host: NULL bits");
  carry_bits_host(bits, n_words, del_bits, n_slots, out_bits, out_allowed, out_live);
  return COLTT_OK;
}

int coltt_hnsw_carry_bits_device(const uint32_t* bits, uint64_t n_bitmaps, uint64_t n_words, const uint32_t* del_bits, uint64_t n_slots,
                                 uint32_t* out_bits, uint64_t* out_allowed, uint32_t* out_lists, const uint64_t* list_off) {
  if (n_slots >= 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_carry_bits_device: more than 2^31-1 slots");
  if (n_bitmaps && n_words && !bits) return fail(COLTT_E_INVALID, "hnsw_carry_bits_device: NULL bits");
  if (out_lists && !list_off) return fail(COLTT_E_INVALID, "hnsw_carry_bits_device: lists without their offsets");
  if (n_bitmaps == 0) return COLTT_OK;
  const size_t words = (size_t)((n_slots + 31) / 32);
  std::vector<uint32_t> rank(words, 0u), oon;
  uint64_t live = 0;
  for (size_t w = 0; w < words; w++) {
    rank[w] = (uint32_t)live;
    for (uint32_t b = carry_live_word_host(del_bits, w, words, n_slots); b; b &= b - 1) oon.push_back((uint32_t)(w * 32 + __builtin_ctz(b)));
    live = oon.size();
  }
  if (live == 0) {   // nothing survives: nothing is launched
    if (out_allowed) std::fill(out_allowed, out_allowed + n_bitmaps, 0ull);
    return COLTT_OK;
  }
  const uint32_t nw_new = (uint32_t)((live + 31) / 32), n_wg = carry_n_wg(live);
  const size_t stride = carry_stride(live);
  if (n_bitmaps * (uint64_t)n_wg > 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_carry_bits_device: %llu bitmaps over %llu slots exceed one launch", (unsigned long long)n_bitmaps, (unsigned long long)live);
  const size_t src_words = (size_t)std::min<uint64_t>(n_words, words);   // (no slot lies past `words`)
  COLTT_DEVICE(-1);
  DevBuf d_src, d_del, d_rank, d_oon, d_maps, d_out, d_cnt, d_loff, d_lists;
  std::vector<CarryMap> maps(n_bitmaps);
  std::vector<uint64_t> loff(n_bitmaps);
  uint64_t total = 0;   // the lists: sized by what each source allows at most, as the compaction sizes them by the old counts
  for (uint64_t p = 0; p < n_bitmaps; p++) {
    uint64_t c = 0;
    for (size_t w = 0; w < src_words; w++) c += (uint64_t)__builtin_popcount(bits[p * n_words + w]);
    loff[p] = total; total += (std::min<uint64_t>(c, live) + 63) & ~63ull;
  }
  if (src_words) COLTT_TRY(d_src.reserve(n_bitmaps * src_words * 4));
  if (del_bits) COLTT_TRY(d_del.reserve(words * 4));
  COLTT_TRY(d_rank.reserve(words * 4));
  COLTT_TRY(d_oon.reserve(live * 4));
  COLTT_TRY(d_maps.reserve(n_bitmaps * sizeof(CarryMap)));
  COLTT_TRY(d_out.reserve(n_bitmaps * stride * 4));
  COLTT_TRY(d_cnt.reserve(n_bitmaps * (size_t)n_wg * 4));
  if (out_lists && total) { COLTT_TRY(d_loff.reserve(n_bitmaps * 8)); COLTT_TRY(d_lists.reserve((size_t)total * 4)); }
  for (uint64_t p = 0; p < n_bitmaps; p++) {
    maps[p] = CarryMap{d_src.as<uint32_t>() + p * src_words, d_out.as<uint32_t>() + p * stride, (uint32_t)src_words, 0u};
    if (src_words) COLTT_HIP(hipMemcpy(d_src.as<uint32_t>() + p * src_words, bits + p * n_words, src_words * 4, hipMemcpyHostToDevice));
  }
  if (del_bits) COLTT_HIP(hipMemcpy(d_del.p, del_bits, words * 4, hipMemcpyHostToDevice));
  COLTT_HIP(hipMemcpy(d_rank.p, rank.data(), words * 4, hipMemcpyHostToDevice));
  COLTT_HIP(hipMemcpy(d_oon.p, oon.data(), live * 4, hipMemcpyHostToDevice));
  COLTT_HIP(hipMemcpy(d_maps.p, maps.data(), n_bitmaps * sizeof(CarryMap), hipMemcpyHostToDevice));
  launch_carry(nullptr, d_maps.as<CarryMap>(), (uint32_t)n_bitmaps, d_del.as<uint32_t>(), (uint32_t)n_slots, d_rank.as<uint32_t>(), d_oon.as<uint32_t>(),
               (uint32_t)live, d_cnt.as<uint32_t>());
  COLTT_HIP(hipGetLastError());
  if (out_lists && total) {
    COLTT_HIP(hipMemcpy(d_loff.p, loff.data(), n_bitmaps * 8, hipMemcpyHostToDevice));
    filter_compact_kernel<<<(uint32_t)(n_bitmaps * n_wg), FEX_THREADS, 0, nullptr>>>(d_out.as<uint32_t>(), stride, nw_new, n_wg, d_cnt.as<uint32_t>(),
                                                                                     d_loff.as<uint64_t>(), d_lists.as<uint32_t>());
    COLTT_HIP(hipGetLastError());
  }
  COLTT_HIP(hipDeviceSynchronize());
  std::vector<uint32_t> cnt(n_bitmaps * (size_t)n_wg);
  COLTT_HIP(hipMemcpy(cnt.data(), d_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost));
  if (out_bits) COLTT_HIP(hipMemcpy2D(out_bits, (size_t)nw_new * 4, d_out.p, stride * 4, (size_t)nw_new * 4, n_bitmaps, hipMemcpyDeviceToHost));
  for (uint64_t p = 0; p < n_bitmaps; p++) {
    uint64_t a = 0;
    for (uint32_t t = 0; t < n_wg; t++) a += cnt[p * n_wg + t];
    if (out_allowed) out_allowed[p] = a;
    if (out_lists && a) COLTT_HIP(hipMemcpy(out_lists + list_off[p], d_lists.as<uint32_t>() + loff[p], (size_t)a * 4, hipMemcpyDeviceToHost));
  }
  return COLTT_OK;
}

int coltt_hnsw_export(coltt_handle_t h, uint64_t* n_slots, uint64_t* n_rows, uint64_t* n_edges, uint64_t* ids,
                      int32_t* levels, uint8_t* deleted, int64_t* row_offsets, int32_t* nbr, float* nbr_dist,
                      int32_t* entry_slot) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_export: unknown handle");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  const uint64_t n = x->n;
  const uint32_t W0 = (uint32_t)x->cfg.m_max0, WU = (uint32_t)x->cfg.m_max;
  const bool filling = ids || levels || deleted || row_offsets || nbr || nbr_dist;
  if (filling) {
    // the caller sized its arrays from an earlier call; an Insert in between must not turn into a write past their end
    if (!n_slots || !n_rows || !n_edges) return fail(COLTT_E_INVALID, "hnsw_export: array capacities (n_slots, n_rows, n_edges) are required when arrays are passed");
    uint64_t need_rows = 0;
    for (uint64_t i = 0; i < n; i++) need_rows += (uint64_t)x->h_levels[i] + 1;
    const bool slots_short = (ids || levels || deleted) && *n_slots < n;
    const bool rows_short = row_offsets && *n_rows < need_rows;
    if (slots_short || rows_short) {
      const uint64_t cs = *n_slots, cr = *n_rows;
      *n_slots = n; *n_rows = need_rows;
      return fail(COLTT_E_INVALID, "hnsw_export: the index grew past the caller's arrays (%llu slots / %llu rows offered, %llu / %llu needed)",
                  (unsigned long long)cs, (unsigned long long)cr, (unsigned long long)n, (unsigned long long)need_rows);
    }
  }
  const uint64_t cap_edges = (filling && n_edges) ? *n_edges : 0;
  std::vector<uint32_t> a0((size_t)n * W0), aU((size_t)x->n_upper * WU);
  std::vector<float> d0, dU;
  if (n) COLTT_HIP(hipMemcpy(a0.data(), x->adj0.p, a0.size() * 4, hipMemcpyDeviceToHost));
  if (x->n_upper) COLTT_HIP(hipMemcpy(aU.data(), x->adjU.p, aU.size() * 4, hipMemcpyDeviceToHost));
  if (nbr_dist) {
    d0.resize(a0.size()); dU.resize(aU.size());
    if (n) COLTT_HIP(hipMemcpy(d0.data(), x->adj0_d.p, d0.size() * 4, hipMemcpyDeviceToHost));
    if (x->n_upper) COLTT_HIP(hipMemcpy(dU.data(), x->adjU_d.p, dU.size() * 4, hipMemcpyDeviceToHost));
  }
  uint64_t rows = 0, edges = 0;
  if (row_offsets) row_offsets[0] = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (ids) ids[i] = x->dense ? x->dense_base + i : x->h_ids[i];
    if (levels) levels[i] = x->h_levels[i];
    if (deleted) deleted[i] = (x->h_del[i >> 5] >> (i & 31)) & 1u;
    for (int l = 0; l <= x->h_levels[i]; l++) {
      uint32_t W = l == 0 ? W0 : WU;
      const uint32_t* r = l == 0 ? &a0[(size_t)i * W0] : &aU[((size_t)x->h_upper_off[i] + l - 1) * WU];
      const float* dr = nbr_dist ? (l == 0 ? &d0[(size_t)i * W0] : &dU[((size_t)x->h_upper_off[i] + l - 1) * WU]) : nullptr;
      for (uint32_t j = 0; j < W && r[j] != NBR_NONE; j++) {
        if (edges < cap_edges) {
          if (nbr) nbr[edges] = (int32_t)r[j];
          if (nbr_dist) nbr_dist[edges] = dr[j];
        }
        edges++;
      }
      rows++;
      if (row_offsets) row_offsets[rows] = (int64_t)edges;
    }
  }
  if (n_slots) *n_slots = n;
  if (n_rows) *n_rows = rows;
  if (n_edges) *n_edges = edges;
  if (entry_slot) *entry_slot = x->entry;
  if ((nbr || nbr_dist) && edges > cap_edges)
    return fail(COLTT_E_INVALID, "hnsw_export: the index grew past the caller's edge arrays (%llu offered, %llu needed)",
                (unsigned long long)cap_edges, (unsigned long long)edges);
  return COLTT_OK;
}

int coltt_hnsw_export_raw(coltt_handle_t h, uint64_t* n_slots, uint64_t* n_upper_rows, int32_t* entry_slot,
                          int32_t* entry_level, uint32_t* adj0, uint32_t* upper_off, uint32_t* adjU) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_export_raw: unknown handle");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  if (n_slots) *n_slots = x->n;
  if (n_upper_rows) *n_upper_rows = x->n_upper;
  if (entry_slot) *entry_slot = x->entry;
  if (entry_level) *entry_level = x->entry_level;
  if (adj0 && x->n) COLTT_HIP(hipMemcpy(adj0, x->adj0.p, (size_t)x->n * x->cfg.m_max0 * 4, hipMemcpyDeviceToHost));
  if (upper_off && x->n) COLTT_HIP(hipMemcpy(upper_off, x->upper_off.p, (size_t)x->n * 4, hipMemcpyDeviceToHost));
  if (adjU && x->n_upper) COLTT_HIP(hipMemcpy(adjU, x->adjU.p, (size_t)x->n_upper * x->cfg.m_max * 4, hipMemcpyDeviceToHost));
  return COLTT_OK;
}

int coltt_hnsw_fetch_rows(coltt_handle_t h, uint64_t first_slot, uint64_t n, void* out_rows) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_fetch_rows: unknown handle");
  if (n == 0) return COLTT_OK;
  ReadLock g(x->rw);
  if (!out_rows || first_slot + n > x->n) return fail(COLTT_E_INVALID, "hnsw_fetch_rows: range outside [0,%llu)", (unsigned long long)x->n);
  COLTT_DEVICE(x->device);
  const size_t rb = (size_t)x->dim * quant_bytes(x->quant);
  if (x->r8) {   // line-transposed rows: natural element order is restored on the device, block by block
    DevBuf d_nat;
    const uint64_t blk = std::max<uint64_t>(1, (256ull << 20) / rb);
    COLTT_TRY(d_nat.reserve(std::min<uint64_t>(blk, n) * rb));
    for (uint64_t b = 0; b < n; b += blk) {
      const uint64_t m = std::min<uint64_t>(blk, n - b);
      if (x->quant == COLTT_Q_NONE) rows_natural_kernel<Q_NONE><<<ceil_div(m * x->dim, 256), 256, 0, nullptr>>>(x->rows.as<uint8_t>(), x->stride, first_slot + b, m, (int)x->dim, d_nat.as<uint8_t>());
      else rows_natural_kernel<Q_F16><<<ceil_div(m * x->dim, 256), 256, 0, nullptr>>>(x->rows.as<uint8_t>(), x->stride, first_slot + b, m, (int)x->dim, d_nat.as<uint8_t>());
      COLTT_HIP(hipGetLastError());
      COLTT_HIP(hipMemcpy(static_cast<uint8_t*>(out_rows) + b * rb, d_nat.p, m * rb, hipMemcpyDeviceToHost));
    }
    return COLTT_OK;
  }
  COLTT_HIP(hipMemcpy2D(out_rows, rb, x->rows.as<uint8_t>() + first_slot * x->stride, x->stride, rb, n, hipMemcpyDeviceToHost));
  return COLTT_OK;
}

int coltt_hnsw_get(coltt_handle_t h, uint64_t id, void* out_row, int32_t* out_level) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_get: unknown handle");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  uint64_t slot;
  if (x->dense) {
    if (id < x->dense_base || id >= x->dense_base + x->n) return fail(COLTT_E_NOT_FOUND, "Item not found");
    slot = id - x->dense_base;
    if ((x->h_del[slot >> 5] >> (slot & 31)) & 1u) return fail(COLTT_E_NOT_FOUND, "Item not found");
  } else {
    auto it = x->id2slot.find(id);
    if (it == x->id2slot.end()) return fail(COLTT_E_NOT_FOUND, "Item not found");  // ItemNotFoundError (hnsw.go:177,188)
    slot = it->second;
  }
  if (out_row && x->r8) {   // one line-transposed row: copied as stored, natural element order restored on the host
    std::vector<uint8_t> raw(x->stride);
    COLTT_HIP(hipMemcpy(raw.data(), x->rows.as<uint8_t>() + slot * x->stride, x->stride, hipMemcpyDeviceToHost));
    if (x->quant == COLTT_Q_NONE) for (uint32_t e = 0; e < x->dim; e++) static_cast<uint32_t*>(out_row)[e] = reinterpret_cast<const uint32_t*>(raw.data())[r8_index<Q_NONE>((int)e)];
    else for (uint32_t e = 0; e < x->dim; e++) static_cast<uint16_t*>(out_row)[e] = reinterpret_cast<const uint16_t*>(raw.data())[r8_index<Q_F16>((int)e)];
  } else if (out_row) COLTT_HIP(hipMemcpy(out_row, x->rows.as<uint8_t>() + slot * x->stride, (size_t)x->dim * quant_bytes(x->quant), hipMemcpyDeviceToHost));
  if (out_level) *out_level = x->h_levels[slot];
  return COLTT_OK;
}

int coltt_hnsw_reserve(coltt_handle_t h, uint64_t n_slots, uint64_t n_upper_rows) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_reserve: unknown handle");
  if (n_slots >= 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_reserve: more than 2^31-1 slots");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  // upper rows: a vertex of level L owns L of them; the level draw floor(-ln(u) / ln(M)) averages 1 / (M - 1) per vertex
  if (n_upper_rows == 0) n_upper_rows = n_slots / (uint64_t)std::max(2, x->cfg.m - 1) + n_slots / 64 + 1024;
  return x->reserve(n_slots, n_upper_rows);
}

// ---- product-quantised HNSW (hnsw_pq.hpp; the reference's call shape: playground/hnswpq_verification.go:69-105) -------------------
int coltt_hnsw_pq_attach(coltt_handle_t h, coltt_handle_t pq) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_attach: unknown index handle");
  WriteLock g(x->rw);
  COLTT_DEVICE(x->device);
  x->pq_nbr_stale.store(true);
  if (x->quant == COLTT_Q_F8) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_attach: \"f8\" rows hold eight distinct values — nothing to quantise");
  PqShape sh;
  COLTT_TRY(pq_snapshot(pq, &sh, &x->pq_stage, x->stream));   // staged first: the index is untouched unless everything checks out
  if (sh.dim != x->dim) return fail(COLTT_E_INVALID, "hnsw_pq_attach: the quantiser is for dim %u, the index holds dim %u", sh.dim, x->dim);
  if (sh.metric == COLTT_PQ_DOT) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_attach: dotProductDistance tables are negative — the walk orders distances by their bits (squared L2, or 1 - dot on a cosine index)");
  if (sh.metric == COLTT_PQ_COSINE && x->metric != COLTT_COSINE) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_attach: cosineDistance tables need a cosine index (normalised rows: every table entry is >= 0)");
  if (x->dim % 4) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_attach: dim %u is not a multiple of 4 (the re-rank reads the prepared query rows with 16-byte loads)", x->dim);
  if (sh.metric == COLTT_PQ_COSINE) {
    // 1 - dot(q_j, centroid) must never be negative (the walk orders table distances by their bits): the index hands the walk normalised queries, so
    // ||centroid|| <= 1 is enough — true of a quantiser trained on the index's own (normalised) rows, not of one trained on raw vectors
    COLTT_TRY(x->w_misc.reserve(256));
    float nmax = 0.f;
    COLTT_TRY(pq_centroid_norm_max(x->stream, x->pq_stage.as<float>(), sh, x->w_misc.as<uint32_t>(), &nmax));
    if (!(nmax <= 1.0f + 1e-4f)) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_attach: cosineDistance quantiser with a centroid of squared norm %g > 1 — its tables can be negative (train it on the index's normalised rows)", (double)nmax);
  }
  const uint32_t row = (sh.m + 15u) & ~15u;
  if (row > 128) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_attach: %u sub-vectors — a query's table (%u KiB) must fit the CU's LDS beside the result set (<= 128)", sh.m, row / 2);
  const size_t bytes = (size_t)sh.m * sh.C * sh.dsub * 4;
  COLTT_TRY(x->pq_cb.reserve(bytes));
  COLTT_HIP(hipMemcpyAsync(x->pq_cb.p, x->pq_stage.p, bytes, hipMemcpyDeviceToDevice, x->stream));
  COLTT_HIP(hipStreamSynchronize(x->stream));
  x->pq_shape = sh; x->pq_row = row; x->pq_done = 0; x->pq_on = true;
  if (x->pq_codes.p) COLTT_HIP(hipMemsetAsync(x->pq_codes.p, 0, x->pq_codes.cap, x->stream));
  int rc = sync_pq(x.get());
  if (rc == COLTT_OK && x->vis_stride != 0) rc = ensure_visg(x.get(), policy());   // (exclusive lock: no traversal holds a region) 2048 -> 3072 regions for the table walk
  if (rc != COLTT_OK) x->pq_on = false;
  return rc;
}

int coltt_hnsw_pq_info(coltt_handle_t h, uint32_t* out_m, uint32_t* out_c, int32_t* out_metric, uint64_t* out_coded) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_info: unknown handle");
  ReadLock g(x->rw);
  if (out_m) *out_m = x->pq_on ? x->pq_shape.m : 0;
  if (out_c) *out_c = x->pq_on ? x->pq_shape.C : 0;
  if (out_metric) *out_metric = x->pq_on ? x->pq_shape.metric : -1;
  if (out_coded) *out_coded = x->pq_on ? x->pq_done : 0;
  return COLTT_OK;
}

int coltt_hnsw_pq_fetch_codes(coltt_handle_t h, uint64_t first_slot, uint64_t n, uint8_t* out_codes) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_fetch_codes: unknown handle");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  if (!x->pq_on) return fail(COLTT_E_INVALID, "hnsw_pq_fetch_codes: no quantiser attached");
  if (first_slot + n > x->pq_done) return fail(COLTT_E_INVALID, "hnsw_pq_fetch_codes: slots [%llu,%llu) outside the %llu coded ones", (unsigned long long)first_slot, (unsigned long long)(first_slot + n), (unsigned long long)x->pq_done);
  if (n == 0) return COLTT_OK;
  if (!out_codes) return fail(COLTT_E_INVALID, "hnsw_pq_fetch_codes: NULL out");
  COLTT_HIP(hipMemcpy2D(out_codes, x->pq_shape.m, x->pq_codes.as<uint8_t>() + first_slot * x->pq_row, x->pq_row, x->pq_shape.m, n, hipMemcpyDeviceToHost));
  return COLTT_OK;
}

namespace {
// 0 = none (no quantiser, COLTT_PQ_NBR=0, never built, not affordable), 1 = current, 2 = built once and stale.  Caller holds pq_nbr_mu.
int pq_nbr_state(const Hnsw* x) {
  if (!policy().pq_nbr || !x->pq_on) return 0;
  if (x->pq_nbr_stale.load()) return x->pq_nbr_built ? 2 : 0;
  return x->pq_nbr_ok ? 1 : 0;
}
}  // namespace

int coltt_hnsw_pq_nbr_stats(coltt_handle_t h, uint64_t* out_builds, uint64_t* out_patches, uint64_t* out_patched_rows, int32_t* out_state) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_nbr_stats: unknown handle");
  ReadLock g(x->rw);
  std::lock_guard<std::mutex> gn(x->pq_nbr_mu);
  if (out_builds) *out_builds = x->pq_nbr_builds.load();
  if (out_patches) *out_patches = x->pq_nbr_patches.load();
  if (out_patched_rows) *out_patched_rows = x->pq_nbr_patched_rows.load();
  if (out_state) *out_state = pq_nbr_state(x.get());
  return COLTT_OK;
}

int coltt_hnsw_pq_fetch_nbr(coltt_handle_t h, uint64_t first_slot, uint64_t n, uint8_t* out_blocks) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_fetch_nbr: unknown handle");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  std::lock_guard<std::mutex> gn(x->pq_nbr_mu);   // (a search that finds the blocks stale rebuilds them under this)
  const int st = pq_nbr_state(x.get());
  if (st != 1) return fail(COLTT_E_UNSUPPORTED, "hnsw_pq_fetch_nbr: the neighbourhood blocks are %s", st == 2 ? "stale (the next product-quantised walk above ef 128 rebuilds them)" : "not kept");
  if (first_slot > x->n || n > x->n - first_slot) return fail(COLTT_E_INVALID, "hnsw_pq_fetch_nbr: slots [%llu,%llu) outside [0,%llu)", (unsigned long long)first_slot, (unsigned long long)(first_slot + n), (unsigned long long)x->n);
  if (n == 0) return COLTT_OK;
  if (!out_blocks) return fail(COLTT_E_INVALID, "hnsw_pq_fetch_nbr: NULL out");
  const size_t blk = (size_t)x->cfg.m_max0 * x->pq_row;
  COLTT_HIP(hipMemcpy(out_blocks, x->pq_nbr.as<uint8_t>() + first_slot * blk, n * blk, hipMemcpyDeviceToHost));
  return COLTT_OK;
}

int coltt_hnsw_pq_search(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, uint32_t ef_override, uint32_t rerank,
                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_search: unknown handle");
  if (nq && (!queries || !out_ids || !out_scores || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_pq_search: NULL buffer");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return pq_search_common(x.get(), ctx.c, queries, false, nq, k, ef_override, rerank, out_ids, out_scores, out_counts, stats, out_n_exact);
}
int coltt_hnsw_pq_search_device(coltt_handle_t h, const float* d_queries, size_t nq, uint32_t k, uint32_t ef_override, uint32_t rerank,
                                uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_search_device: unknown handle");
  if (nq && (!d_queries || !d_out_ids || !d_out_scores || !d_out_counts)) return fail(COLTT_E_INVALID, "hnsw_pq_search_device: NULL buffer");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return pq_search_common(x.get(), ctx.c, d_queries, true, nq, k, ef_override, rerank, d_out_ids, d_out_scores, d_out_counts, stats, out_n_exact);
}

int coltt_hnsw_rows8_searches(coltt_handle_t h, uint64_t* out_launches, int32_t* out_has_copy) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_rows8_searches: unknown handle");
  ReadLock g(x->rw);
  if (out_launches) *out_launches = x->ev8_launches.load();
  if (out_has_copy) *out_has_copy = x->r8 ? 1 : 0;
  return COLTT_OK;
}

int coltt_hnsw_visited_stats(coltt_handle_t h, int32_t* out_kind, uint32_t* out_waves_per_cu, uint32_t* out_grid, uint64_t* out_launches16, uint64_t* out_stash_max, uint64_t* out_visited_max) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_visited_stats: unknown handle");
  ReadLock g(x->rw);
  if (out_kind) *out_kind = x->last_vis_kind.load();
  if (out_waves_per_cu) *out_waves_per_cu = x->last_per_cu.load();
  if (out_grid) *out_grid = x->last_grid.load();
  if (out_launches16) *out_launches16 = x->v16_launches.load();
  if (out_stash_max) *out_stash_max = x->last_stash_max.load();
  if (out_visited_max) *out_visited_max = x->last_visited_max.load();
  return COLTT_OK;
}

int coltt_hnsw_search_plan_host(const coltt_hnsw_plan_facts* facts, size_t nq, uint32_t k, uint32_t ef_override, int force, coltt_hnsw_search_plan* out) {
  if (!facts || !out) return fail(COLTT_E_INVALID, "hnsw_search_plan_host: NULL facts or out");
  if (nq == 0 || ef_override == 0) return fail(COLTT_E_INVALID, "hnsw_search_plan_host: nq and ef_override must be >= 1 (the index's default ef is not among the facts)");
  SearchPlan sp;
  const int rc = plan_search(*facts, policy(), nq, k, ef_override, force, sp);
  *out = rc == COLTT_OK ? sp : SearchPlan{};
  return rc;
}

int coltt_hnsw_search_plan_facts(coltt_handle_t h, coltt_hnsw_plan_facts* out_facts) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_search_plan_facts: unknown handle");
  if (!out_facts) return fail(COLTT_E_INVALID, "hnsw_search_plan_facts: NULL out");
  ReadLock g(x->rw);
  *out_facts = plan_facts(x.get());
  return COLTT_OK;
}

int coltt_last_kernel_ms(coltt_handle_t h, float* out_ms) {
  if (!out_ms) return fail(COLTT_E_INVALID, "last_kernel_ms: NULL out");
  if (auto x = lookup<Hnsw>(h)) { *out_ms = x->last_ms.load(); return COLTT_OK; }
  return coltt_last_kernel_ms_flat(h, out_ms);
}

}  // extern "C"

// ---- Filtered search: an allow-list of ids against one index (coltt_hnsw_filter_*, coltt_hnsw_search_filtered) ----------------------
// An extension the reference does not have (its Core.HybridSearch post-filters an unfiltered search): definitions in include/coltt_gpu.h.
namespace {

// id -> live slot, as coltt_hnsw_filter_create maps it (the caller holds the index's lock); false: unknown or removed
inline bool live_slot_of(const Hnsw* x, uint64_t id, uint32_t& s) {
  if (x->dense) {
    if (id < x->dense_base || id - x->dense_base >= x->n) return false;
    s = (uint32_t)(id - x->dense_base);
    return !(x->h_del.size() > (s >> 5) && ((x->h_del[s >> 5] >> (s & 31)) & 1u));
  }
  auto it = x->id2slot.find(id);
  if (it == x->id2slot.end()) return false;
  s = it->second;
  return true;
}


// coltt_hnsw_filter_eval / _eval_batch (definitions: include/coltt_gpu.h, "Filter expressions"; kernels: filter_expr.hpp).  n_out programmes
// over one leaf table under one index state: one upload (leaf table, programme offsets, programmes), the evaluate launch, the counts back
// (they size the lists), the list offsets up, the compact launch.  The outputs' bitmaps and lists are slices of one slab each.
// With predicates (coltt_hnsw_filter_eval_attr / _eval_attr_batch; attr_filter.hpp) the predicate table rides in the same upload and the
// evaluate launch is attr_filter_eval_kernel; without any, the launch is filter_eval_kernel as before.
int filter_eval_common(coltt_handle_t h, const char* who, const int32_t* progs, const uint64_t* prog_off, size_t n_out,
                       const coltt_handle_t* leaves, size_t n_leaves, const coltt_attr_pred* preds, size_t n_preds,
                       uint64_t* out_allowed, coltt_handle_t* out) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "%s: unknown index handle", who);
  if (n_out == 0) return COLTT_OK;
  if (!out) return fail(COLTT_E_INVALID, "%s: out is NULL", who);
  if (!prog_off) return fail(COLTT_E_INVALID, "%s: NULL programme offsets", who);
  if (n_leaves && !leaves) return fail(COLTT_E_INVALID, "%s: NULL leaves", who);
  if (n_preds && !preds) return fail(COLTT_E_INVALID, "%s: NULL preds", who);
  uint64_t total = 0;
  for (size_t i = 0; i < n_out; i++) {   // every programme is checked before anything is created
    if (prog_off[i + 1] < prog_off[i]) return fail(COLTT_E_INVALID, "%s: programme %zu: its offsets descend", who, i);
    const uint64_t len = prog_off[i + 1] - prog_off[i];
    const int rc = coltt_hnsw_filter_prog_check_host(progs ? progs + prog_off[i] : nullptr, (size_t)len, n_leaves + n_preds, nullptr);
    if (rc != COLTT_OK) {
      const std::string why = coltt_last_error();
      return fail(rc, "%s: programme %zu: %s", who, i, why.c_str());
    }
    total += len;
  }
  ReadLock g(x->rw);
  std::unordered_map<coltt_handle_t, std::shared_ptr<HnswFilter>> held;   // each distinct leaf, until the call returns (a concurrent destroy only unregisters it)
  std::vector<HnswFilter*> lf(n_leaves);
  for (size_t i = 0; i < n_leaves; i++) {
    auto it = held.find(leaves[i]);
    if (it == held.end()) {
      auto f = lookup<HnswFilter>(leaves[i]);
      if (!f) return fail(COLTT_E_NOT_FOUND, "%s: unknown filter handle at leaf %zu", who, i);
      if (f->index != h) return fail(COLTT_E_INVALID, "%s: the filter at leaf %zu was built for another index", who, i);
      if (f->gen != x->gen) return fail(COLTT_E_INVALID, "%s: the filter at leaf %zu is stale (the index was loaded since it was built)", who, i);
      it = held.emplace(leaves[i], std::move(f)).first;
    }
    lf[i] = it->second.get();
  }
  // each distinct column: held, and locked shared until the call returns (the call sees it wholly before or wholly after a concurrent attr_set)
  std::unordered_map<coltt_handle_t, std::shared_ptr<HnswAttr>> cheld;
  std::vector<ReadLock> clocks;
  std::vector<HnswAttr*> pc(n_preds);
  for (size_t i = 0; i < n_preds; i++) {
    const coltt_attr_pred& P = preds[i];
    auto it = cheld.find(P.column);
    if (it == cheld.end()) {
      auto a = lookup<HnswAttr>(P.column);
      if (!a) return fail(COLTT_E_NOT_FOUND, "%s: unknown column handle at predicate %zu", who, i);
      if (a->index != h) return fail(COLTT_E_INVALID, "%s: the column at predicate %zu belongs to another index", who, i);
      clocks.emplace_back(a->rw);
      if (a->gen != x->gen) return fail(COLTT_E_INVALID, "%s: the column at predicate %zu is stale (the index was renumbered since it was created)", who, i);
      it = cheld.emplace(P.column, std::move(a)).first;
    }
    pc[i] = it->second.get();
    if (P.op < COLTT_CMP_EQ || P.op > COLTT_CMP_SET) return fail(COLTT_E_INVALID, "%s: unknown op %d at predicate %zu", who, (int)P.op, i);
    if (P.reserved != 0) return fail(COLTT_E_INVALID, "%s: reserved != 0 at predicate %zu", who, i);
    if (pc[i]->type == COLTT_ATTR_F64 && P.op != COLTT_CMP_SET && P.value.f64 != P.value.f64)
      return fail(COLTT_E_INVALID, "%s: a NaN operand at predicate %zu", who, i);
  }
  COLTT_DEVICE(x->device);
  const uint32_t n_slots = (uint32_t)x->n, n_words = (n_slots + 31) / 32, n_wg = ceil_div(n_words, FEX_TILE_WORDS);
  if ((uint64_t)n_out * std::max(1u, n_wg) > 0x7fffffffull || total > 0xffffffffull)
    return fail(COLTT_E_UNSUPPORTED, "%s: %zu programmes over %u slots exceed one launch", who, n_out, n_slots);
  std::vector<std::shared_ptr<HnswFilter>> res(n_out);
  for (auto& f : res) {
    f = std::make_shared<HnswFilter>();
    f->device = x->device; f->index = h; f->gen = x->gen; f->slots = n_slots;
  }
  if (n_words) {
    CtxLease<HCtx> ctx(x->pool);
    if (!ctx.c) return COLTT_E_DEVICE;
    HCtx* c = ctx.c;
    auto slab = std::make_shared<FilterSlab>();
    slab->device = x->device;
    const size_t stride = ((size_t)n_words + 63) & ~(size_t)63;   // words per output bitmap: 256-byte slices
    COLTT_TRY(slab->bits.reserve(n_out * stride * 4));
    // one upload: [leaf table][predicate table][list offsets, filled later][programme offsets][programmes]
    const size_t o_pred = n_leaves * sizeof(FexLeaf), o_loff = o_pred + n_preds * sizeof(AttrPredDev), o_poff = o_loff + n_out * 8, o_prog = o_poff + (n_out + 1) * 4, bytes = o_prog + (size_t)total * 4;
    COLTT_TRY(c->h_in.reserve(bytes));
    COLTT_TRY(c->w_fdesc.reserve(bytes));
    COLTT_TRY(c->w_scnt.reserve(n_out * (size_t)n_wg * 4));
    COLTT_TRY(c->h_out.reserve(n_out * (size_t)n_wg * 4));
    uint8_t* hb = static_cast<uint8_t*>(c->h_in.p);
    FexLeaf* h_leaf = reinterpret_cast<FexLeaf*>(hb);
    uint64_t* h_loff = reinterpret_cast<uint64_t*>(hb + o_loff);
    uint32_t* h_poff = reinterpret_cast<uint32_t*>(hb + o_poff);
    int32_t* h_prog = reinterpret_cast<int32_t*>(hb + o_prog);
    AttrPredDev* h_pred = reinterpret_cast<AttrPredDev*>(hb + o_pred);
    for (size_t i = 0; i < n_preds; i++) {
      uint64_t operand;
      std::memcpy(&operand, &preds[i].value, 8);
      h_pred[i] = AttrPredDev{pc[i]->vals.as<uint64_t>(), pc[i]->set.as<uint32_t>(), operand, std::min(pc[i]->slots, n_slots), preds[i].op | (pc[i]->type << 8)};
    }
    for (size_t i = 0; i < n_leaves; i++) h_leaf[i] = FexLeaf{lf[i]->bits.as<uint32_t>(), std::min((lf[i]->slots + 31) / 32, n_words), 0u};
    uint32_t at = 0;
    for (size_t i = 0; i < n_out; i++) {
      h_loff[i] = 0; h_poff[i] = at;
      const size_t len = (size_t)(prog_off[i + 1] - prog_off[i]);
      std::memcpy(h_prog + at, progs + prog_off[i], len * 4);
      at += (uint32_t)len;
    }
    h_poff[n_out] = at;
    uint8_t* db = c->w_fdesc.as<uint8_t>();
    COLTT_HIP(hipMemcpyAsync(db, hb, bytes, hipMemcpyHostToDevice, c->stream));
    const uint32_t grid = (uint32_t)(n_out * n_wg);
    if (n_preds)
      attr_filter_eval_kernel<<<grid, FEX_THREADS, 0, c->stream>>>(reinterpret_cast<const FexLeaf*>(db), (uint32_t)n_leaves, reinterpret_cast<const AttrPredDev*>(db + o_pred),
                                                                   reinterpret_cast<const uint32_t*>(db + o_poff), reinterpret_cast<const int32_t*>(db + o_prog),
                                                                   x->any_deleted ? x->del_bits.as<uint32_t>() : nullptr, n_slots, n_words, n_wg,
                                                                   slab->bits.as<uint32_t>(), stride, c->w_scnt.as<uint32_t>());
    else
      filter_eval_kernel<<<grid, FEX_THREADS, 0, c->stream>>>(reinterpret_cast<const FexLeaf*>(db), reinterpret_cast<const uint32_t*>(db + o_poff),
                                                              reinterpret_cast<const int32_t*>(db + o_prog), x->any_deleted ? x->del_bits.as<uint32_t>() : nullptr,
                                                              n_slots, n_words, n_wg, slab->bits.as<uint32_t>(), stride, c->w_scnt.as<uint32_t>());
    COLTT_HIP(hipGetLastError());
    COLTT_HIP(hipMemcpyAsync(c->h_out.p, c->w_scnt.p, n_out * (size_t)n_wg * 4, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipStreamSynchronize(c->stream));
    const uint32_t* h_cnt = static_cast<const uint32_t*>(c->h_out.p);
    uint64_t entries = 0;   // the lists: 256-byte slices of the second slab
    for (size_t i = 0; i < n_out; i++) {
      uint64_t a = 0;
      for (uint32_t t = 0; t < n_wg; t++) a += h_cnt[i * n_wg + t];
      res[i]->allowed = a;
      h_loff[i] = entries;
      entries += (a + 63) & ~63ull;
    }
    if (entries) {
      COLTT_TRY(slab->lists.reserve((size_t)entries * 4));
      COLTT_HIP(hipMemcpyAsync(db + o_loff, h_loff, n_out * 8, hipMemcpyHostToDevice, c->stream));
      filter_compact_kernel<<<grid, FEX_THREADS, 0, c->stream>>>(slab->bits.as<uint32_t>(), stride, n_words, n_wg, c->w_scnt.as<uint32_t>(),
                                                                 reinterpret_cast<const uint64_t*>(db + o_loff), slab->lists.as<uint32_t>());
      COLTT_HIP(hipGetLastError());
      COLTT_HIP(hipStreamSynchronize(c->stream));   // the outputs are read on other streams from here on
    }
    for (size_t i = 0; i < n_out; i++) {
      HnswFilter* f = res[i].get();
      f->slab = slab;
      f->bits.p = slab->bits.as<uint32_t>() + i * stride; f->bits.cap = (size_t)n_words * 4;
      if (f->allowed) { f->list.p = slab->lists.as<uint32_t>() + h_loff[i]; f->list.cap = (size_t)f->allowed * 4; }
    }
  }
  for (size_t i = 0; i < n_out; i++) {
    if (out_allowed) out_allowed[i] = res[i]->allowed;
    out[i] = Registry::get().add(res[i]);
  }
  return COLTT_OK;
}
}  // namespace

extern "C" {

int coltt_hnsw_filter_create(coltt_handle_t h, const uint64_t* ids, size_t n, uint64_t* out_allowed, coltt_handle_t* out) {
  if (!out) return fail(COLTT_E_INVALID, "hnsw_filter_create: out is NULL");
  if (n && !ids) return fail(COLTT_E_INVALID, "hnsw_filter_create: NULL ids");
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_filter_create: unknown index handle");
  ReadLock g(x->rw);
  COLTT_DEVICE(x->device);
  auto f = std::make_shared<HnswFilter>();
  f->device = x->device; f->index = h; f->gen = x->gen; f->slots = (uint32_t)x->n;
  std::vector<uint32_t> words(((size_t)x->n + 31) / 32, 0u);
  for (size_t i = 0; i < n; i++) {   // ids -> live slots; unknown / removed ids are ignored, duplicates count once
    const uint64_t id = ids[i];
    uint32_t s;
    if (x->dense) {
      if (id < x->dense_base || id - x->dense_base >= x->n) continue;
      s = (uint32_t)(id - x->dense_base);
      if (x->h_del.size() > (s >> 5) && ((x->h_del[s >> 5] >> (s & 31)) & 1u)) continue;
    } else {
      auto it = x->id2slot.find(id);
      if (it == x->id2slot.end()) continue;
      s = it->second;
    }
    words[s >> 5] |= 1u << (s & 31);
  }
  std::vector<uint32_t> list;
  for (size_t w = 0; w < words.size(); w++)
    for (uint32_t b = words[w]; b; b &= b - 1) list.push_back((uint32_t)(w * 32 + __builtin_ctz(b)));
  f->allowed = list.size();
  if (!words.empty()) {
    COLTT_TRY(f->bits.reserve(words.size() * 4));
    COLTT_HIP(hipMemcpy(f->bits.p, words.data(), words.size() * 4, hipMemcpyHostToDevice));
  }
  if (!list.empty()) {
    COLTT_TRY(f->list.reserve(list.size() * 4));
    COLTT_HIP(hipMemcpy(f->list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice));
  }
  if (out_allowed) *out_allowed = f->allowed;
  *out = Registry::get().add(f);
  return COLTT_OK;
}

int coltt_hnsw_filter_destroy(coltt_handle_t fh) {
  if (!lookup<HnswFilter>(fh)) return fail(COLTT_E_NOT_FOUND, "hnsw_filter_destroy: unknown filter handle");
  Registry::get().erase(fh);
  return COLTT_OK;
}

int coltt_hnsw_filter_prog_check_host(const int32_t* prog, size_t n_prog, size_t n_leaves, uint32_t* out_depth) {
  size_t pos = 0; const char* why = "";
  const int rc = fex_prog_check(prog, n_prog, n_leaves, out_depth, &pos, &why);
  if (rc != COLTT_OK) return fail(rc, "filter programme: %s at position %zu", why, pos);
  return COLTT_OK;
}

int coltt_hnsw_filter_eval(coltt_handle_t h, const int32_t* prog, size_t n_prog, const coltt_handle_t* leaves, size_t n_leaves,
                           uint64_t* out_allowed, coltt_handle_t* out) {
  if (!out) return fail(COLTT_E_INVALID, "hnsw_filter_eval: out is NULL");
  const uint64_t off[2] = {0, (uint64_t)n_prog};
  return filter_eval_common(h, "hnsw_filter_eval", prog, off, 1, leaves, n_leaves, nullptr, 0, out_allowed, out);
}

int coltt_hnsw_filter_eval_batch(coltt_handle_t h, const int32_t* progs, const uint64_t* prog_off, size_t n_out, const coltt_handle_t* leaves,
                                 size_t n_leaves, uint64_t* out_allowed, coltt_handle_t* out) {
  return filter_eval_common(h, "hnsw_filter_eval_batch", progs, prog_off, n_out, leaves, n_leaves, nullptr, 0, out_allowed, out);
}

int coltt_hnsw_filter_eval_attr(coltt_handle_t h, const int32_t* prog, size_t n_prog, const coltt_handle_t* leaves, size_t n_leaves,
                                const coltt_attr_pred* preds, size_t n_preds, uint64_t* out_allowed, coltt_handle_t* out) {
  if (!lookup<Hnsw>(h)) return fail(COLTT_E_NOT_FOUND, "hnsw_filter_eval_attr: unknown index handle");
  if (!out) return fail(COLTT_E_INVALID, "hnsw_filter_eval_attr: out is NULL");
  const uint64_t off[2] = {0, (uint64_t)n_prog};
  return filter_eval_common(h, "hnsw_filter_eval_attr", prog, off, 1, leaves, n_leaves, preds, n_preds, out_allowed, out);
}

int coltt_hnsw_filter_eval_attr_batch(coltt_handle_t h, const int32_t* progs, const uint64_t* prog_off, size_t n_out, const coltt_handle_t* leaves,
                                      size_t n_leaves, const coltt_attr_pred* preds, size_t n_preds, uint64_t* out_allowed, coltt_handle_t* out) {
  return filter_eval_common(h, "hnsw_filter_eval_attr_batch", progs, prog_off, n_out, leaves, n_leaves, preds, n_preds, out_allowed, out);
}

// ---- attribute columns (include/coltt_gpu.h, "Attribute columns and predicates"; kernels: attr_filter.hpp)
int coltt_hnsw_attr_create(coltt_handle_t h, int type, coltt_handle_t* out) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_create: unknown index handle");
  if (!out) return fail(COLTT_E_INVALID, "hnsw_attr_create: out is NULL");
  if (type != COLTT_ATTR_I64 && type != COLTT_ATTR_F64) return fail(COLTT_E_INVALID, "hnsw_attr_create: unknown type %d", type);
  ReadLock g(x->rw);
  auto a = std::make_shared<HnswAttr>();
  a->device = x->device; a->index = h; a->gen = x->gen; a->type = type;
  *out = Registry::get().add(a);
  return COLTT_OK;
}

int coltt_hnsw_attr_destroy(coltt_handle_t ah) {
  if (!lookup<HnswAttr>(ah)) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_destroy: unknown column handle");
  Registry::get().erase(ah);
  return COLTT_OK;
}

int coltt_hnsw_attr_info(coltt_handle_t ah, coltt_handle_t* out_index, int32_t* out_type, uint64_t* out_slots, uint64_t* out_set) {
  auto a = lookup<HnswAttr>(ah);
  if (!a) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_info: unknown column handle");
  ReadLock ga(a->rw);
  if (out_index) *out_index = a->index;
  if (out_type) *out_type = a->type;
  if (out_slots) *out_slots = a->slots;
  if (out_set) *out_set = a->n_set;
  return COLTT_OK;
}

int coltt_hnsw_attr_set(coltt_handle_t ah, const uint64_t* ids, const void* values, size_t n, uint64_t* out_applied) {
  auto a = lookup<HnswAttr>(ah);
  if (!a) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_set: unknown column handle");
  if (n && (!ids || !values)) return fail(COLTT_E_INVALID, "hnsw_attr_set: NULL ids or values");
  if (n > 0xffffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_attr_set: more than 2^32-1 values in one call");
  auto x = lookup<Hnsw>(a->index);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_set: the column's index is gone");
  const uint64_t* v = static_cast<const uint64_t*>(values);
  if (a->type == COLTT_ATTR_F64)   // the whole call, before anything is written
    for (size_t i = 0; i < n; i++)
      if (attr_is_nan(v[i])) return fail(COLTT_E_INVALID, "hnsw_attr_set: value %zu is NaN", i);
  ReadLock g(x->rw);
  WriteLock ga(a->rw);
  if (a->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_attr_set: the column is stale (the index was renumbered since it was created)");
  if (out_applied) *out_applied = 0;
  const uint64_t n_slots = x->n;
  if (n_slots == 0) return COLTT_OK;
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  HCtx* c = ctx.c;
  if (n_slots > a->cap) {   // grow to the index's capacity; the new set words are 0
    const uint64_t ncap = std::max<uint64_t>(x->cap, n_slots), ow = (a->cap + 31) / 32, nw = (ncap + 31) / 32;
    COLTT_TRY(a->vals.reserve(ncap * 8, true, c->stream));
    COLTT_TRY(a->set.reserve(nw * 4, true, c->stream));
    COLTT_HIP(hipMemsetAsync(a->set.as<uint32_t>() + ow, 0, (nw - ow) * 4, c->stream));
    a->h_set.resize(nw, 0u);
    a->cap = ncap;
  }
  // ids -> live slots, last value wins: walk the call backwards and keep the first sight of every slot
  const size_t o_val = (n * 4 + 7) & ~(size_t)7;
  COLTT_TRY(c->h_in.reserve(o_val + n * 8));
  COLTT_TRY(c->w_fdesc.reserve(o_val + n * 8));
  uint8_t* hb = static_cast<uint8_t*>(c->h_in.p);
  uint32_t* h_slot = reinterpret_cast<uint32_t*>(hb);
  uint64_t* h_val = reinterpret_cast<uint64_t*>(hb + o_val);
  std::vector<uint32_t> seen((n_slots + 31) / 32, 0u);
  size_t m = 0; uint64_t fresh = 0;
  uint32_t w_lo = 0xffffffffu, w_hi = 0;
  for (size_t i = n; i-- > 0;) {
    uint32_t s;
    if (!live_slot_of(x.get(), ids[i], s)) continue;
    const uint32_t bit = 1u << (s & 31);
    if (seen[s >> 5] & bit) continue;
    seen[s >> 5] |= bit;
    h_slot[m] = s; h_val[m] = v[i]; m++;
    if (!(a->h_set[s >> 5] & bit)) { a->h_set[s >> 5] |= bit; fresh++; w_lo = std::min(w_lo, s >> 5); w_hi = std::max(w_hi, s >> 5); }
  }
  if (m) {
    uint8_t* db = c->w_fdesc.as<uint8_t>();
    COLTT_HIP(hipMemcpyAsync(db, hb, o_val + m * 8, hipMemcpyHostToDevice, c->stream));
    attr_scatter_kernel<<<ceil_div(m, 256), 256, 0, c->stream>>>(reinterpret_cast<const uint32_t*>(db), reinterpret_cast<const uint64_t*>(db + o_val), m,
                                                                 a->vals.as<uint64_t>());
    COLTT_HIP(hipGetLastError());
    if (fresh) COLTT_HIP(hipMemcpyAsync(a->set.as<uint32_t>() + w_lo, a->h_set.data() + w_lo, (size_t)(w_hi - w_lo + 1) * 4, hipMemcpyHostToDevice, c->stream));
  }
  COLTT_HIP(hipStreamSynchronize(c->stream));
  a->slots = (uint32_t)n_slots;
  a->n_set += fresh;
  if (out_applied) *out_applied = m;
  return COLTT_OK;
}

int coltt_hnsw_attr_get(coltt_handle_t ah, const uint64_t* ids, size_t n, void* out_values, uint8_t* out_set) {
  auto a = lookup<HnswAttr>(ah);
  if (!a) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_get: unknown column handle");
  if (n && !ids) return fail(COLTT_E_INVALID, "hnsw_attr_get: NULL ids");
  if (n > 0xffffffffull) return fail(COLTT_E_UNSUPPORTED, "hnsw_attr_get: more than 2^32-1 ids in one call");
  auto x = lookup<Hnsw>(a->index);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_attr_get: the column's index is gone");
  ReadLock g(x->rw);
  ReadLock ga(a->rw);
  if (a->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_attr_get: the column is stale (the index was renumbered since it was created)");
  if (n == 0) return COLTT_OK;
  if (a->slots == 0) {   // nothing was ever set
    if (out_values) std::memset(out_values, 0, n * 8);
    if (out_set) std::memset(out_set, 0, n);
    return COLTT_OK;
  }
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  HCtx* c = ctx.c;
  // up: [slots]; down: [values][flags]
  COLTT_TRY(c->h_in.reserve(n * 4));
  COLTT_TRY(c->h_out.reserve(n * 9));
  COLTT_TRY(c->w_fdesc.reserve(n * 4));
  COLTT_TRY(c->w_out_ids.reserve(n * 9));
  uint32_t* h_slot = static_cast<uint32_t*>(c->h_in.p);
  for (size_t i = 0; i < n; i++)
    if (!live_slot_of(x.get(), ids[i], h_slot[i])) h_slot[i] = 0xffffffffu;
  COLTT_HIP(hipMemcpyAsync(c->w_fdesc.p, h_slot, n * 4, hipMemcpyHostToDevice, c->stream));
  uint64_t* d_val = c->w_out_ids.as<uint64_t>();
  uint8_t* d_flag = reinterpret_cast<uint8_t*>(d_val + n);
  attr_gather_kernel<<<ceil_div(n, 256), 256, 0, c->stream>>>(c->w_fdesc.as<uint32_t>(), n, a->vals.as<uint64_t>(), a->set.as<uint32_t>(), a->slots, d_val, d_flag);
  COLTT_HIP(hipGetLastError());
  COLTT_HIP(hipMemcpyAsync(c->h_out.p, d_val, n * 9, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));
  if (out_values) std::memcpy(out_values, c->h_out.p, n * 8);
  if (out_set) std::memcpy(out_set, static_cast<const uint8_t*>(c->h_out.p) + n * 8, n);
  return COLTT_OK;
}

int coltt_attr_cmp_host(int type, int op, const void* operand, const void* value, int is_set) {
  if (type != COLTT_ATTR_I64 && type != COLTT_ATTR_F64) return fail(COLTT_E_INVALID, "attr_cmp_host: unknown type %d", type);
  if (op < COLTT_CMP_EQ || op > COLTT_CMP_SET) return fail(COLTT_E_INVALID, "attr_cmp_host: unknown op %d", op);
  uint64_t o = 0, v = 0;
  if (op != COLTT_CMP_SET) {
    if (!operand) return fail(COLTT_E_INVALID, "attr_cmp_host: NULL operand");
    std::memcpy(&o, operand, 8);
    if (type == COLTT_ATTR_F64 && attr_is_nan(o)) return fail(COLTT_E_INVALID, "attr_cmp_host: a NaN operand");
  }
  if (is_set) {
    if (!value) return fail(COLTT_E_INVALID, "attr_cmp_host: NULL value");
    std::memcpy(&v, value, 8);
    if (type == COLTT_ATTR_F64 && attr_is_nan(v)) return fail(COLTT_E_INVALID, "attr_cmp_host: a NaN value (no column holds one)");
  }
  return is_set && attr_cmp(type, op, v, o) ? 1 : 0;
}

int coltt_hnsw_filter_info(coltt_handle_t fh, coltt_handle_t* out_index, uint64_t* out_allowed, uint64_t* out_slots) {
  auto f = lookup<HnswFilter>(fh);
  if (!f) return fail(COLTT_E_NOT_FOUND, "hnsw_filter_info: unknown filter handle");
  // coltt_hnsw_compact_carry swaps `allowed` and `slots` under the index's exclusive lock: read the pair under the shared one while the index exists
  auto x = lookup<Hnsw>(f->index);
  ReadLock g;
  if (x) g = ReadLock(x->rw);
  if (out_index) *out_index = f->index;
  if (out_allowed) *out_allowed = f->allowed;
  if (out_slots) *out_slots = f->slots;
  return COLTT_OK;
}

int coltt_hnsw_filter_ids(coltt_handle_t fh, uint64_t* out_ids, uint64_t cap, uint64_t* out_n) {
  auto f = lookup<HnswFilter>(fh);   // held until the call returns
  if (!f) return fail(COLTT_E_NOT_FOUND, "hnsw_filter_ids: unknown filter handle");
  if (cap && !out_ids) return fail(COLTT_E_INVALID, "hnsw_filter_ids: NULL out_ids");
  auto x = lookup<Hnsw>(f->index);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_filter_ids: the filter's index is gone");
  ReadLock g(x->rw);
  if (f->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_filter_ids: the filter is stale (the index was loaded since it was built)");
  if (out_n) *out_n = f->allowed;
  const uint64_t m = std::min<uint64_t>(cap, f->allowed);
  if (m == 0) return COLTT_OK;
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  HCtx* c = ctx.c;
  COLTT_TRY(c->w_out_ids.reserve(m * 8));
  filter_ids_kernel<<<ceil_div(m, 256), 256, 0, c->stream>>>(f->list.as<uint32_t>(), m, x->dense ? nullptr : x->ids.as<uint64_t>(), x->dense_base,
                                                             c->w_out_ids.as<uint64_t>());
  COLTT_HIP(hipGetLastError());
  COLTT_HIP(hipMemcpyAsync(out_ids, c->w_out_ids.p, m * 8, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));
  return COLTT_OK;
}

}  // extern "C"
