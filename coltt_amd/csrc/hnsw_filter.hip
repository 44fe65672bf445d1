// hnsw_filter.hip — filtered search: an allow-list of ids against one index (coltt_hnsw_search_filtered and its batch and product-quantised
// forms).  An extension the reference does not have (its Core.HybridSearch post-filters an unfiltered search): definitions in
// include/coltt_gpu.h.  The filter objects themselves (create, expressions, attribute columns): hnsw.hip.
#include <algorithm>
#include <cmath>
#include <map>

#include "hnsw_index.hpp"
#include "hnsw_kernels.hpp"   // the filtered one-wave walks, the exact scan and its select

using namespace coltt;
using namespace coltt::dev;
using namespace coltt::kern;
using namespace coltt::hnsw;

// coltt_hnsw_search_filtered, EXACT, step 2 (step 1: hnsw_kernels.hpp, hnsw_filter_scan_kernel).  Not a template: it stands in the one translation
// unit that launches it.
namespace coltt {
namespace kern {
// step 2: one wave per query merges its chunks' lists (the same top-k in LDS) and writes the answer ascending
__global__ __launch_bounds__(64) void hnsw_filter_select_kernel(const unsigned long long* __restrict__ part, const uint32_t* __restrict__ part_cnt,
                                                                uint32_t nchunks, uint32_t k, const uint64_t* __restrict__ ids, uint64_t* __restrict__ out_ids,
                                                                float* __restrict__ out_scores, uint32_t* __restrict__ out_counts) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  unsigned long long* const top = reinterpret_cast<unsigned long long*>(smem);
  const size_t q = blockIdx.x;
  const int lane_in = threadIdx.x;
  uint32_t len = 0;
  for (uint32_t c = 0; c < nchunks; c++) {
    const uint32_t cnt = part_cnt[q * nchunks + c];
    const unsigned long long* src = part + (q * nchunks + c) * k;
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

namespace {

// AUTO: with A allowed vertices out of n_live, a walk at ef meets about ef * A / n_live allowed ones among its result-set-sized share of
// the walk; ef_need raises the breadth so that about ef of them are met.  The exact scan reads A rows and has no dependent chain; the walk
// evaluates about 32 rows per unit of ef (n_dist / ef = 4 040 / 128 on the headline collection), so the scan wins on rows read while
// A <= FILTER_ROWS_PER_EF * ef_walk.
constexpr uint64_t FILTER_EF_MAX = 4096;
#ifndef COLTT_FILTER_ROWS_PER_EF
#define COLTT_FILTER_ROWS_PER_EF 32
#endif
int filter_path(uint64_t allowed, uint64_t n_live, uint32_t ef, int mode, uint32_t& ef_walk) {
  ef_walk = ef;
  if (mode == COLTT_FILTER_WALK) return COLTT_FILTER_WALK;
  if (mode == COLTT_FILTER_EXACT || allowed == 0) return COLTT_FILTER_EXACT;
  const uint64_t ef_need = ((uint64_t)ef * n_live + allowed - 1) / allowed;
  ef_walk = (uint32_t)std::min<uint64_t>(FILTER_EF_MAX, std::max<uint64_t>(ef, ef_need));
  if (ef_need > FILTER_EF_MAX || allowed <= (uint64_t)COLTT_FILTER_ROWS_PER_EF * ef_walk) return COLTT_FILTER_EXACT;
  return COLTT_FILTER_WALK;
}

// ---- What the filtered drivers share (filter_search_common, filter_batch_common, pq_filter_search_common, pq_filter_batch_common); `who` is the entry
// point's name in the messages.

// The argument checks and the breadth.  ef == 0 on COLTT_OK: no queries, nothing to do.
int filter_args(const Hnsw* x, const char* who, size_t nq, uint32_t k, uint32_t ef_override, int mode, coltt_hnsw_filter_stats* st, uint32_t& ef) {
  std::memset(st, 0, sizeof(*st));
  ef = 0;
  if (mode != COLTT_FILTER_AUTO && mode != COLTT_FILTER_WALK && mode != COLTT_FILTER_EXACT) return fail(COLTT_E_INVALID, "%s: unknown mode %d", who, mode);
  if (nq == 0) return COLTT_OK;
  if (k == 0) return fail(COLTT_E_INVALID, "%s: k must be >= 1", who);
  if (nq > 0xffffffffull) return fail(COLTT_E_UNSUPPORTED, "%s: more than 2^32-1 queries in one call", who);
  const uint32_t e = std::max<uint32_t>(ef_override ? ef_override : (uint32_t)x->cfg.ef, k);   // as Search (hnsw.go:258)
  if (e > FILTER_EF_MAX) return fail(COLTT_E_UNSUPPORTED, "%s: ef=%u > %llu", who, e, (unsigned long long)FILTER_EF_MAX);
  ef = e;
  return COLTT_OK;
}

// Each query's path from its own filter's allowed count (n_live read once, under the caller's read lock).  walk_q / exact_q: the served
// queries (a non-empty filter on a non-empty index); none served — only empty filters, or an empty index — is counts 0, not an error.
struct FiltRoute {
  std::vector<uint32_t> efw, walk_q, exact_q;
  bool none() const { return walk_q.empty() && exact_q.empty(); }
};
void filter_route(const Hnsw* x, const std::vector<HnswFilter*>& fl, size_t nq, uint32_t ef, int mode, int32_t* out_paths, uint32_t* out_counts,
                  coltt_hnsw_filter_stats* st, FiltRoute& r) {
  const uint64_t n_live = x->live;
  r.efw.resize(nq);
  bool any_walk = false, any_exact = false;
  for (size_t i = 0; i < nq; i++) {
    const int path = filter_path(fl[i]->allowed, n_live, ef, mode, r.efw[i]);
    if (out_paths) out_paths[i] = path;
    if (path == COLTT_FILTER_WALK) { any_walk = true; st->ef_walk = std::max(st->ef_walk, r.efw[i]); }
    else any_exact = true;
    if (x->entry < 0 || fl[i]->allowed == 0) continue;
    (path == COLTT_FILTER_WALK ? r.walk_q : r.exact_q).push_back((uint32_t)i);
  }
  st->path = any_walk && any_exact ? COLTT_FILTER_AUTO : any_walk ? COLTT_FILTER_WALK : COLTT_FILTER_EXACT;
  if (r.none()) std::memset(out_counts, 0, nq * 4);
}

// The wave of the exact scan (hnsw_filter_scan_kernel and its batch form): up to FILT_QG queries while the wave's LDS — the queries and one
// top-k each — stays within 64 KiB (two waves per SIMD); a single query may take up to the CU's 160 KiB.  kbytes: one top-k, the select's LDS.
struct FiltExactGeom { uint32_t qg = 0; size_t lds = 0, kbytes = 0; };
int filter_exact_geom(const Hnsw* x, uint32_t k, const char* who, FiltExactGeom& out) {
  const size_t qbytes = (((size_t)x->dim + 3) & ~(size_t)3) * 4, kbytes = (size_t)((k + 63) & ~63u) * 8;
  uint32_t qg = FILT_QG;
  while (qg > 1 && qg * (qbytes + kbytes) > 64 * 1024) qg--;
  const size_t lds = qg * (qbytes + kbytes);
  if (lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "%s: dim %u / k %u need %zu B of LDS (> 160 KiB)", who, x->dim, k, lds);
  out.qg = qg; out.lds = lds; out.kbytes = kbytes;
  return COLTT_OK;
}

// The exact path of a batch with a filter per query (coltt_hnsw_search_filtered_batch, coltt_hnsw_pq_search_filtered_batch): the rows of exact_q
// sorted by filter, groups of <= geom.qg sharing one, chunk lists as launch_filter_exact sizes them.
// eq / tiles: what the scan and the select read; d_eq / d_tiles: where filter_upload put them.
struct FiltExactPlan {
  FiltExactGeom geom; std::vector<FiltExactQ> eq; std::vector<FiltTile> tiles; uint64_t nlists = 0;
  const FiltExactQ* d_eq = nullptr; const FiltTile* d_tiles = nullptr;
};

// The answer's three device buffers.
struct FiltOut { uint64_t* oi; float* os; uint32_t* oc; };

template <int METRIC, int QUANT>
int launch_search_filtered_batch(Hnsw* x, HCtx* c, bool visg, size_t lds, uint32_t grid, uint32_t region_base, uint32_t nw, uint32_t k,
                                 const FiltQuery* fq, uint32_t* counter, uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  auto kern = visg ? hnsw_search_filtered_batch_kernel<METRIC, QUANT, true> : hnsw_search_filtered_batch_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (x->r8) kern = visg ? hnsw_search_filtered_batch_kernel<METRIC, QUANT, true, true> : hnsw_search_filtered_batch_kernel<METRIC, QUANT, false, true>; }
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, 64, lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nw, k, fq, counter, oi, os, oc, stats,
                                     x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                     x->w_vepoch.as<uint32_t>() + region_base);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

template <int METRIC, int QUANT>
int launch_filter_exact_batch(Hnsw* x, HCtx* c, const FiltExactPlan& ep, uint32_t k, const FiltOut& o, unsigned long long* stats) {
  const size_t lds = ep.geom.lds, kbytes = ep.geom.kbytes;
  COLTT_TRY(c->w_keys.reserve((size_t)ep.nlists * k * 8));
  COLTT_TRY(c->w_scnt.reserve((size_t)ep.nlists * 4));
  GraphView gv = x->view();
  auto scan = hnsw_filter_scan_batch_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (x->r8) scan = hnsw_filter_scan_batch_kernel<METRIC, QUANT, true>; }
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(scan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  scan<<<(uint32_t)ep.tiles.size(), 64, lds, c->stream>>>(gv, c->w_qeff.as<float>(), c->w_qn.as<float>(), ep.d_tiles, ep.d_eq, ep.geom.qg, k, (k + 63) & ~63u,
                                                          c->w_keys.as<unsigned long long>(), c->w_scnt.as<uint32_t>(), stats);
  COLTT_HIP(hipGetLastError());
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_filter_select_batch_kernel<>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kbytes));
  hnsw_filter_select_batch_kernel<><<<(uint32_t)ep.eq.size(), 64, kbytes, c->stream>>>(c->w_keys.as<unsigned long long>(), c->w_scnt.as<uint32_t>(), ep.d_eq, k, gv.ids,
                                                                                       o.oi, o.os, o.oc);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}
// the exact scan and its select over the uploaded plan, if any query took the exact path
int run_filter_exact(Hnsw* x, HCtx* c, const FiltExactPlan& ep, uint32_t k, const FiltOut& o, unsigned long long* d_stats) {
  if (ep.eq.empty()) return COLTT_OK;
  const bool cos = x->metric == COLTT_COSINE;
  int rc = COLTT_OK;
#define COLTT_FE(Q) rc = cos ? launch_filter_exact_batch<M_COS, Q>(x, c, ep, k, o, d_stats) : launch_filter_exact_batch<M_L2, Q>(x, c, ep, k, o, d_stats)
  COLTT_DISPATCH_QUANT(x->quant, COLTT_FE)
#undef COLTT_FE
  return rc;
}

// FiltExactPlan for the rows of exact_q (sorted in place)
int plan_filter_exact_batch(Hnsw* x, const std::vector<HnswFilter*>& fl, std::vector<uint32_t>& exact_q, uint32_t k, const char* who, FiltExactPlan& out) {
  std::vector<FiltExactQ>& eq = out.eq;
  std::vector<FiltTile>& tiles = out.tiles;
  uint64_t& nlists = out.nlists;
  eq.clear(); tiles.clear(); nlists = 0;
  if (!exact_q.empty()) {
    COLTT_TRY(filter_exact_geom(x, k, who, out.geom));
    const uint32_t qg = out.geom.qg;
    std::stable_sort(exact_q.begin(), exact_q.end(), [&](uint32_t a, uint32_t b) { return std::less<const HnswFilter*>()(fl[a], fl[b]); });
    struct Run { size_t first, len; uint64_t nch, chunk; };
    std::vector<Run> runs;
    uint64_t groups = 0;
    for (size_t a = 0; a < exact_q.size();) {
      size_t b = a;
      while (b < exact_q.size() && fl[exact_q[b]] == fl[exact_q[a]]) b++;
      runs.push_back(Run{a, b - a, 0, 0});
      groups += ceil_div(b - a, qg);
      a = b;
    }
    for (Run& r : runs) r.nch = std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(4096, groups), ceil_div(fl[exact_q[r.first]]->allowed, 256)));
    auto lists = [&] { uint64_t t = 0; for (const Run& r : runs) t += r.len * r.nch; return t; };
    while (lists() * k * 8 > (256ull << 20)) {   // the chunk lists' workspace
      bool any = false;
      for (Run& r : runs) if (r.nch > 1) { r.nch = (r.nch + 1) / 2; any = true; }
      if (!any) break;
    }
    for (Run& r : runs) {
      const HnswFilter* f = fl[exact_q[r.first]];
      const uint64_t A = f->allowed;
      r.chunk = (((A + r.nch - 1) / r.nch) + 31) & ~31ull;
      r.nch = (A + r.chunk - 1) / r.chunk;
      for (size_t j = 0; j < r.len; j++) {
        eq.push_back(FiltExactQ{exact_q[r.first + j], (uint32_t)nlists, (uint32_t)r.nch, 0u});
        nlists += r.nch;
      }
      for (size_t g0 = 0; g0 < r.len; g0 += qg)
        for (uint64_t ch = 0; ch < r.nch; ch++)
          tiles.push_back(FiltTile{f->list.as<uint32_t>(), (uint32_t)(ch * r.chunk), (uint32_t)std::min<uint64_t>(A, (ch + 1) * r.chunk),
                                   (uint32_t)(r.first + g0), (uint32_t)std::min<size_t>(qg, r.len - g0), (uint32_t)ch, 0u});
    }
    if (nlists > 0xffffffffull || tiles.size() > 0x7fffffffull) return fail(COLTT_E_UNSUPPORTED, "%s: too many exact-path chunk lists", who);
  }
  return COLTT_OK;
}

// One upload of every table of a call into w_fdesc — [walk descriptors w0 | w1][exact queries][tiles, 32-byte aligned] — then the answer's
// buffers, the counts cleared.  blob is the caller's: the host copy outlives the transfer.  desc: the blob on the device (w0 at desc, w1 at desc + w0_bytes).
int filter_upload(HCtx* c, const void* w0, size_t w0_bytes, const void* w1, size_t w1_bytes, FiltExactPlan& ep, size_t nq, uint32_t k,
                  std::vector<uint8_t>& blob, uint8_t*& desc, FiltOut& o) {
  const size_t o_eq = w0_bytes + w1_bytes;
  const size_t o_t = (o_eq + ep.eq.size() * sizeof(FiltExactQ) + 31) & ~(size_t)31, o_end = o_t + ep.tiles.size() * sizeof(FiltTile);
  blob.resize(o_end);
  if (w0_bytes) std::memcpy(blob.data(), w0, w0_bytes);
  if (w1_bytes) std::memcpy(blob.data() + w0_bytes, w1, w1_bytes);
  if (!ep.eq.empty()) std::memcpy(blob.data() + o_eq, ep.eq.data(), ep.eq.size() * sizeof(FiltExactQ));
  if (!ep.tiles.empty()) std::memcpy(blob.data() + o_t, ep.tiles.data(), ep.tiles.size() * sizeof(FiltTile));
  COLTT_TRY(c->w_fdesc.reserve(o_end));
  desc = c->w_fdesc.as<uint8_t>();
  ep.d_eq = reinterpret_cast<const FiltExactQ*>(desc + o_eq);
  ep.d_tiles = reinterpret_cast<const FiltTile*>(desc + o_t);
  COLTT_HIP(hipMemcpyAsync(desc, blob.data(), o_end, hipMemcpyHostToDevice, c->stream));
  COLTT_TRY(c->w_out_ids.reserve(nq * k * 8));
  COLTT_TRY(c->w_out_sc.reserve(nq * k * 4));
  COLTT_TRY(c->w_out_cnt.reserve(nq * 4));
  o = FiltOut{c->w_out_ids.as<uint64_t>(), c->w_out_sc.as<float>(), c->w_out_cnt.as<uint32_t>()};
  COLTT_HIP(hipMemsetAsync(o.oc, 0, nq * 4, c->stream));   // rows of empty filters stay at count 0
  return COLTT_OK;
}

// The queries of a call whose walks read the prepared batch in place: up to the device and Normalize / Lower as Search does — which also clears
// the first 256 bytes of w_misc: the work counters (counters[0], [1]) and, 16 bytes in, the traversal counters (d_stats) — then the start of the kernel time.
int filter_queries(Hnsw* x, HCtx* c, const float* queries, size_t nq, uint32_t*& counters, unsigned long long*& d_stats) {
  COLTT_TRY(c->w_qraw.reserve(nq * x->dim * 4));
  COLTT_HIP(hipMemcpyAsync(c->w_qraw.p, queries, nq * x->dim * 4, hipMemcpyHostToDevice, c->stream));
  COLTT_TRY(c->w_misc.reserve(256));
  COLTT_TRY(c->h_out.reserve(256));   // where filter_finish reads the counters back
  uint8_t* misc = c->w_misc.as<uint8_t>();
  counters = reinterpret_cast<uint32_t*>(misc);
  d_stats = reinterpret_cast<unsigned long long*>(misc + 16);
  COLTT_TRY(prep_queries_any(x, c, c->w_qraw.as<float>(), nq, reinterpret_cast<uint32_t*>(misc)));
  COLTT_HIP(hipEventRecord(c->ev0, c->stream));
  return COLTT_OK;
}

// The end of a call: the answer and (unless the caller has read them: have_stats) the six counters back to the host, the kernel time, the watchdog.
int filter_finish(Hnsw* x, HCtx* c, const char* who, const FiltOut& o, size_t nq, uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                  const unsigned long long* d_stats, unsigned long long* h_stats, bool have_stats) {
  COLTT_HIP(hipEventRecord(c->ev1, c->stream));
  if (x->dense && x->dense_base) add_base(c->stream, o.oi, nq * k, x->dense_base);
  COLTT_HIP(hipMemcpyAsync(out_ids, o.oi, nq * k * 8, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipMemcpyAsync(out_scores, o.os, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipMemcpyAsync(out_counts, o.oc, nq * 4, hipMemcpyDeviceToHost, c->stream));
  if (!have_stats) COLTT_HIP(hipMemcpyAsync(c->h_out.p, d_stats, 48, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));   // the lease, the host tables and the callers' filters outlive the kernels
  if (!have_stats) std::memcpy(h_stats, c->h_out.p, 48);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  x->last_ms.store(ms);
  if (h_stats[4]) return fail(COLTT_E_DEVICE, "%s: traversal watchdog tripped (code %llu)", who, h_stats[4]);
  return COLTT_OK;
}

// ---- coltt_hnsw_search_filtered: one filter for the whole call.
template <int METRIC, int QUANT>
int launch_search_filtered(Hnsw* x, HCtx* c, const SearchGeom& sg, const HnswFilter* f, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k,
                           uint32_t* counter, uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  auto kern = sg.visg ? hnsw_search_filtered_kernel<METRIC, QUANT, true> : hnsw_search_filtered_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (x->r8) kern = sg.visg ? hnsw_search_filtered_kernel<METRIC, QUANT, true, true> : hnsw_search_filtered_kernel<METRIC, QUANT, false, true>; }
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sg.lds));
  kern<<<grid, 64, sg.lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                        k, sg.ef, sg.ef_pad, sg.hcap, counter, oi, os, oc, stats,
                                        x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                        x->w_vepoch.as<uint32_t>() + region_base, FilterView{f->bits.as<uint32_t>(), f->slots});
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

template <int METRIC, int QUANT>
int launch_filter_exact(Hnsw* x, HCtx* c, const HnswFilter* f, uint32_t nq, uint32_t k, uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  // geometry: the wave's (filter_exact_geom); enough (group, chunk) waves to fill the device (4096), chunks of >= 256 slots
  FiltExactGeom eg;
  COLTT_TRY(filter_exact_geom(x, k, "hnsw_search_filtered", eg));
  const uint32_t qg = eg.qg;
  const size_t lds = eg.lds;
  if (lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "hnsw_search_filtered: dim %u / k %u need %zu B of LDS (> 160 KiB)", x->dim, k, lds);
  const uint32_t groups = ceil_div(nq, qg);
  const uint64_t A = f->allowed;
  uint64_t nchunks = std::max<uint64_t>(1, std::min<uint64_t>(ceil_div(4096, groups), ceil_div(A, 256)));
  while (nchunks > 1 && (uint64_t)nq * nchunks * k * 8 > (256ull << 20)) nchunks = (nchunks + 1) / 2;   // the chunk lists' workspace
  uint64_t chunk = (A + nchunks - 1) / nchunks;
  chunk = (chunk + 31) & ~31ull;
  nchunks = (A + chunk - 1) / chunk;
  COLTT_TRY(c->w_keys.reserve((size_t)nq * nchunks * k * 8));
  COLTT_TRY(c->w_scnt.reserve((size_t)nq * nchunks * 4));
  GraphView gv = x->view();
  auto scan = hnsw_filter_scan_kernel<METRIC, QUANT, false>;
  if constexpr (QUANT != Q_F8) { if (x->r8) scan = hnsw_filter_scan_kernel<METRIC, QUANT, true>; }
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(scan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  scan<<<dim3((uint32_t)nchunks, groups), 64, lds, c->stream>>>(gv, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq, qg, f->list.as<uint32_t>(), (uint32_t)A,
                                                                (uint32_t)chunk, k, (k + 63) & ~63u, c->w_keys.as<unsigned long long>(), c->w_scnt.as<uint32_t>(), stats);
  COLTT_HIP(hipGetLastError());
  const size_t lds2 = eg.kbytes;
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(hnsw_filter_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
  hnsw_filter_select_kernel<<<nq, 64, lds2, c->stream>>>(c->w_keys.as<unsigned long long>(), c->w_scnt.as<uint32_t>(), (uint32_t)nchunks, k, gv.ids, oi, os, oc);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

int filter_search_common(Hnsw* x, HCtx* c, const HnswFilter* f, const float* queries, size_t nq, uint32_t k, uint32_t ef_override, int mode,
                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_filter_stats* st) {
  const char* const who = "hnsw_search_filtered";
  coltt_hnsw_filter_stats local{};
  if (!st) st = &local;
  uint32_t ef;
  COLTT_TRY(filter_args(x, who, nq, k, ef_override, mode, st, ef));
  if (!ef) return COLTT_OK;
  uint32_t ef_walk = ef;
  const int path = filter_path(f->allowed, x->live, ef, mode, ef_walk);
  st->path = path; st->ef_walk = path == COLTT_FILTER_WALK ? ef_walk : 0;
  if (x->entry < 0 || f->allowed == 0) {   // empty index or empty filter: counts 0, not an error
    std::memset(out_counts, 0, nq * 4);
    return COLTT_OK;
  }
  COLTT_TRY(c->w_out_ids.reserve(nq * k * 8));
  COLTT_TRY(c->w_out_sc.reserve(nq * k * 4));
  COLTT_TRY(c->w_out_cnt.reserve(nq * 4));
  const FiltOut o{c->w_out_ids.as<uint64_t>(), c->w_out_sc.as<float>(), c->w_out_cnt.as<uint32_t>()};
  SearchGeom sg{};
  uint32_t grid = 0;
  RegionLease lease;
  if (path == COLTT_FILTER_WALK) {
    const Policy pol = policy();
    if (wants_visg(pol, ef_walk)) COLTT_TRY(ensure_visg(x, pol));
    sg = walk_geom(plan_facts(x), pol, ef_walk, k);   // the one-wave walk (hnsw_dev.hpp: search_level) over the LDS hash or the HBM byte map
    if (sg.lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "%s: dim/ef/k need %zu B of LDS (> 160 KiB)", who, sg.lds);
    grid = std::min<uint32_t>((uint32_t)nq, resident_waves(pol, x->quant, sg.lds));
    if (sg.visg) { acquire_regions(x, grid, lease); grid = lease.count; }
  }
  uint32_t* counter;
  unsigned long long* d_stats;
  COLTT_TRY(filter_queries(x, c, queries, nq, counter, d_stats));
  int rc = COLTT_OK;
#define COLTT_FS(Q) rc = path == COLTT_FILTER_WALK \
    ? (x->metric == COLTT_COSINE ? launch_search_filtered<M_COS, Q>(x, c, sg, f, grid, lease.base, (uint32_t)nq, k, counter, o.oi, o.os, o.oc, d_stats) \
                                 : launch_search_filtered<M_L2, Q>(x, c, sg, f, grid, lease.base, (uint32_t)nq, k, counter, o.oi, o.os, o.oc, d_stats)) \
    : (x->metric == COLTT_COSINE ? launch_filter_exact<M_COS, Q>(x, c, f, (uint32_t)nq, k, o.oi, o.os, o.oc, d_stats) \
                                 : launch_filter_exact<M_L2, Q>(x, c, f, (uint32_t)nq, k, o.oi, o.os, o.oc, d_stats))
  COLTT_DISPATCH_QUANT(x->quant, COLTT_FS)
#undef COLTT_FS
  COLTT_TRY(rc);
  unsigned long long h_stats[6];
  COLTT_TRY(filter_finish(x, c, who, o, nq, k, out_ids, out_scores, out_counts, d_stats, h_stats, false));
  st->n_dist = h_stats[0]; st->n_exp = h_stats[1]; st->n_hops = h_stats[2]; st->n_visit_resets = h_stats[3]; st->n_exact_rows = h_stats[5];
  return COLTT_OK;
}

// ---- coltt_hnsw_search_filtered_batch: a filter per query.  Row i is the single-filter call on query i alone: its path from its own filter's
// allowed count (filter_path), its walk at the geometry walk_geom gives its ef_walk, its exact scan chunked by launch_filter_exact's rule (the
// answer is a pure top-k, so the chunking cannot change it).  One call launches at most two walks (LDS hash, HBM byte map), one scan, one select.
int filter_batch_common(Hnsw* x, HCtx* c, const std::vector<HnswFilter*>& fl, const float* queries, size_t nq, uint32_t k, uint32_t ef_override,
                        int mode, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, int32_t* out_paths, coltt_hnsw_filter_stats* st) {
  const char* const who = "hnsw_search_filtered_batch";
  coltt_hnsw_filter_stats local{};
  if (!st) st = &local;
  uint32_t ef;
  COLTT_TRY(filter_args(x, who, nq, k, ef_override, mode, st, ef));
  if (!ef) return COLTT_OK;
  FiltRoute rt;
  filter_route(x, fl, nq, ef, mode, out_paths, out_counts, st, rt);
  if (rt.none()) return COLTT_OK;
  // the walks: each query's geometry is walk_geom(facts, policy, ef_walk, k), the one-wave walk (hnsw_dev.hpp: search_level) over the LDS hash
  // or the HBM byte map; split by visited set
  const Policy pol = policy();
  for (uint32_t i : rt.walk_q)
    if (wants_visg(pol, rt.efw[i])) { COLTT_TRY(ensure_visg(x, pol)); break; }
  const PlanFacts facts = plan_facts(x);
  std::map<uint32_t, SearchGeom> geoms;
  std::vector<FiltQuery> wq[2];
  SearchGeom wmax[2]{};
  for (uint32_t i : rt.walk_q) {
    auto it = geoms.find(rt.efw[i]);
    if (it == geoms.end()) it = geoms.emplace(rt.efw[i], walk_geom(facts, pol, rt.efw[i], k)).first;
    const SearchGeom& sg = it->second;
    if (sg.lds > 160 * 1024) return fail(COLTT_E_UNSUPPORTED, "%s: dim/ef/k need %zu B of LDS (> 160 KiB)", who, sg.lds);
    const int v = sg.visg ? 1 : 0;
    wq[v].push_back(FiltQuery{fl[i]->bits.as<uint32_t>(), fl[i]->slots, sg.ef, sg.ef_pad, sg.hcap, i, 0u});
    if (wq[v].size() == 1 || sg.lds > wmax[v].lds) wmax[v] = sg;   // the launch's LDS: its largest query's
  }
  FiltExactPlan ep;
  COLTT_TRY(plan_filter_exact_batch(x, fl, rt.exact_q, k, who, ep));
  // the tables: [walks over the LDS hash][walks over the byte map][exact queries][tiles]
  std::vector<uint8_t> blob;
  uint8_t* d_desc;
  FiltOut o;
  const size_t w0_bytes = wq[0].size() * sizeof(FiltQuery);
  COLTT_TRY(filter_upload(c, wq[0].data(), w0_bytes, wq[1].data(), wq[1].size() * sizeof(FiltQuery), ep, nq, k, blob, d_desc, o));
  uint32_t grid[2] = {0, 0};
  RegionLease lease;
  for (int v = 0; v < 2; v++) if (!wq[v].empty()) grid[v] = std::min<uint32_t>((uint32_t)wq[v].size(), resident_waves(pol, x->quant, wmax[v].lds));
  if (grid[1]) { acquire_regions(x, grid[1], lease); grid[1] = lease.count; }
  uint32_t* counters;   // [0]: the LDS-hash walk's work counter, [1]: the byte-map walk's
  unsigned long long* d_stats;
  COLTT_TRY(filter_queries(x, c, queries, nq, counters, d_stats));
  int rc = COLTT_OK;
  const bool cos = x->metric == COLTT_COSINE;
  for (int v = 0; v < 2 && rc == COLTT_OK; v++) {
    if (!grid[v]) continue;
    const FiltQuery* fq = reinterpret_cast<const FiltQuery*>(d_desc + (v ? w0_bytes : 0));
    const uint32_t nw = (uint32_t)wq[v].size();
#define COLTT_FW(Q) rc = cos ? launch_search_filtered_batch<M_COS, Q>(x, c, v == 1, wmax[v].lds, grid[v], lease.base, nw, k, fq, counters + v, o.oi, o.os, o.oc, d_stats) \
                         : launch_search_filtered_batch<M_L2, Q>(x, c, v == 1, wmax[v].lds, grid[v], lease.base, nw, k, fq, counters + v, o.oi, o.os, o.oc, d_stats)
    COLTT_DISPATCH_QUANT(x->quant, COLTT_FW)
#undef COLTT_FW
  }
  COLTT_TRY(rc);
  COLTT_TRY(run_filter_exact(x, c, ep, k, o, d_stats));
  unsigned long long h_stats[6];
  COLTT_TRY(filter_finish(x, c, who, o, nq, k, out_ids, out_scores, out_counts, d_stats, h_stats, false));
  st->n_dist = h_stats[0]; st->n_exp = h_stats[1]; st->n_hops = h_stats[2]; st->n_visit_resets = h_stats[3]; st->n_exact_rows = h_stats[5];
  return COLTT_OK;
}

// coltt_hnsw_pq_search_filtered (the entry point has checked that the index carries codes): the path is filter_path's, word for word; EXACT is filter_search_common's, WALK the walk over the quantiser's codes
// at ef_walk (pq_search_once: the same grouping of queries, region lease, neighbourhood blocks and retry over the byte map) with the allowed set.
int pq_filter_search_common(Hnsw* x, HCtx* c, const HnswFilter* f, const float* queries, size_t nq, uint32_t k, uint32_t ef_override, uint32_t rerank, int mode,
                            uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_filter_stats* st) {
  coltt_hnsw_filter_stats local{};
  if (!st) st = &local;
  uint32_t ef;
  COLTT_TRY(filter_args(x, "hnsw_pq_search_filtered", nq, k, ef_override, mode, st, ef));
  if (!ef) return COLTT_OK;
  uint32_t ef_walk = ef;
  const int path = filter_path(f->allowed, x->live, ef, mode, ef_walk);
  if (path == COLTT_FILTER_EXACT) return filter_search_common(x, c, f, queries, nq, k, ef_override, COLTT_FILTER_EXACT, out_ids, out_scores, out_counts, st);
  st->path = COLTT_FILTER_WALK; st->ef_walk = ef_walk;
  if (x->entry < 0 || f->allowed == 0) {   // empty index or empty filter: counts 0, not an error
    std::memset(out_counts, 0, nq * 4);
    return COLTT_OK;
  }
  coltt_hnsw_stats ws{};
  uint64_t n_exact = 0;
  const FilterView fv{f->bits.as<uint32_t>(), f->slots};
  COLTT_TRY(pq_search_filtered_walk(x, c, fv, queries, nq, k, ef_walk, rerank, out_ids, out_scores, out_counts, &ws, &n_exact));
  st->n_dist = ws.n_dist; st->n_exp = ws.n_exp; st->n_hops = ws.n_hops; st->n_visit_resets = 0; st->n_exact_rows = n_exact;
  return COLTT_OK;
}

// ---- coltt_hnsw_pq_search_filtered_batch: a filter per query over the walk on the quantiser's codes.  Row i is coltt_hnsw_pq_search_filtered on query i
// alone: its path from its own filter (filter_path), its walk at ef_walk with the geometry and the capacity of R the single call gives it (pq_walk_geom,
// pq_filt_cap), EXACT rows through the row batch's exact scan.  The walking queries are compacted (their prepared vectors gathered side by side: the
// tables, survivors and keys are addressed by position in the launch) and run as at most two walk launches per group of queries — LDS hash, byte map — each
// followed by the re-rank over its survivors; the select kernel answers the batch row of each.  A query whose LDS-hash walk reports the reset code runs
// once more over the byte map, as the single call re-runs itself, and is counted once.
__global__ void pq_gather_queries_kernel(const float* __restrict__ q_eff, const float* __restrict__ qnorms, const PqFiltQuery* __restrict__ pd, uint32_t dim,
                                         float* __restrict__ out_q, float* __restrict__ out_n) {
  const uint32_t j = blockIdx.x, row = pd[j].row;
  for (uint32_t e = threadIdx.x; e < dim; e += blockDim.x) out_q[(size_t)j * dim + e] = q_eff[(size_t)row * dim + e];
  if (threadIdx.x == 0) out_n[j] = qnorms[row];
}

int pq_filter_batch_common(Hnsw* x, HCtx* c, const std::vector<HnswFilter*>& fl, const float* queries, size_t nq, uint32_t k, uint32_t ef_override,
                           uint32_t rerank, int mode, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, int32_t* out_paths,
                           coltt_hnsw_filter_stats* st) {
  const char* const who = "hnsw_pq_search_filtered_batch";
  coltt_hnsw_filter_stats local{};
  if (!st) st = &local;
  uint32_t ef;
  COLTT_TRY(filter_args(x, who, nq, k, ef_override, mode, st, ef));
  if (!ef) return COLTT_OK;
  FiltRoute rt;
  filter_route(x, fl, nq, ef, mode, out_paths, out_counts, st, rt);
  if (rt.none()) return COLTT_OK;
  const std::vector<uint32_t>& efw = rt.efw;
  if (!rt.walk_q.empty() && x->pq_done != x->n)
    return fail(COLTT_E_DEVICE, "%s: codes cover %llu of %llu slots", who, (unsigned long long)x->pq_done, (unsigned long long)x->n);
  // the walks: each query's geometry is the single call's for its ef_walk; split by visited set.  A launch takes the LDS of its largest query, keeps
  // as many traversals per CU as that one allows, and its survivors' rows are as long as its longest result set
  struct Launch { std::vector<PqFiltQuery> q; size_t lds = 0; uint32_t ef_pad = 0, per_cu = 0; };
  Launch wl[2];
  auto add_walk = [&](Launch& l, const PqGeom& sg, uint32_t fcap, uint32_t i) {
    l.q.push_back(PqFiltQuery{fl[i]->bits.as<uint32_t>(), fl[i]->slots, sg.ef, sg.ef_pad, sg.vis_words, fcap, i, 0u, 0u});
    if (l.q.size() == 1 || sg.lds > l.lds) { l.lds = sg.lds; l.per_cu = sg.per_cu; }
    l.ef_pad = std::max(l.ef_pad, sg.ef_pad);
  };
  {
    std::map<uint32_t, PqGeom> geoms;
    for (uint32_t i : rt.walk_q) {
      const uint32_t fcap = pq_filt_cap(efw[i], k, rerank);
      auto it = geoms.find(efw[i]);
      if (it == geoms.end()) {
        PqGeom sg;
        COLTT_TRY(pq_walk_geom(x, efw[i], false, fcap, sg));
        it = geoms.emplace(efw[i], sg).first;
      }
      add_walk(wl[it->second.variant != 0 ? 1 : 0], it->second, fcap, i);
    }
  }
  FiltExactPlan ep;
  COLTT_TRY(plan_filter_exact_batch(x, fl, rt.exact_q, k, who, ep));
  // the tables: [walks over the LDS hash][walks over the byte map][exact queries][tiles]
  const size_t nw0 = wl[0].q.size(), nw1 = wl[1].q.size(), nw = nw0 + nw1;
  std::vector<uint8_t> blob;
  uint8_t* d_desc;
  FiltOut o;
  COLTT_TRY(filter_upload(c, wl[0].q.data(), nw0 * sizeof(PqFiltQuery), wl[1].q.data(), nw1 * sizeof(PqFiltQuery), ep, nq, k, blob, d_desc, o));
  PqFiltQuery* d_pd = reinterpret_cast<PqFiltQuery*>(d_desc);
  RegionLease lease;
  bool nbr = false, nbr_known = false;
  auto byte_map_ready = [&](uint32_t want) -> int {   // one lease and one look at the neighbourhood blocks per call
    if (!lease.count) acquire_regions(x, want, lease);
    if (!nbr_known) { COLTT_TRY(ensure_pq_nbr(x, c->stream, &nbr)); nbr_known = true; }
    return COLTT_OK;
  };
  if (nw1) COLTT_TRY(byte_map_ready((uint32_t)std::min<size_t>(nw1, (size_t)256 * wl[1].per_cu)));
  // the queries: all of them prepared as Search prepares them, the walking ones' then gathered into [nw][dim] | [nw] behind the raw batch
  const size_t dim = x->dim;
  COLTT_TRY(c->w_qraw.reserve(nq * dim * 4 + nw * dim * 4 + nw * 4));
  COLTT_HIP(hipMemcpyAsync(c->w_qraw.p, queries, nq * dim * 4, hipMemcpyHostToDevice, c->stream));
  COLTT_TRY(c->w_misc.reserve(256));
  COLTT_TRY(c->h_out.reserve(256));
  uint8_t* misc = c->w_misc.as<uint8_t>();
  uint32_t* counter = reinterpret_cast<uint32_t*>(misc);
  unsigned long long* d_stats = reinterpret_cast<unsigned long long*>(misc + 16);
  COLTT_TRY(prep_queries_any(x, c, c->w_qraw.as<float>(), nq, reinterpret_cast<uint32_t*>(misc)));   // as the single call; clears the counters
  float* cq = c->w_qraw.as<float>() + nq * dim; float* cn = cq + nw * dim;
  COLTT_HIP(hipEventRecord(c->ev0, c->stream));
  const uint32_t lsh = pq_lut_shift(x);
  const size_t lut_q = ((size_t)x->pq_row << lsh) * 2;
  bool first_launch = true;
  // the n walks whose descriptors are pd[0..n) (position j of the compacted queries = pd[j]): groups of queries under the workspaces' 256 MiB, as pq_search_once
  auto run_walks = [&](const Launch& l, int variant, const PqFiltQuery* pd, size_t j0, size_t n) -> int {
    pq_gather_queries_kernel<<<(uint32_t)n, 64, 0, c->stream>>>(c->w_qeff.as<float>(), c->w_qn.as<float>(), pd, (uint32_t)dim, cq + j0 * dim, cn + j0);
    COLTT_HIP(hipGetLastError());
    PqGeom sg{};
    sg.variant = variant; sg.lds = l.lds; sg.ef_pad = l.ef_pad; sg.per_cu = l.per_cu;
    uint32_t grid = (uint32_t)std::min<size_t>(n, (size_t)256 * l.per_cu);
    if (variant != 0) grid = std::min(grid, lease.count);
    const size_t group = std::max<size_t>(1, std::min<size_t>({n, (256ull << 20) / lut_q, (256ull << 20) / ((size_t)l.ef_pad * 12), (size_t)32768}));
    COLTT_TRY(c->w_pack.reserve(group * lut_q + group * 4));
    COLTT_TRY(c->w_surv.reserve(group * l.ef_pad * 4)); COLTT_TRY(c->w_scnt.reserve(group * 4)); COLTT_TRY(c->w_keys.reserve(group * l.ef_pad * 8));
    for (size_t g0 = 0; g0 < n; g0 += group) {
      const size_t gn = std::min(group, n - g0);
      COLTT_TRY(pq_lut16_batch(c->stream, x->pq_cb.as<float>(), x->pq_shape, cq + (j0 + g0) * dim, gn, x->pq_row, lsh,
                               reinterpret_cast<uint32_t*>(c->w_pack.as<uint8_t>() + group * lut_q), c->w_pack.as<unsigned short>()));
      if (!first_launch) COLTT_HIP(hipMemsetAsync(counter, 0, 4, c->stream));
      first_launch = false;
      COLTT_TRY(launch_pq_walk(x, c, sg, nbr, (uint32_t)std::min<size_t>(grid, gn), lease.base, c->w_pack.as<unsigned short>(), (uint32_t)gn, k, rerank, counter,
                               c->w_surv.as<uint32_t>(), c->w_scnt.as<uint32_t>(), d_stats, nullptr, 0u, pd + g0));
      COLTT_TRY(launch_pq_rerank(x, c, sg, 0u, (uint32_t)gn, k, c->w_surv.as<uint32_t>(), c->w_scnt.as<uint32_t>(), c->w_keys.as<unsigned long long>(), o.oi, o.os, o.oc, pd + g0,
                                 cq + (j0 + g0) * dim, cn + j0 + g0));
    }
    return COLTT_OK;
  };
  if (nw0) COLTT_TRY(run_walks(wl[0], 0, d_pd, 0, nw0));
  if (nw1) COLTT_TRY(run_walks(wl[1], 2, d_pd + nw0, nw0, nw1));
  COLTT_TRY(run_filter_exact(x, c, ep, k, o, d_stats));
  unsigned long long h_stats[6];
  COLTT_HIP(hipMemcpyAsync(c->h_out.p, d_stats, 48, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));
  std::memcpy(h_stats, c->h_out.p, 48);
  if (nw0 && (h_stats[4] & 8ull) && !(h_stats[4] & ~8ull)) {   // some LDS-hash walks gave up (they added nothing to the sums): those queries over the byte map
    std::vector<PqFiltQuery> back(nw0);
    COLTT_HIP(hipMemcpy(back.data(), d_pd, nw0 * sizeof(PqFiltQuery), hipMemcpyDeviceToHost));
    Launch rl;
    std::map<uint32_t, PqGeom> geoms;
    for (const PqFiltQuery& q : back) {
      if (!(q.err & 8u)) continue;
      auto it = geoms.find(q.ef);
      if (it == geoms.end()) {
        PqGeom sg;
        COLTT_TRY(pq_walk_geom(x, q.ef, true, q.fcap, sg));
        it = geoms.emplace(q.ef, sg).first;
      }
      add_walk(rl, it->second, q.fcap, q.row);
    }
    const size_t nr = rl.q.size();   // <= nw0: their descriptors and gathered queries take the places of the LDS-hash launch's
    COLTT_TRY(byte_map_ready((uint32_t)std::min<size_t>(nr, (size_t)256 * rl.per_cu)));
    COLTT_HIP(hipMemcpyAsync(d_pd, rl.q.data(), nr * sizeof(PqFiltQuery), hipMemcpyHostToDevice, c->stream));
    COLTT_HIP(hipMemsetAsync(d_stats + 4, 0, 8, c->stream));
    COLTT_TRY(run_walks(rl, 2, d_pd, 0, nr));
    COLTT_HIP(hipMemcpyAsync(c->h_out.p, d_stats, 48, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipStreamSynchronize(c->stream));
    std::memcpy(h_stats, c->h_out.p, 48);
  }
  COLTT_TRY(filter_finish(x, c, who, o, nq, k, out_ids, out_scores, out_counts, d_stats, h_stats, true));
  // [3]: the members of R the walks handed to the re-rank, [5]: the rows the exact scan read
  st->n_dist = h_stats[0]; st->n_exp = h_stats[1]; st->n_hops = h_stats[2]; st->n_visit_resets = 0; st->n_exact_rows = h_stats[3] + h_stats[5];
  return COLTT_OK;
}

}  // namespace

extern "C" {

int coltt_hnsw_search_filtered(coltt_handle_t h, coltt_handle_t fh, const float* queries, size_t nq, uint32_t k, uint32_t ef_override, int mode,
                               uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_filter_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_search_filtered: unknown index handle");
  auto f = lookup<HnswFilter>(fh);
  if (!f) return fail(COLTT_E_NOT_FOUND, "hnsw_search_filtered: unknown filter handle");
  if (nq && (!queries || !out_ids || !out_scores || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_search_filtered: NULL buffer");
  if (f->index != h) return fail(COLTT_E_INVALID, "hnsw_search_filtered: the filter was built for another index");
  ReadLock g(x->rw);
  if (f->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_search_filtered: the filter is stale (the index was loaded since it was built)");
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return filter_search_common(x.get(), ctx.c, f.get(), queries, nq, k, ef_override, mode, out_ids, out_scores, out_counts, stats);
}

int coltt_hnsw_pq_search_filtered(coltt_handle_t h, coltt_handle_t fh, const float* queries, size_t nq, uint32_t k, uint32_t ef_override, uint32_t rerank, int mode,
                                  uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_filter_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_search_filtered: unknown index handle");
  {   // no codes attached: checked first, for every mode
    ReadLock g0(x->rw);
    if (!x->pq_on) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered: the index carries no product-quantiser codes (coltt_hnsw_pq_attach)");
  }
  auto f = lookup<HnswFilter>(fh);   // held until the call returns: a concurrent destroy only unregisters it
  if (!f) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_search_filtered: unknown filter handle");
  if (nq && (!queries || !out_ids || !out_scores || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered: NULL buffer");
  if (f->index != h) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered: the filter was built for another index");
  ReadLock g(x->rw);
  if (f->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered: the filter is stale (the index was loaded since it was built)");
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return pq_filter_search_common(x.get(), ctx.c, f.get(), queries, nq, k, ef_override, rerank, mode, out_ids, out_scores, out_counts, stats);
}

int coltt_hnsw_search_filtered_batch(coltt_handle_t h, const coltt_handle_t* filters, const float* queries, size_t nq, uint32_t k, uint32_t ef_override,
                                     int mode, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, int32_t* out_paths,
                                     coltt_hnsw_filter_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_search_filtered_batch: unknown index handle");
  if (nq && !filters) return fail(COLTT_E_INVALID, "hnsw_search_filtered_batch: NULL filters");
  if (nq && (!queries || !out_ids || !out_scores || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_search_filtered_batch: NULL buffer");
  ReadLock g(x->rw);
  // every handle is checked before anything is launched; each distinct filter is held until the call returns (a concurrent destroy
  // only unregisters it)
  std::unordered_map<coltt_handle_t, std::shared_ptr<HnswFilter>> held;
  std::vector<HnswFilter*> fl(nq);
  for (size_t i = 0; i < nq; i++) {
    auto it = held.find(filters[i]);
    if (it == held.end()) {
      auto f = lookup<HnswFilter>(filters[i]);
      if (!f) return fail(COLTT_E_NOT_FOUND, "hnsw_search_filtered_batch: unknown filter handle at position %zu", i);
      if (f->index != h) return fail(COLTT_E_INVALID, "hnsw_search_filtered_batch: the filter at position %zu was built for another index", i);
      if (f->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_search_filtered_batch: the filter at position %zu is stale (the index was loaded since it was built)", i);
      it = held.emplace(filters[i], std::move(f)).first;
    }
    fl[i] = it->second.get();
  }
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return filter_batch_common(x.get(), ctx.c, fl, queries, nq, k, ef_override, mode, out_ids, out_scores, out_counts, out_paths, stats);
}

int coltt_hnsw_pq_search_filtered_batch(coltt_handle_t h, const coltt_handle_t* filters, const float* queries, size_t nq, uint32_t k, uint32_t ef_override,
                                        uint32_t rerank, int mode, uint64_t* out_ids, float* out_scores, uint32_t* out_counts, int32_t* out_paths,
                                        coltt_hnsw_filter_stats* stats) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_search_filtered_batch: unknown index handle");
  ReadLock g(x->rw);
  // no codes attached: checked first, for every mode
  if (!x->pq_on) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered_batch: the index carries no product-quantiser codes (coltt_hnsw_pq_attach)");
  if (nq && !filters) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered_batch: NULL filters");
  if (nq && (!queries || !out_ids || !out_scores || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered_batch: NULL buffer");
  // every handle is checked before anything is launched; each distinct filter is held until the call returns (a concurrent destroy
  // only unregisters it)
  std::unordered_map<coltt_handle_t, std::shared_ptr<HnswFilter>> held;
  std::vector<HnswFilter*> fl(nq);
  for (size_t i = 0; i < nq; i++) {
    auto it = held.find(filters[i]);
    if (it == held.end()) {
      auto f = lookup<HnswFilter>(filters[i]);
      if (!f) return fail(COLTT_E_NOT_FOUND, "hnsw_pq_search_filtered_batch: unknown filter handle at position %zu", i);
      if (f->index != h) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered_batch: the filter at position %zu was built for another index", i);
      if (f->gen != x->gen) return fail(COLTT_E_INVALID, "hnsw_pq_search_filtered_batch: the filter at position %zu is stale (the index was loaded since it was built)", i);
      it = held.emplace(filters[i], std::move(f)).first;
    }
    fl[i] = it->second.get();
  }
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  return pq_filter_batch_common(x.get(), ctx.c, fl, queries, nq, k, ef_override, rerank, mode, out_ids, out_scores, out_counts, out_paths, stats);
}

}  // extern "C"
