// hnsw_search2.hip — the level-0 walks of hnsw_walk2.hpp (delta result set, adjacency-carried norms, Bloom filter; the eight-lane distance
// core and its certified row filter): their launcher, the row filter's counters, shadow read-back and probe.
#include <algorithm>
#include <cmath>

#include "hnsw_index.hpp"
#include "hnsw_kernels.hpp"   // hnsw_search2_kernel, hnsw_search2_rowfilter_kernel, hnsw_row_filter_probe_kernel

using namespace coltt;
using namespace coltt::dev;
using namespace coltt::kern;
using namespace coltt::hnsw;

namespace {

// What the prologue of a row-filter launch does unless COLTT_DESCENT_NT / COLTT_ROW_FILTER_UPPER say otherwise.  Measured on 10 M x 768, ef 128, 10 000 queries
// per launch, four sides alternating in one process (tools/descent_filter_ab.py; profiles/r12a_descent_filter.md): cacheable descent loads 9.06 -> 8.76 ms
// (+3.4 %); the filtered descent on top of them 8.80 ms — it rejects 90 % of the 116 evaluations above level 0 and asks for a third of the bytes, but with the
// top of the graph served from cache those bytes were no longer HBM's, and a hop now waits for two dependent phases instead of one.
constexpr bool DESCENT_NT_DEFAULT = false;         // the entrypoint's and the descent's rows are loaded cacheable: every query of a launch reads them
constexpr bool ROW_FILTER_UPPER_DEFAULT = false;   // the greedy descent evaluates every listed neighbour exactly

// hnsw_walk2.hpp kernels: the shipped variant (and its Bloom-less twin for geometries whose LDS has no room for the filter).
template <int METRIC, int QUANT>
int launch_search2_for(Hnsw* x, HCtx* c, const SearchGeom& sg, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                   uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  typedef void (*kern_t)(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*,
                         uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*);
  typedef void (*fkern_t)(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*,
                          uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*, uint32_t);   // the row-filter twins: + how the prologue descends
  kern_t kern = nullptr;
  fkern_t fkern = nullptr;
  const bool nt = rows_nt(x);   // non-temporal row loads (eight-lane kernels): see exact.hpp: row_ld
  bool flt = false;             // the row-filter twin (row_filter_on)
  bool v16 = false;             // ... over the 16-bit visited set (search_geom: vis16)
#define COLTT_W2(V, PROF, OPT) case V: kern = hnsw_search2_kernel<METRIC, QUANT, PROF, OPT>; break;
  if (sg.w2_lds) {
    switch (sg.w2) {
      case 4:
        kern = hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_LDS, 4, VIS_LDS>;
        if constexpr (QUANT != Q_F8) {
          if (sg.ev8) kern = nt ? hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_LDS, 4, VIS_LDS, false, true, false, true> : hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_LDS, 4, VIS_LDS, false, true>;
          else if (x->r8) kern = hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_LDS, 4, VIS_LDS, false, false, true>;   // the pair-owned core over the line-transposed rows
        }
        if constexpr (METRIC == M_COS && QUANT == Q_NONE) {   // the row-filter twin of the eight-lane instance just chosen
          if (sg.ev8 && row_filter_on(x, false)) {
            const int fb = row_filter_bits(x);
            if (fb == ROW_FILTER_8I && sg.qd8i && sg.vis16) { fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS16, true, ROW_FILTER_8I> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS16, false, ROW_FILTER_8I>; v16 = true; }
            else if (fb == ROW_FILTER_8I && sg.qd8i) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS, true, ROW_FILTER_8I> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS, false, ROW_FILTER_8I>;   // (sg.qd8i: search_geom made room for the digit planes)
            else if (fb == 8 || fb == ROW_FILTER_8I) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS, true, 8> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS, false, 8>;
            else fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS, true> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_LDS, 4, VIS_LDS, false>;
            flt = true;
          }
        }
        break;   // (adjacency prefetch for f32 rows in small batches: measured, no gain — 1 M x 128, ef 20, one query 105 vs 111 us)
      default: break;
    }
  } else
  {
    switch (sg.w2) {
      COLTT_W2(6, PROF_SEARCH_HBM, 6) COLTT_W2(7, PROF_SEARCH_HBM, 7)
      default: break;
    }
    if constexpr (METRIC == M_COS && QUANT == Q_NONE) {   // W2_ADJN: both shipped HBM-visited variants carry the neighbours' norms
      if (sg.ev8 && row_filter_on(x, true) && (sg.w2 == 6 || sg.w2 == 7)) flt = true;
      if (flt && sg.w2 == 6) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 6, VIS_HBM, true> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 6, VIS_HBM, false>;
      if (flt && sg.w2 == 7) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 7, VIS_HBM, true> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 7, VIS_HBM, false>;
      const int fb = flt ? row_filter_bits(x) : 0;
      if (fb == ROW_FILTER_8I && sg.qd8i) {
        if (sg.w2 == 6) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 6, VIS_HBM, true, ROW_FILTER_8I> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 6, VIS_HBM, false, ROW_FILTER_8I>;
        if (sg.w2 == 7) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 7, VIS_HBM, true, ROW_FILTER_8I> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 7, VIS_HBM, false, ROW_FILTER_8I>;
      } else if (fb == 8 || fb == ROW_FILTER_8I) {
        if (sg.w2 == 6) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 6, VIS_HBM, true, 8> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 6, VIS_HBM, false, 8>;
        if (sg.w2 == 7) fkern = nt ? hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 7, VIS_HBM, true, 8> : hnsw_search2_rowfilter_kernel<PROF_SEARCH_HBM, 7, VIS_HBM, false, 8>;
      }
    }
    if constexpr (QUANT != Q_F8) { if (!flt) {
      if (sg.ev8 && sg.w2 == 6) kern = nt ? hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_HBM, 6, VIS_HBM, false, true, false, true> : hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_HBM, 6, VIS_HBM, false, true>;
      if (sg.ev8 && sg.w2 == 7) kern = nt ? hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_HBM, 7, VIS_HBM, false, true, false, true> : hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_HBM, 7, VIS_HBM, false, true>;
      if (!sg.ev8 && x->r8 && sg.w2 == 6) kern = hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_HBM, 6, VIS_HBM, false, false, true>;
      if (!sg.ev8 && x->r8 && sg.w2 == 7) kern = hnsw_search2_kernel<METRIC, QUANT, PROF_SEARCH_HBM, 7, VIS_HBM, false, false, true>;
    } }
  }
#undef COLTT_W2
  uint32_t upper = 0;
  if (flt && fkern) {   // (the binary16 kind has no per-slot (scale, error norm): its descent stays exact)
    const Policy p = policy();
    const int fb = row_filter_bits(x);
    if ((fb == 8 || fb == ROW_FILTER_8I) && (p.row_filter_upper >= 0 ? p.row_filter_upper != 0 : ROW_FILTER_UPPER_DEFAULT)) upper |= ROWF_UPPER_FILTER;
    if (nt && (p.descent_nt >= 0 ? p.descent_nt == 0 : !DESCENT_NT_DEFAULT)) upper |= ROWF_UPPER_CACHED;
  }
  c->upper_launch = (upper & ROWF_UPPER_FILTER) != 0;
  if (!kern && !fkern) return fail(COLTT_E_UNSUPPORTED, "hnsw_search: walk variant %d is not compiled into this build (COLTT_WALK2)", sg.w2);
  if (x->r8 && !sg.ev8 && !(sg.w2_lds ? sg.w2 == 4 : (sg.w2 == 6 || sg.w2 == 7)))
    return fail(COLTT_E_UNSUPPORTED, "hnsw_search: walk variant %d has no instance for line-transposed rows (create the index with COLTT_ROWS8=0 for this experiment)", sg.w2);
  if (sg.ev8) x->ev8_launches.fetch_add(1);
  if (sg.vis16 && !v16) return fail(COLTT_E_DEVICE, "hnsw_search: the launch's LDS was sized for the 16-bit visited set, but the walk chosen does not use it");
  c->flt_launch = flt; c->v16_launch = v16;
  const void* const kp = fkern ? reinterpret_cast<const void*>(fkern) : reinterpret_cast<const void*>(kern);
  COLTT_HIP(hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sg.lds));
  static const bool dbg_occ = [] { const char* e = getenv("COLTT_DEBUG_OCCUPANCY"); return e && *e == '1'; }();   // diagnostics: the waves the runtime keeps resident per CU at this launch's LDS
  if (dbg_occ || v16) {   // (the 16-bit launches report it through coltt_hnsw_visited_stats: asked once per (kernel, LDS) and context)
    if (c->occ_kern != kp || c->occ_lds != sg.lds) {
      int per_cu = 0;
      COLTT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kp, 64, sg.lds));
      c->occ_kern = kp; c->occ_lds = sg.lds; c->occ_per_cu = per_cu;
    }
    if (dbg_occ) fprintf(stderr, "[occupancy] walk variant %d%s filter %d (8i planes %d) visited set %s: %zu B of LDS per wave, %d waves resident per CU, grid %u\n", sg.w2, sg.w2_lds ? " (LDS hash)" : "", flt ? 1 : 0, sg.qd8i ? 1 : 0,
                         v16 ? "16-bit LDS table" : (sg.w2_lds ? "32-bit LDS table" : "HBM byte map"), sg.lds, c->occ_per_cu, grid);
  }
  const uint32_t vis_arg = sg.w2_lds ? (v16 ? ((sg.v16_limit << 8) | sg.v16_bits) : sg.hcap) : sg.bloom_words;
  if (fkern) fkern<<<grid, 64, sg.lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                                    k, sg.ef, sg.ef_pad, vis_arg, counter, oi, os, oc, stats,
                                                    x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                                    x->w_vepoch.as<uint32_t>() + region_base, upper);
  else kern<<<grid, 64, sg.lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                             k, sg.ef, sg.ef_pad, vis_arg, counter, oi, os, oc, stats,
                                             x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                             x->w_vepoch.as<uint32_t>() + region_base);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

}  // namespace

namespace coltt {
namespace hnsw {

// the launcher for the index's metric and row format
int launch_search2(Hnsw* x, HCtx* c, const SearchGeom& sg, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                   uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  int rc;
#define COLTT_LS_ARGS x, c, sg, grid, region_base, nq, k, counter, oi, os, oc, stats
#define COLTT_LS(Q) rc = x->metric == COLTT_COSINE ? launch_search2_for<M_COS, Q>(COLTT_LS_ARGS) : launch_search2_for<M_L2, Q>(COLTT_LS_ARGS)
  COLTT_DISPATCH_QUANT(x->quant, COLTT_LS)
#undef COLTT_LS
#undef COLTT_LS_ARGS
  return rc;
}

}  // namespace hnsw
}  // namespace coltt

extern "C" {

int coltt_hnsw_row_filter_stats(coltt_handle_t h, uint64_t* out_rejected, uint64_t* out_f32_rows, uint64_t* out_shadow_rows, uint64_t* out_launches, int32_t* out_has_shadow) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_row_filter_stats: unknown handle");
  ReadLock g(x->rw);
  if (out_rejected) *out_rejected = x->flt_rejected.load();
  if (out_f32_rows) *out_f32_rows = x->flt_f32_rows.load();
  if (out_launches) *out_launches = x->flt_launches.load();
  if (out_shadow_rows) *out_shadow_rows = x->flt_shadow_rows.load();
  if (out_has_shadow) *out_has_shadow = (x->has_shadow16() ? 16 : 0) | (x->has_shadow8() ? 8 : 0);   // non-zero: some shadow is kept; bit 3 / bit 4: which
  return COLTT_OK;
}

int coltt_hnsw_row_filter_stats_ex(coltt_handle_t h, uint64_t* out_upper_shadow_rows, uint64_t* out_upper_rejected, uint64_t* out_upper_f32_rows, uint64_t* out_upper_launches) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_row_filter_stats_ex: unknown handle");
  ReadLock g(x->rw);
  if (out_upper_shadow_rows) *out_upper_shadow_rows = x->flt_up_shadow_rows.load();
  if (out_upper_rejected) *out_upper_rejected = x->flt_up_rejected.load();
  if (out_upper_f32_rows) *out_upper_f32_rows = x->flt_up_f32_rows.load();
  if (out_upper_launches) *out_upper_launches = x->flt_up_launches.load();
  return COLTT_OK;
}

int coltt_hnsw_fetch_shadow8(coltt_handle_t h, uint64_t first_slot, uint64_t n, int8_t* out_codes, float* out_meta, float* out_adj_meta) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_fetch_shadow8: unknown handle");
  ReadLock g(x->rw);
  if (!x->has_shadow8()) return fail(COLTT_E_UNSUPPORTED, "hnsw_fetch_shadow8: the index keeps no 8-bit shadow");
  if (first_slot > x->n || n > x->n - first_slot) return fail(COLTT_E_INVALID, "hnsw_fetch_shadow8: range outside [0,%llu)", (unsigned long long)x->n);
  if (n == 0) return COLTT_OK;
  COLTT_DEVICE(x->device);
  const size_t dim = x->dim, w = x->cfg.m_max0;
  if (out_codes) {   // rows8.hpp's layout -> natural element order, on the host (a read-back for tests and tools)
    std::vector<uint8_t> raw(n * dim);
    COLTT_HIP(hipMemcpy(raw.data(), x->rows_b.as<uint8_t>() + first_slot * dim, n * dim, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < n; i++)
      for (size_t e = 0; e < dim; e++) {
        const size_t r = e & 7, step = e >> 3, l = step >> 2, t_ = step & 3;
        out_codes[i * dim + e] = (int8_t)raw[i * dim + ((l >> 2) * 8 + r) * 16 + (l & 3) * 4 + t_];
      }
  }
  if (out_meta) COLTT_HIP(hipMemcpy(out_meta, x->rows_m.as<uint8_t>() + first_slot * 8, n * 8, hipMemcpyDeviceToHost));
  if (out_adj_meta) COLTT_HIP(hipMemcpy(out_adj_meta, x->adj0_m.as<uint8_t>() + first_slot * w * 8, n * w * 8, hipMemcpyDeviceToHost));
  return COLTT_OK;
}

int coltt_hnsw_row_filter_probe(coltt_handle_t h, const float* queries, size_t nq, const uint32_t* slots, const float* lower_bound, int bits, int nt,
                                int full_at_pop, float* out_r, float* out_qnorm, float* out_rnorm, uint32_t* out_counts) {
  if (bits != 8 && bits != 16) return fail(COLTT_E_INVALID, "hnsw_row_filter_probe: bits must be 8 or 16");
  return coltt_hnsw_row_filter_probe_ex(h, queries, nq, slots, lower_bound, bits, nt, full_at_pop, out_r, out_qnorm, out_rnorm, out_counts, nullptr, nullptr);
}

int coltt_hnsw_row_filter_probe_ex(coltt_handle_t h, const float* queries, size_t nq, const uint32_t* slots, const float* lower_bound, int bits, int nt,
                                   int full_at_pop, float* out_r, float* out_qnorm, float* out_rnorm, uint32_t* out_counts, int64_t* out_isum, float* out_qte) {
  auto x = lookup<Hnsw>(h);
  if (!x) return fail(COLTT_E_NOT_FOUND, "hnsw_row_filter_probe: unknown handle");
  if (bits != 8 && bits != 16 && bits != ROW_FILTER_8I) return fail(COLTT_E_INVALID, "hnsw_row_filter_probe: bits must be 8, 16 or 80 (8i)");
  const bool k8i = bits == ROW_FILTER_8I;
  if (nq && (!queries || !slots || !lower_bound || !out_r || !out_qnorm || !out_rnorm || !out_counts)) return fail(COLTT_E_INVALID, "hnsw_row_filter_probe: NULL buffer");
  if (nq > 0x7fffffffu / 32) return fail(COLTT_E_INVALID, "hnsw_row_filter_probe: too many queries");
  ReadLock g(x->rw);
  if (!x->r8 || (bits != 16 ? !x->has_shadow8() : !x->has_shadow16())) return fail(COLTT_E_UNSUPPORTED, "hnsw_row_filter_probe: the index keeps no %d-bit shadow", bits == 16 ? 16 : 8);
  if (nq == 0) return COLTT_OK;
  for (size_t i = 0; i < nq * 32; i++)
    if (slots[i] != NBR_NONE && slots[i] >= x->n) return fail(COLTT_E_INVALID, "hnsw_row_filter_probe: slot %u outside [0,%llu)", slots[i], (unsigned long long)x->n);
  COLTT_DEVICE(x->device);
  CtxLease<HCtx> ctx(x->pool);
  if (!ctx.c) return COLTT_E_DEVICE;
  HCtx* c = ctx.c;
  const size_t dim = x->dim;
  COLTT_TRY(c->w_qraw.reserve(nq * dim * 4));
  COLTT_TRY(c->w_misc.reserve(256));
  // one block of inputs and outputs: slots [nq][32] | lower_bound [nq] | out_r [nq][32] | out_rnorm [nq][32] | out_counts [nq][3]
  // (8i: | pad to 8 bytes | out_isum [nq][32] i64 | out_qte [nq][2])
  COLTT_TRY(c->w_out_ids.reserve(nq * (32 * 3 + 1 + 3) * 4 + 8 + nq * (32 * 8 + 2 * 4)));
  uint32_t* d_slots = c->w_out_ids.as<uint32_t>();
  float* d_lb = reinterpret_cast<float*>(d_slots + nq * 32);
  float* d_r = d_lb + nq; float* d_rn = d_r + nq * 32;
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(d_rn + nq * 32);
  COLTT_HIP(hipMemcpyAsync(c->w_qraw.p, queries, nq * dim * 4, hipMemcpyHostToDevice, c->stream));
  COLTT_HIP(hipMemcpyAsync(d_slots, slots, nq * 32 * 4, hipMemcpyHostToDevice, c->stream));
  COLTT_HIP(hipMemcpyAsync(d_lb, lower_bound, nq * 4, hipMemcpyHostToDevice, c->stream));
  COLTT_TRY(prep_queries_any(x.get(), c, c->w_qraw.as<float>(), nq, c->w_misc.as<uint32_t>()));   // Normalize the queries as Search does
  long long* d_isum = reinterpret_cast<long long*>((reinterpret_cast<uintptr_t>(d_cnt + nq * 3) + 7) & ~(uintptr_t)7);
  float* d_qte = reinterpret_cast<float*>(d_isum + nq * 32);
  if (k8i) COLTT_HIP(hipMemsetAsync(d_isum, 0, nq * (32 * 8 + 2 * 4), c->stream));
  const size_t lds = ((dim * 4 + 15) & ~(size_t)15) + 96 * 4 + (k8i ? dim * 2 : 0);   // 8i: the digit planes behind the scratch
  auto kern = k8i ? (nt ? hnsw_row_filter_probe_kernel<true, ROW_FILTER_8I> : hnsw_row_filter_probe_kernel<false, ROW_FILTER_8I>)
            : bits == 8 ? (nt ? hnsw_row_filter_probe_kernel<true, 8> : hnsw_row_filter_probe_kernel<false, 8>)
                        : (nt ? hnsw_row_filter_probe_kernel<true, 16> : hnsw_row_filter_probe_kernel<false, 16>);
  COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<(uint32_t)nq, 64, lds, c->stream>>>(x->view(), c->w_qeff.as<float>(), c->w_qn.as<float>(), d_slots, d_lb, full_at_pop ? 1 : 0, d_r, d_rn, d_cnt,
                                             k8i ? d_isum : nullptr, k8i ? d_qte : nullptr);
  COLTT_HIP(hipGetLastError());
  if (k8i && out_isum) COLTT_HIP(hipMemcpyAsync(out_isum, d_isum, nq * 32 * 8, hipMemcpyDeviceToHost, c->stream));
  if (k8i && out_qte) COLTT_HIP(hipMemcpyAsync(out_qte, d_qte, nq * 2 * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipMemcpyAsync(out_r, d_r, nq * 32 * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipMemcpyAsync(out_rnorm, d_rn, nq * 32 * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipMemcpyAsync(out_counts, d_cnt, nq * 3 * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipMemcpyAsync(out_qnorm, c->w_qn.p, nq * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));
  return COLTT_OK;
}

}  // extern "C"
