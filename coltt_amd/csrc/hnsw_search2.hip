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

typedef void (*kern_t)(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*,
                       uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*);
typedef void (*fkern_t)(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*,
                        uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*, uint32_t);   // the row-filter twins: + how the prologue descends

// The instances of one shipped walk (profile, variant, visited set), each named once.  The distance core: eight lanes per row (with non-temporal row loads
// or not: exact.hpp: row_ld), the pair-owned core over line-transposed rows, the pair-owned core over natural rows.
template <int METRIC, int QUANT, int PROF, int OPT, int VIS>
kern_t walk_instance(const SearchPlan& sp) {
  if constexpr (QUANT != Q_F8) {
    if (sp.ev8) return sp.nt ? hnsw_search2_kernel<METRIC, QUANT, PROF, OPT, VIS, false, true, false, true> : hnsw_search2_kernel<METRIC, QUANT, PROF, OPT, VIS, false, true>;
    if (sp.r8) return hnsw_search2_kernel<METRIC, QUANT, PROF, OPT, VIS, false, false, true>;
  }
  return hnsw_search2_kernel<METRIC, QUANT, PROF, OPT, VIS>;
}
// ... and its row-filter twins (f32 cosine, eight-lane core) by the shadow they read; the 16-bit visited set serves the filter over the quantised query only.
// (adjacency prefetch for f32 rows in small batches: measured, no gain — 1 M x 128, ef 20, one query 105 vs 111 us)
template <int PROF, int OPT, int VIS>
fkern_t filter_instance(const SearchPlan& sp) {
  if (sp.filter == ROW_FILTER_8I) return sp.nt ? hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, true, ROW_FILTER_8I> : hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, false, ROW_FILTER_8I>;
  if constexpr (VIS != VIS_LDS16) {
    if (sp.filter == 8) return sp.nt ? hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, true, 8> : hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, false, 8>;
    if (sp.filter == 16) return sp.nt ? hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, true> : hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, false>;
  }
  return nullptr;
}

// hnsw_walk2.hpp kernels: the launch of one plan (hnsw.hip: plan_search decided everything; a plan it passed has an instance here).
template <int METRIC, int QUANT>
int launch_search2_for(Hnsw* x, HCtx* c, const SearchPlan& sp, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                   uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  kern_t kern = nullptr;
  fkern_t fkern = nullptr;
  const bool v16 = sp.vis_kind == 16;
#define COLTT_W2(PROF, OPT, VIS)                                                                                                   \
  do {                                                                                                                           \
    if constexpr (METRIC == M_COS && QUANT == Q_NONE) { if (sp.filter) fkern = filter_instance<PROF, OPT, VIS>(sp); }             \
    if (!sp.filter) kern = walk_instance<METRIC, QUANT, PROF, OPT, VIS>(sp);                                                    \
  } while (0)
  switch (sp.vis_kind << 4 | sp.w2) {
    case 32 << 4 | 4: COLTT_W2(PROF_SEARCH_LDS, 4, VIS_LDS); break;
    case 16 << 4 | 4: if constexpr (METRIC == M_COS && QUANT == Q_NONE) fkern = filter_instance<PROF_SEARCH_LDS, 4, VIS_LDS16>(sp); break;
    case 0 << 4 | 6: COLTT_W2(PROF_SEARCH_HBM, 6, VIS_HBM); break;   // W2_ADJN: both shipped HBM-visited variants carry the neighbours' norms
    case 0 << 4 | 7: COLTT_W2(PROF_SEARCH_HBM, 7, VIS_HBM); break;
    default: break;
  }
#undef COLTT_W2
  if (!kern && !fkern) return fail(COLTT_E_DEVICE, "hnsw_search: no kernel instance for the plan (walk variant %d)", sp.w2);   // (walk2_shipped names the same set)
  const void* const kp = fkern ? reinterpret_cast<const void*>(fkern) : reinterpret_cast<const void*>(kern);
  COLTT_HIP(hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sp.lds));
  static const bool dbg_occ = [] { const char* e = getenv("COLTT_DEBUG_OCCUPANCY"); return e && *e == '1'; }();   // diagnostics: the waves the runtime keeps resident per CU at this launch's LDS
  if (dbg_occ || v16) {   // (the 16-bit launches report it through coltt_hnsw_visited_stats: asked once per (kernel, LDS) and context)
    if (c->occ_kern != kp || c->occ_lds != sp.lds) {
      int per_cu = 0;
      COLTT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kp, 64, sp.lds));
      c->occ_kern = kp; c->occ_lds = sp.lds; c->occ_per_cu = per_cu;
    }
    if (dbg_occ) fprintf(stderr, "[occupancy] walk variant %d%s filter %d (8i planes %d) visited set %s: %zu B of LDS per wave, %d waves resident per CU, grid %u\n", sp.w2, sp.vis_kind ? " (LDS hash)" : "", sp.filter ? 1 : 0, sp.filter == ROW_FILTER_8I ? 1 : 0,
                         v16 ? "16-bit LDS table" : (sp.vis_kind ? "32-bit LDS table" : "HBM byte map"), (size_t)sp.lds, c->occ_per_cu, grid);
  }
  const uint32_t vis_arg = sp.vis_kind ? (v16 ? ((sp.v16_limit << 8) | sp.v16_bits) : sp.hcap) : sp.bloom_words;
  if (fkern) fkern<<<grid, 64, sp.lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                                    k, sp.ef, sp.ef_pad, vis_arg, counter, oi, os, oc, stats,
                                                    x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                                    x->w_vepoch.as<uint32_t>() + region_base, sp.upper);
  else kern<<<grid, 64, sp.lds, c->stream>>>(x->view(), x->entry, x->entry_level, c->w_qeff.as<float>(), c->w_qn.as<float>(), nq,
                                             k, sp.ef, sp.ef_pad, vis_arg, counter, oi, os, oc, stats,
                                             x->w_visg.as<uint8_t>() + (size_t)region_base * x->vis_stride, (size_t)x->vis_stride,
                                             x->w_vepoch.as<uint32_t>() + region_base);
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

}  // namespace

namespace coltt {
namespace hnsw {

// the launcher for the index's metric and row format
int launch_search2(Hnsw* x, HCtx* c, const SearchPlan& sp, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                   uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats) {
  int rc;
#define COLTT_LS_ARGS x, c, sp, grid, region_base, nq, k, counter, oi, os, oc, stats
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
