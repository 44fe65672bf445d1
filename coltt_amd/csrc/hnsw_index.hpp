// hnsw_index.hpp — the state of one HNSW index on the GPU and what its translation units share: the index object and its per-call search
// context, the geometry records the launchers pass around, the filter object, and the declarations of the host functions that cross a file
// boundary.  No kernels and no kernel headers.
//   hnsw.hip          life cycle (create, load, commit, export, compact), builder, search policy and geometry, the one-wave walk and the
//                     latency kernel, the walk over product-quantiser codes, filter objects and expressions, attribute columns
//   hnsw_search2.hip  the large-ef / eight-lane walks of hnsw_walk2.hpp, the row filter's counters, read-back and probe
//   hnsw_filter.hip   the filtered drivers (allow-list walk, exact scan) and their entry points
// A named namespace: lookup<Hnsw>(h) must see one type in every translation unit.
#pragma once
#include <algorithm>
#include <atomic>

#include "common.hpp"
#include "hnsw_dev.hpp"

namespace coltt {
namespace hnsw {
using namespace coltt::dev;

// Per-call search context: searches hold the index lock shared and run concurrently, each on its own stream and workspaces.
struct HCtx {
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  DevBuf w_qraw, w_qeff, w_qn, w_out_ids, w_out_sc, w_out_cnt, w_misc, w_pack;
  DevBuf w_surv, w_scnt, w_keys;   // product-quantised walk: survivors (slots), their count, their exact keys
  DevBuf w_mbox;                   // latency kernel: the walking workgroups' hint mailboxes (hnsw_lat.hpp: cache-warming helper workgroups)
  DevBuf w_fdesc;                  // filtered batch: the walks' per-query descriptors, the exact path's queries and tiles
  PinnedBuf h_in, h_out;   // small calls: see PinnedBuf
  const void* occ_kern = nullptr; size_t occ_lds = 0; int occ_per_cu = 0;   // the runtime's occupancy answer for the last (kernel, LDS) asked about
  int init() {  // the caller has selected the index's device
    COLTT_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    COLTT_HIP(hipEventCreate(&ev0));
    COLTT_HIP(hipEventCreate(&ev1));
    return COLTT_OK;
  }
  ~HCtx() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct Hnsw : Object {
  uint32_t dim = 0; int metric = 0, quant = 0; size_t stride = 0;
  coltt_hnsw_cfg cfg{};
  uint64_t n = 0 /*slots*/, live = 0, cap = 0, n_upper = 0, ucap = 0;
  int32_t entry = -1, entry_level = 0;
  bool any_deleted = false;
  DevBuf rows, norms, ids, adj0, adj0_d, adj0_n, upper_off, adjU, adjU_d, del_bits;
  // rows8.hpp (round 5: ONE row array).  r8: `rows` itself is stored LINE-TRANSPOSED — every 128-byte line rewritten so that its 16-byte chunk r
  // holds residue r's consecutive AVX steps — for the shapes the eight-lanes-per-row core covers (f32 / 2-byte rows whose byte length is a
  // multiple of 128, dim >= 256 unless COLTT_ROWS8=2; never with COLTT_ROWS8=0).  Every reader knows the layout: the eight-lane core reads whole
  // lines, the pair-owned core reads its four chunks of a line (exact.hpp: pair_distance_r8 — same values, same order, same bits), the builder,
  // Commit / Get / fetch and the quantiser's Encode un-permute element indices (r8_index).  Writers go through a natural-order staging block.
  bool r8 = false;
  DevBuf w_stage;   // natural-order rows of the batch being ingested (r8 indexes)
  std::atomic<uint64_t> ev8_launches{0};   // search launches whose level-0 distances came from rows8
  // The level-0 row filter (row_filter.hpp, rows8.hpp): rows_h = one binary16 value per stored element of a line-transposed f32 cosine index, dim * 2 bytes
  // per slot — DERIVED data, written wherever `rows` is written (prep_rows_any), grown with it, never part of a stream or a read-back.  shadow: the index
  // keeps one (decided at create: shape, COLTT_ROW_SHADOW; dropped for good when its allocation fails — the index then works without the filter).
  bool shadow = false;
  DevBuf rows_h;
  // The 8-bit shadow (row_filter8.hpp, rows8.hpp): rows_b = one code byte per stored element, rows_m = (scale, error norm) per slot, adj0_m = rows_m of every
  // level-0 edge's target, written wherever adj0_n is.  Derived data like rows_h: written and grown with `rows`, dropped for good when an allocation fails.
  // Which of the two an index keeps is decided at create (COLTT_ROW_SHADOW_BITS; default: this one).
  bool shadow8 = false;
  DevBuf rows_b, rows_m, adj0_m;
  void drop_shadow8() {
    shadow8 = false;
    for (DevBuf* b : {&rows_b, &rows_m, &adj0_m}) if (b->p) { (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    (void)hipGetLastError();
  }
  bool has_shadow8() const { return shadow8 && rows_b.p && rows_m.p && adj0_m.p; }
  bool has_shadow16() const { return shadow && rows_h.p; }
  std::atomic<uint64_t> flt_up_launches{0}, flt_up_shadow_rows{0}, flt_up_rejected{0}, flt_up_f32_rows{0};   // the same for the filtered descent (levels above 0): launches that ran it; shadow rows, rejected evaluations, f32 rows up there
  std::atomic<uint64_t> flt_launches{0}, flt_rejected{0}, flt_f32_rows{0}, flt_shadow_rows{0};   // filtered launches whose call completed; evaluations the filter rejected; f32 rows / shadow rows they read at level 0
  // the visited set of the last search launch (coltt_hnsw_visited_stats): 0 HBM byte map, 32 the LDS hash of 32-bit slots, 16 the 16-bit one (vis16.hpp); the
  // traversals that launch kept resident per CU, its grid and, if it ran on the 16-bit table, the fullest stash and the most vertices one of its traversals
  // visited; v16_launches: launches on the 16-bit table so far (one that overflowed and was re-run included)
  std::atomic<int32_t> last_vis_kind{-1}; std::atomic<uint32_t> last_per_cu{0}, last_grid{0};
  std::atomic<uint64_t> v16_launches{0}, last_stash_max{0}, last_visited_max{0};
  void drop_shadow() { shadow = false; if (rows_h.p) { (void)hipFree(rows_h.p); rows_h.p = nullptr; rows_h.cap = 0; } (void)hipGetLastError(); }
  // hnsw_pq.hpp: a snapshot of a trained product quantiser and one row-major code per slot (derived data, maintained like rows8:
  // writers encode the slots they added before they release the exclusive lock)
  bool pq_on = false; PqShape pq_shape; uint32_t pq_row = 0 /* bytes per code row: m rounded up to 16 */; uint64_t pq_done = 0;
  DevBuf pq_cb, pq_codes, pq_stage;
  // Neighbourhood blocks of the product-quantised walk (hnsw_pq.hpp: AdcEval<.., NBR>): pq_nbr[slot][p][pq_row] = pq_codes[adj0[slot][p]] (zeros for an
  // empty position) — derived from the level-0 rows and the codes.  Built whole by the first product-quantised search that finds them stale (searches hold
  // the lock shared and settle the build among themselves under pq_nbr_mu), then MAINTAINED by the writers like adj0_n: Insert / InsertBatchDevice / Remove
  // raise pq_nbr_stale before their first device write and, if the blocks were current, re-gather the blocks of exactly the level-0 rows they rewrote
  // (PqNbrPatch below) and lower it again before they release the exclusive lock — a call that does not reach its end leaves them stale.  Load / BulkLoad /
  // PqAttach (everything renumbered or re-coded) and a grown slot capacity leave them stale: the next walk that reads them rebuilds.
  DevBuf pq_nbr; bool pq_nbr_ok = false; std::atomic<bool> pq_nbr_stale{true}; std::mutex pq_nbr_mu;
  bool pq_nbr_built = false;   // pq_nbr has held a whole build (a stale array is then state 2, not 0)
  DevBuf pq_dirty;             // [0] = level-0 rows the link kernels of the mutation in flight rewrote, [2 ..] their slots (PqNbrPatch)
  std::atomic<uint64_t> pq_nbr_builds{0}, pq_nbr_patches{0}, pq_nbr_patched_rows{0};
  bool dense = true; uint64_t dense_base = 0;
  std::unordered_map<uint64_t, uint32_t> id2slot;
  std::vector<uint64_t> h_ids;       // !dense
  std::vector<int32_t> h_levels;     // per slot
  std::vector<uint32_t> h_upper_off; // per slot
  std::vector<uint32_t> h_del;       // bitmap mirror
  hipStream_t stream = nullptr;        // mutations (exclusive lock); searches use their context's stream
  std::atomic<float> last_ms{0.f};     // kernel time of the most recently finished search call
  CtxPool<HCtx> pool;
  DevBuf w_raw, w_misc;
  DevBuf b_head, b_req, b_levels; uint64_t head_cap = 0;  // builder scratch
  // HBM visited set (hnsw_dev.hpp, VISG): vis_regions regions of vis_stride bytes; concurrent searches lease disjoint
  // contiguous runs of regions (vis_busy), the builder (exclusive lock) uses all of them.
  DevBuf w_visg, w_vepoch; uint64_t vis_stride = 0; uint32_t vis_regions = 0, vis_want = 0;
  std::mutex vis_mu; std::condition_variable vis_cv; std::vector<uint8_t> vis_busy;
  coltt_hnsw_stats build_stats{};
  uint64_t gen = 0;   // bumped whenever the slots are renumbered (Load / bulk_load, a failed install): filters built before are stale
  ~Hnsw() override {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamDestroy(stream);
  }
  GraphView view() const {
    GraphView g;
    g.rows = rows.as<uint8_t>(); g.stride = stride; g.norms = norms.as<float>();
    g.rows8 = r8 ? rows.as<uint8_t>() : nullptr;   // the same array: which core reads it is the kernel's choice
    g.ids = dense ? nullptr : ids.as<uint64_t>();
    g.adj0 = adj0.as<uint32_t>(); g.adj0_d = adj0_d.as<float>(); g.upper_off = upper_off.as<uint32_t>();
    g.adj0_n = metric == COLTT_COSINE ? adj0_n.as<float>() : nullptr;
    g.adjU = adjU.as<uint32_t>(); g.adjU_d = adjU_d.as<float>();
    g.del_bits = any_deleted ? del_bits.as<uint32_t>() : nullptr;
    g.mMax = (uint32_t)cfg.m_max; g.mMax0 = (uint32_t)cfg.m_max0; g.dim = (int)dim;
    g.rows_h = shadow ? rows_h.as<uint8_t>() : nullptr;
    g.rows_b = shadow8 ? rows_b.as<uint8_t>() : nullptr;
    g.rows_m = shadow8 ? rows_m.as<float2>() : nullptr;
    g.adj0_m = shadow8 ? adj0_m.as<float2>() : nullptr;
    return g;
  }
  int reserve(uint64_t slots, uint64_t upper_rows) {
    if (slots > cap) {
      uint64_t nc = std::max<uint64_t>({slots, cap + cap / 2, 1024});
      COLTT_TRY(rows.reserve(nc * stride, true, stream));
      if (shadow && rows_h.reserve(nc * (size_t)dim * 2, true, stream) != COLTT_OK) drop_shadow();   // not an error: no shadow, no filter
      if (shadow8 && (rows_b.reserve(nc * (size_t)dim, true, stream) != COLTT_OK || rows_m.reserve(nc * 8, true, stream) != COLTT_OK ||
                      adj0_m.reserve(nc * cfg.m_max0 * 8, true, stream) != COLTT_OK)) drop_shadow8();
      COLTT_TRY(norms.reserve(nc * 4, true, stream));
      if (!dense) COLTT_TRY(ids.reserve(nc * 8, true, stream));
      COLTT_TRY(adj0.reserve(nc * cfg.m_max0 * 4, true, stream));
      COLTT_TRY(adj0_d.reserve(nc * cfg.m_max0 * 4, true, stream));
      if (metric == COLTT_COSINE) COLTT_TRY(adj0_n.reserve(nc * cfg.m_max0 * 4, true, stream));
      COLTT_TRY(upper_off.reserve(nc * 4, true, stream));
      size_t old_words = (cap + 31) / 32, new_words = (nc + 31) / 32;
      COLTT_TRY(del_bits.reserve(new_words * 4, true, stream));
      if (new_words > old_words) COLTT_HIP(hipMemsetAsync(del_bits.as<uint32_t>() + old_words, 0, (new_words - old_words) * 4, stream));
      cap = nc;
    }
    if (upper_rows > ucap) {
      uint64_t nc = std::max<uint64_t>({upper_rows, ucap + ucap / 2, 256});
      COLTT_TRY(adjU.reserve(nc * cfg.m_max * 4, true, stream));
      COLTT_TRY(adjU_d.reserve(nc * cfg.m_max * 4, true, stream));
      ucap = nc;
    }
    return COLTT_OK;
  }
};

// What the search decisions read of an index, and what they decide (include/coltt_gpu.h; hnsw.hip: plan_search).
typedef coltt_hnsw_plan_facts PlanFacts;
typedef coltt_hnsw_search_plan SearchPlan;

// The LDS layout of the one-wave walk (hnsw_dev.hpp: search_level) at one ef: what the builder and the filtered drivers launch (walk_geom).
struct SearchGeom { uint32_t ef, ef_pad, hcap; size_t lds; bool visg; uint32_t max_grid; };

// Lease a contiguous run of visited-set regions for one search launch: `want` if a free run that long exists, else the
// longest free run; blocks while every region is out.  Released by the RegionLease destructor.
struct RegionLease {
  Hnsw* x = nullptr; uint32_t base = 0, count = 0;
  ~RegionLease() {
    if (!x || !count) return;
    { std::lock_guard<std::mutex> g(x->vis_mu); for (uint32_t i = 0; i < count; i++) x->vis_busy[base + i] = 0; }
    x->vis_cv.notify_all();
  }
};

// The launch geometry of one walk over the quantiser's codes at one ef (pq_walk_geom).
struct PqGeom { uint32_t ef, ef_pad, vis_words; size_t lds; int variant; /* 0: LDS hash | 2: byte map + delta result set */ uint32_t per_cu; };

// The two device allocations the outputs of one coltt_hnsw_filter_eval(_batch) call share (filter_expr.hpp): freed when the last output goes.
struct FilterSlab {
  int device = 0;
  DevBuf bits, lists;
  ~FilterSlab() { (void)hipSetDevice(device); }
};

struct HnswFilter : Object {
  coltt_handle_t index = 0; uint64_t gen = 0;   // built against this index at this generation (Hnsw::gen)
  uint32_t slots = 0;                           // the index's slots when the filter was built: the bitmap covers [0, slots)
  uint64_t allowed = 0;
  DevBuf bits;   // [ceil(slots / 32)] u32, bit s = slot s allowed
  DevBuf list;   // [allowed] u32, the allowed slots ascending (the exact path's gather list)
  std::shared_ptr<FilterSlab> slab;   // set: bits and list point into the slab and are not this filter's to free
  ~HnswFilter() override {
    (void)hipSetDevice(device);
    if (slab) { bits.p = nullptr; list.p = nullptr; }
  }
};

// An attribute column (coltt_hnsw_attr_*; include/coltt_gpu.h, "Attribute columns and predicates").  `rw` is the column's own lock: attr_set holds
// it exclusive (and the index's shared), attr_get and an evaluation hold it shared.
struct HnswAttr : Object {
  coltt_handle_t index = 0; uint64_t gen = 0;   // as HnswFilter
  int type = COLTT_ATTR_I64;
  uint32_t slots = 0;            // covered: the index's slot count at the last attr_set
  uint64_t cap = 0, n_set = 0;   // slots allocated; slots that hold a value
  DevBuf vals;                   // [cap] 8-byte values
  DevBuf set;                    // [ceil(cap / 32)] u32, bit s = slot s holds a value; words past the covered slots are 0
  std::vector<uint32_t> h_set;   // its mirror
  ~HnswAttr() override { (void)hipSetDevice(device); }
};

// log2 of a table row in LDS: the centroid count rounded up to a power of two, at least 16 (codes >= C never occur)
inline uint32_t pq_lut_shift(const Hnsw* x) { uint32_t sh = 4; while ((1u << sh) < x->pq_shape.C) sh++; return sh; }
// the capacity of a filtered walk's allowed set R: what the re-rank may read
inline uint32_t pq_filt_cap(uint32_t ef, uint32_t k, uint32_t rerank) { return rerank == 0 ? ef : std::min(std::max(rerank, k), ef); }

// ---- hnsw.hip
int prep_queries_any(Hnsw* x, HCtx* c, const float* d_qraw, size_t nq, uint32_t* zero64 = nullptr);
// ids[i] += base on `stream`: the answers of a dense-id index whose ids do not start at 0
void add_base(hipStream_t stream, uint64_t* ids, size_t n, uint64_t base);
int ensure_visg(Hnsw* x, const Policy& pol);
void acquire_regions(Hnsw* x, uint32_t want, RegionLease& out);
// The search decisions: pure functions of (facts, knob snapshot).  A caller takes ONE policy() snapshot per call and passes it down.
PlanFacts plan_facts(const Hnsw* x);
bool wants_visg(const Policy& pol, uint32_t ef);   // does this ef want the HBM visited set (whether the workspace could be had is PlanFacts::vis_ready)
// allowed > 0: the filtered walk's allowed set (rounded up to 64 entries) sits beside the result set (hnsw_kernels.hpp: search_one_wave)
SearchGeom walk_geom(const PlanFacts& f, const Policy& pol, uint32_t ef, uint32_t allowed = 0);
uint32_t resident_waves(const Policy& pol, int quant, size_t lds, int w2 = -1, bool vis16 = false);
// the hnsw_walk2.hpp variants the library carries over the HBM map / the LDS hash (hnsw_search2.hip instantiates exactly these)
inline bool walk2_shipped(bool hbm, int w2) { return hbm ? (w2 == 6 || w2 == 7) : w2 == 4; }
int plan_search(const PlanFacts& f, const Policy& pol, size_t nq, uint32_t k, uint32_t ef, int force, SearchPlan& out);
int ensure_pq_nbr(Hnsw* x, hipStream_t stream, bool* use);
int pq_walk_geom(Hnsw* x, uint32_t ef, bool force_hbm, uint32_t fcap, PqGeom& sg);
int launch_pq_walk(Hnsw* x, HCtx* c, const PqGeom& sg, bool nbr, uint32_t grid, uint32_t region_base, const unsigned short* lut, uint32_t nq, uint32_t k,
                   uint32_t rerank, uint32_t* counter, uint32_t* surv, uint32_t* surv_cnt, unsigned long long* stats, const FilterView* fv = nullptr, uint32_t fcap = 0,
                   const PqFiltQuery* pd = nullptr);
int launch_pq_rerank(Hnsw* x, HCtx* c, const PqGeom& sg, uint32_t q0, uint32_t nq, uint32_t k, const uint32_t* surv, const uint32_t* surv_cnt,
                     unsigned long long* keys, uint64_t* oi, float* os, uint32_t* oc, const PqFiltQuery* pd = nullptr, const float* pd_qe = nullptr,
                     const float* pd_qn = nullptr);
int pq_search_filtered_walk(Hnsw* x, HCtx* c, const FilterView& fv, const float* queries, size_t nq, uint32_t k, uint32_t ef_walk, uint32_t rerank,
                            uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact);

// ---- hnsw_search2.hip
int launch_search2(Hnsw* x, HCtx* c, const SearchPlan& sp, uint32_t grid, uint32_t region_base, uint32_t nq, uint32_t k, uint32_t* counter,
                   uint64_t* oi, float* os, uint32_t* oc, unsigned long long* stats);

}  // namespace hnsw
}  // namespace coltt
