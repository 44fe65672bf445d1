// coltt_gpu.hpp — header-only C++ mirror of the reference's Go interfaces over the C-ABI (include/coltt_gpu.h).
//
// The reference is compiled code (Go) whose toolchain is absent from the build image, so the host side above the C-ABI is
// mirrored here in C++ with the reference's own names, argument meaning and error behaviour:
//   coltt::VecSpace  <->  edge.vectorspace            (edge/vectorstore.go:30-49)
//   coltt::Hnsw      <->  *vectorindex.Hnsw           (core/vectorindex/hnsw.go:43-54)
// Metadata maps stay with the caller: results carry ids and scores only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "coltt_gpu.h"

namespace coltt {

struct Error : std::runtime_error {
  int code;
  Error(int c, const char* m) : std::runtime_error(m), code(c) {}
};
struct ItemNotFoundError : Error { using Error::Error; };       // core/vectorindex/hnsw.go:39
struct ItemAlreadyExistsError : Error { using Error::Error; };  // core/vectorindex/hnsw.go:40

inline void check(int rc) {
  if (rc == COLTT_OK) return;
  if (rc == COLTT_E_NOT_FOUND) throw ItemNotFoundError(rc, coltt_last_error());
  if (rc == COLTT_E_EXISTS) throw ItemAlreadyExistsError(rc, coltt_last_error());
  throw Error(rc, coltt_last_error());
}

using Vector = std::vector<float>;                                 // edge.Vector (edge/constants.go:76)
struct SearchResultItem { uint64_t Id; float Score; };             // edge/priority_queue.go:27-31 minus Metadata
using SearchResult = std::vector<SearchResultItem>;

// edge.Metadata (edge/edge_metadata.go:25-55): what CreateCollection fixes for a collection.  IndexType carries the caller's
// index features by name (edge.IndexFeature is the inverted index's business — pkg/inverted is out of scope).
struct CollectionMetadata {
  uint32_t Dim = 0; int Distance = COLTT_COSINE; int Quantization = COLTT_Q_NONE; bool Versioning = false;
  std::map<std::string, std::string> IndexType;
};

// edge.vectorspace implemented on the GPU — all 16 methods of edge/vectorstore.go:30-49.  Metadata maps and the inverted
// index stay with the caller: ChangedVertex / RemoveVertex / FilterableVertexSearch take the ids the
// caller's index resolved, Save/LoadVertexInverted carry the caller's serialized index as an opaque blob, results carry
// ids and scores.  (The Go file go/edge/gpu_vectorstore.go is the variant that owns those parts inside package edge.)
class VecSpace {
 public:
  VecSpace(uint32_t dim, int distance /*COLTT_COSINE|EUCLIDEAN*/, int quantization /*COLTT_Q_**/)
      : dim_(dim), distance_(distance), quant_(quantization) {
    meta_.Dim = dim; meta_.Distance = distance; meta_.Quantization = quantization;
    check(coltt_flat_create(dim, distance, quantization, &h_));
  }
  explicit VecSpace(const CollectionMetadata& m) : VecSpace(m.Dim, m.Distance, m.Quantization) { meta_ = m; }
  ~VecSpace() { if (h_) coltt_flat_destroy(h_); }
  VecSpace(const VecSpace&) = delete;
  VecSpace& operator=(const VecSpace&) = delete;

  // ChangedVertex(updateID, Id, ENode) — vector half (edge/none_vectorstore.go:66-103)
  void ChangedVertex(uint64_t id, const Vector& v) {
    if (v.size() != dim_)  // none_vectorstore.go:86-88
      throw Error(COLTT_E_INVALID, ("Dim Length UnmatchdError: expect dimension: [" + std::to_string(dim_) + "], but got [" +
                                    std::to_string(v.size()) + "]").c_str());
    check(coltt_flat_upsert(h_, &id, v.data(), 1));
  }
  void ChangedVertices(const std::vector<uint64_t>& ids, const float* rows) { check(coltt_flat_upsert(h_, ids.data(), rows, ids.size())); }
  // RemoveVertex after the inverted index resolved the drop filter to ids (none_vectorstore.go:105-127)
  void RemoveVertex(const std::vector<uint64_t>& ids) { check(coltt_flat_remove(h_, ids.data(), ids.size())); }
  // VertexSearch(target, topK, highCpu) (none_vectorstore.go:129-180); highCpu has no meaning on the GPU
  SearchResult VertexSearch(const Vector& target, int topK, bool /*highCpu*/ = false, int select = COLTT_SELECT_REFERENCE) const {
    std::vector<uint64_t> ids(topK); std::vector<float> sc(topK); uint32_t n = 0;
    check(coltt_flat_search(h_, target.data(), 1, (uint32_t)topK, select, COLTT_MODE_EXACT, ids.data(), sc.data(), &n));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  // FilterableVertexSearch(filter, target, topK, highCpu) with the filter already evaluated to candidate ids (:182-253)
  SearchResult FilterableVertexSearch(const std::vector<uint64_t>& candidates, const Vector& target, int topK,
                                      int select = COLTT_SELECT_REFERENCE) const {
    std::vector<uint64_t> ids(topK); std::vector<float> sc(topK); uint32_t n = 0;
    check(coltt_flat_search_ids(h_, target.data(), 1, (uint32_t)topK, select, candidates.data(), candidates.size(), ids.data(), sc.data(), &n));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  // a batch of FilterableVertexSearch RPCs in one call, every target with its own candidate list (coltt_flat_search_ids_batch): result i
  // equals FilterableVertexSearch(candidates[list_of[i]], targets[i], topK, select); an empty list_of means target i uses candidates[i]
  std::vector<SearchResult> FilterableVertexSearchBatch(const std::vector<std::vector<uint64_t>>& candidates, const std::vector<Vector>& targets,
                                                        int topK, int select = COLTT_SELECT_REFERENCE, const std::vector<uint32_t>& list_of = {}) const {
    const size_t nq = targets.size();
    std::vector<float> q(nq * dim_);
    for (size_t i = 0; i < nq; i++) {
      if (targets[i].size() != dim_) throw Error(COLTT_E_INVALID, "FilterableVertexSearchBatch: a target's length differs from the store's dimension");
      std::copy(targets[i].begin(), targets[i].end(), q.begin() + i * dim_);
    }
    if (!list_of.empty() && list_of.size() != nq) throw Error(COLTT_E_INVALID, "FilterableVertexSearchBatch: list_of needs one entry per target");
    std::vector<uint64_t> off(candidates.size() + 1, 0), cand;
    for (size_t l = 0; l < candidates.size(); l++) { cand.insert(cand.end(), candidates[l].begin(), candidates[l].end()); off[l + 1] = cand.size(); }
    const size_t kk = topK > 0 ? (size_t)topK : 1;
    std::vector<uint64_t> ids(nq * kk); std::vector<float> sc(nq * kk); std::vector<uint32_t> n(nq, 0);
    check(coltt_flat_search_ids_batch(h_, q.data(), nq, (uint32_t)topK, select, cand.data(), off.data(), candidates.size(),
                                      list_of.empty() ? nullptr : list_of.data(), ids.data(), sc.data(), n.data()));
    std::vector<SearchResult> out(nq);
    for (size_t i = 0; i < nq; i++) {
      out[i].resize(n[i]);
      for (uint32_t j = 0; j < n[i]; j++) out[i][j] = {ids[i * kk + j], sc[i * kk + j]};
    }
    return out;
  }
  // SaveVertex / LoadVertex (none_vectorstore.go:308-516 and twins): the `.vertex` byte stream, metadata written as empty maps
  std::vector<uint8_t> SaveVertex() const {
    uint64_t n = 0;
    check(coltt_flat_save_vertex(h_, nullptr, nullptr, nullptr, 0, nullptr, 0, &n));
    std::vector<uint8_t> out(n);
    check(coltt_flat_save_vertex(h_, nullptr, nullptr, nullptr, 0, out.data(), out.size(), &n));
    return out;
  }
  uint64_t LoadVertex(const std::vector<uint8_t>& data) {
    uint64_t n = 0;
    check(coltt_flat_load_vertex(h_, data.data(), data.size(), &n, nullptr, nullptr, nullptr, 0));
    return n;
  }
  // SaveVertexMetadata / LoadVertexMetadata (none_vectorstore.go:255-274): the collection metadata as JSON; loading re-checks
  // it against the device store (dim / distance / quantisation are fixed at creation).
  std::string SaveVertexMetadata() const {
    std::string j = "{\"dim\":" + std::to_string(meta_.Dim) + ",\"distance\":" + std::to_string(meta_.Distance) + ",\"quantization\":" +
                    std::to_string(meta_.Quantization) + ",\"versioning\":" + (meta_.Versioning ? "true" : "false") + ",\"index_type\":{";
    bool first = true;
    for (auto& kv : meta_.IndexType) { j += (first ? "\"" : ",\"") + kv.first + "\":\"" + kv.second + "\""; first = false; }
    return j + "}}";
  }
  void LoadVertexMetadata(const std::string& /*collectionName*/, const CollectionMetadata& m) {
    if (m.Dim != dim_ || m.Distance != distance_ || m.Quantization != quant_)
      throw Error(COLTT_E_INVALID, "LoadVertexMetadata: dim / distance / quantization differ from the device store's");
    meta_ = m;
  }
  // SaveVertexInverted / LoadVertexInverted (:276-283): the caller's inverted index, carried opaquely
  const std::vector<uint8_t>& SaveVertexInverted() const { return inverted_blob_; }
  void LoadVertexInverted(const std::vector<uint8_t>& data) { inverted_blob_ = data; }
  int Quantization() const { return quant_; }
  int Distance() const { return distance_; }
  uint32_t Dim() const { return dim_; }
  int64_t LoadSize() const { uint64_t n = 0; check(coltt_flat_len(h_, &n)); return (int64_t)n; }
  const std::map<std::string, std::string>& Indexer() const { return meta_.IndexType; }
  bool Versional() const { return meta_.Versioning; }
  coltt_handle_t handle() const { return h_; }

 private:
  coltt_handle_t h_ = 0; uint32_t dim_; int distance_, quant_;
  CollectionMetadata meta_; std::vector<uint8_t> inverted_blob_;
};

// functional options of NewHnsw (hnsw_config.go:57-109) as a fluent builder: HnswOptions().M(32).Ef(64).SearchAlgorithm(1)
struct HnswOptions {
  coltt_hnsw_cfg c{16, -1, -1, 20, 200, 0, -1.f, 0, 1};   // newHnswConfig defaults (hnsw_config.go:135-162)
  int quantization = COLTT_Q_NONE;
  HnswOptions& LevelMultiplier(float v) { c.level_multiplier = v; return *this; }
  HnswOptions& Ef(int v) { c.ef = v; return *this; }
  HnswOptions& EfConstruction(int v) { c.ef_construction = v; return *this; }
  HnswOptions& M(int v) { c.m = v; return *this; }
  HnswOptions& Mmax(int v) { c.m_max = v; return *this; }
  HnswOptions& Mmax0(int v) { c.m_max0 = v; return *this; }
  HnswOptions& SearchAlgorithm(int v /*0 HnswSearchSimple, 1 HnswSearchHeuristic; COLTT_HNSW_DIVERSE (2) is NOT reference behaviour, see coltt_gpu.h*/) { c.algo = v; return *this; }
  HnswOptions& HeuristicExtendCandidates(bool v) { c.extend_candidates = v; return *this; }
  HnswOptions& HeuristicKeepPruned(bool v) { c.keep_pruned = v; return *this; }
  HnswOptions& Quantization(int q) { quantization = q; return *this; }   // extension: BASELINE.json configs[4]
};
struct ProtoConfig {   // hnsw_config.go:123-133
  std::string SearchAlgorithm; float LevelMultiplier; int Ef, EfConstruction, M, MMax, MMax0; bool HeuristicExtendCandidates, HeuristicKeepPruned;
};
struct Vertex { uint64_t Id; Vector Vec; int Level; };   // what GetVertex hands out (hnsw_vertex.go:54-68), minus Metadata

// *vectorindex.Hnsw implemented on the GPU
class Hnsw {
 public:
  Hnsw(uint32_t dim, int distance, const HnswOptions& o) : Hnsw(dim, distance, &o.c, o.quantization) {}
  // NewHnsw(dim, distancer, options...) (hnsw.go:56-73)
  Hnsw(uint32_t dim, int distance, const coltt_hnsw_cfg* cfg = nullptr, int quantization = COLTT_Q_NONE) : dim_(dim), distance_(distance) {
    check(coltt_hnsw_create(dim, distance, quantization, cfg, &h_));
  }
  ~Hnsw() { if (h_) coltt_hnsw_destroy(h_); }
  Hnsw(const Hnsw&) = delete;
  Hnsw& operator=(const Hnsw&) = delete;

  void Insert(uint64_t id, const Vector& value, int vertexLevel) { check(coltt_hnsw_insert(h_, id, value.data(), vertexLevel)); }  // hnsw.go:104
  void Remove(uint64_t id) { check(coltt_hnsw_remove(h_, id)); }                                                                    // hnsw.go:191
  // Reclaim the slots Remove left behind — an extension the reference does not have (coltt_gpu.h, "HNSW compaction"): vertex s moves to slot
  // new(s) = live slots below s, no search answer changes, Filters built before are stale.  stage_bytes: the staging block (0 = 64 MiB);
  // new_of_old (may be NULL) receives new() for the slots before the call, 0xffffffff for a dropped one.
  coltt_hnsw_compact_stats Compact(uint64_t stage_bytes = 0, std::vector<uint32_t>* new_of_old = nullptr) {
    coltt_hnsw_compact_stats st{};
    if (!new_of_old) { check(coltt_hnsw_compact(h_, stage_bytes, nullptr, 0, &st)); return st; }
    uint64_t n = 0;
    check(coltt_hnsw_export_raw(h_, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    new_of_old->resize(n);
    check(coltt_hnsw_compact(h_, stage_bytes, new_of_old->data(), n, &st));
    new_of_old->resize(st.slots_before);
    return st;
  }
  // Compact, after which the listed filters and attribute columns are valid at the new generation under the same handles (coltt_gpu.h,
  // "Carrying resident filters and attribute columns through a compaction"); what is not listed goes stale.  Defined below the two classes.
  struct CarryResult {
    coltt_hnsw_compact_stats stats{}; coltt_hnsw_carry_stats carry{};
    std::vector<uint64_t> allowed, set;   // per listed filter / column, after the call
  };
  class Filter;
  class AttrColumn;
  CarryResult CompactCarry(const std::vector<Filter*>& filters, const std::vector<AttrColumn*>& columns, uint64_t stage_bytes = 0,
                           std::vector<uint32_t>* new_of_old = nullptr);
  SearchResult Search(const Vector& query, unsigned k) const {                                                                       // hnsw.go:243
    std::vector<uint64_t> ids(k); std::vector<float> sc(k); uint32_t n = 0;
    check(coltt_hnsw_search(h_, query.data(), 1, k, 0, ids.data(), sc.data(), &n, nullptr));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  // Filtered search — an extension the reference does not have (coltt_gpu.h, "Filtered HNSW search"): the k nearest among the ids of a
  // Filter built against this index.  mode: COLTT_FILTER_AUTO / _WALK / _EXACT.
  class Filter {
   public:
    Filter(const Hnsw& index, const std::vector<uint64_t>& ids) { check(coltt_hnsw_filter_create(index.h_, ids.data(), ids.size(), &allowed_, &h_)); }
    ~Filter() { if (h_) coltt_hnsw_filter_destroy(h_); }
    Filter(const Filter&) = delete;
    Filter& operator=(const Filter&) = delete;
    uint64_t Allowed() const { return allowed_; }
    coltt_handle_t handle() const { return h_; }
    // the allowed ids in ascending slot order, gathered on the device (coltt_hnsw_filter_ids); cap: at most that many
    std::vector<uint64_t> Ids(uint64_t cap = UINT64_MAX) const {
      std::vector<uint64_t> o((size_t)std::min<uint64_t>(cap, allowed_)); uint64_t n = 0;
      check(coltt_hnsw_filter_ids(h_, o.data(), o.size(), &n));
      return o;
    }
    // the slots of the index the filter covers (coltt_hnsw_filter_info)
    uint64_t Slots() const { uint64_t s = 0; check(coltt_hnsw_filter_info(h_, nullptr, nullptr, &s)); return s; }
   private:
    friend class Hnsw;
    Filter(coltt_handle_t h, uint64_t allowed) : h_(h), allowed_(allowed) {}
    coltt_handle_t h_ = 0; uint64_t allowed_ = 0;
  };
  // Filter expressions (coltt_gpu.h, "Filter expressions"): a postfix programme (leaf indices >= 0, COLTT_FOP_* operators) over resident
  // filters, evaluated on the device.  The result is an ordinary Filter.
  std::unique_ptr<Filter> FilterEval(const std::vector<int32_t>& prog, const std::vector<const Filter*>& leaves) const {
    std::vector<coltt_handle_t> lh(leaves.size());
    for (size_t i = 0; i < leaves.size(); i++) lh[i] = leaves[i] ? leaves[i]->handle() : 0;
    coltt_handle_t h = 0; uint64_t allowed = 0;
    check(coltt_hnsw_filter_eval(h_, prog.data(), prog.size(), lh.data(), lh.size(), &allowed, &h));
    return std::unique_ptr<Filter>(new Filter(h, allowed));
  }
  // one Filter per programme over a shared leaf table, under one index state, in two kernel launches (coltt_hnsw_filter_eval_batch)
  std::vector<std::unique_ptr<Filter>> FilterEvalBatch(const std::vector<std::vector<int32_t>>& progs, const std::vector<const Filter*>& leaves) const {
    std::vector<coltt_handle_t> lh(leaves.size());
    for (size_t i = 0; i < leaves.size(); i++) lh[i] = leaves[i] ? leaves[i]->handle() : 0;
    std::vector<int32_t> flat; std::vector<uint64_t> off(progs.size() + 1, 0);
    for (size_t i = 0; i < progs.size(); i++) { flat.insert(flat.end(), progs[i].begin(), progs[i].end()); off[i + 1] = flat.size(); }
    std::vector<coltt_handle_t> hs(progs.size(), 0); std::vector<uint64_t> al(progs.size(), 0);
    check(coltt_hnsw_filter_eval_batch(h_, flat.data(), off.data(), progs.size(), lh.data(), lh.size(), al.data(), hs.data()));
    std::vector<std::unique_ptr<Filter>> out;
    for (size_t i = 0; i < progs.size(); i++) out.emplace_back(new Filter(hs[i], al[i]));
    return out;
  }
  // Attribute columns (coltt_gpu.h, "Attribute columns and predicates"): one int64_t (COLTT_ATTR_I64) or double (COLTT_ATTR_F64) per slot beside
  // the index; comparisons over them are leaves of a filter programme.  Stale after Load / BulkLoad / a Compact that renumbered: set again by ids
  // (CompactCarry keeps the listed ones valid).
  class AttrColumn {
   public:
    AttrColumn(const Hnsw& index, int type) : type_(type) { check(coltt_hnsw_attr_create(index.h_, type, &h_)); }
    ~AttrColumn() { if (h_) coltt_hnsw_attr_destroy(h_); }
    AttrColumn(const AttrColumn&) = delete;
    AttrColumn& operator=(const AttrColumn&) = delete;
    coltt_handle_t handle() const { return h_; }
    int Type() const { return type_; }
    // ids -> values (an id repeated takes its last value; unknown and removed ids are ignored); returns the vertices set
    uint64_t Set(const std::vector<uint64_t>& ids, const std::vector<int64_t>& values) { return set(COLTT_ATTR_I64, ids, values.data(), values.size()); }
    uint64_t Set(const std::vector<uint64_t>& ids, const std::vector<double>& values) { return set(COLTT_ATTR_F64, ids, values.data(), values.size()); }
    // the raw 8-byte values of ids and whether each has one
    void Get(const std::vector<uint64_t>& ids, std::vector<uint64_t>* raw_values, std::vector<uint8_t>* is_set) const {
      if (raw_values) raw_values->assign(ids.size(), 0);
      if (is_set) is_set->assign(ids.size(), 0);
      check(coltt_hnsw_attr_get(h_, ids.data(), ids.size(), raw_values ? raw_values->data() : nullptr, is_set ? is_set->data() : nullptr));
    }
    uint64_t Slots() const { uint64_t s = 0; check(coltt_hnsw_attr_info(h_, nullptr, nullptr, &s, nullptr)); return s; }
    uint64_t SetCount() const { uint64_t s = 0; check(coltt_hnsw_attr_info(h_, nullptr, nullptr, nullptr, &s)); return s; }
    // a predicate over this column for FilterEvalAttr: op = COLTT_CMP_*
    coltt_attr_pred Pred(int op, int64_t operand) const { coltt_attr_pred p{}; p.column = h_; p.op = op; p.value.i64 = operand; return p; }
    coltt_attr_pred Pred(int op, double operand) const { coltt_attr_pred p{}; p.column = h_; p.op = op; p.value.f64 = operand; return p; }
   private:
    uint64_t set(int type, const std::vector<uint64_t>& ids, const void* values, size_t n) {
      if (type != type_ || n != ids.size()) throw std::invalid_argument("AttrColumn::Set: values of the wrong type or length");
      uint64_t applied = 0;
      check(coltt_hnsw_attr_set(h_, ids.data(), values, n, &applied));
      return applied;
    }
    coltt_handle_t h_ = 0; int type_ = COLTT_ATTR_I64;
  };
  // a programme over leaves and predicates: a value v >= 0 pushes leaves[v] when v < leaves.size(), predicate v - leaves.size() otherwise
  std::unique_ptr<Filter> FilterEvalAttr(const std::vector<int32_t>& prog, const std::vector<const Filter*>& leaves,
                                         const std::vector<coltt_attr_pred>& preds) const {
    std::vector<coltt_handle_t> lh(leaves.size());
    for (size_t i = 0; i < leaves.size(); i++) lh[i] = leaves[i] ? leaves[i]->handle() : 0;
    coltt_handle_t h = 0; uint64_t allowed = 0;
    check(coltt_hnsw_filter_eval_attr(h_, prog.data(), prog.size(), lh.data(), lh.size(), preds.data(), preds.size(), &allowed, &h));
    return std::unique_ptr<Filter>(new Filter(h, allowed));
  }
  std::vector<std::unique_ptr<Filter>> FilterEvalAttrBatch(const std::vector<std::vector<int32_t>>& progs, const std::vector<const Filter*>& leaves,
                                                           const std::vector<coltt_attr_pred>& preds) const {
    std::vector<coltt_handle_t> lh(leaves.size());
    for (size_t i = 0; i < leaves.size(); i++) lh[i] = leaves[i] ? leaves[i]->handle() : 0;
    std::vector<int32_t> flat; std::vector<uint64_t> off(progs.size() + 1, 0);
    for (size_t i = 0; i < progs.size(); i++) { flat.insert(flat.end(), progs[i].begin(), progs[i].end()); off[i + 1] = flat.size(); }
    std::vector<coltt_handle_t> hs(progs.size(), 0); std::vector<uint64_t> al(progs.size(), 0);
    check(coltt_hnsw_filter_eval_attr_batch(h_, flat.data(), off.data(), progs.size(), lh.data(), lh.size(), preds.data(), preds.size(), al.data(), hs.data()));
    std::vector<std::unique_ptr<Filter>> out;
    for (size_t i = 0; i < progs.size(); i++) out.emplace_back(new Filter(hs[i], al[i]));
    return out;
  }
  SearchResult SearchFiltered(const Vector& query, unsigned k, const Filter& f, unsigned ef = 0, int mode = COLTT_FILTER_AUTO,
                              coltt_hnsw_filter_stats* stats = nullptr) const {
    std::vector<uint64_t> ids(k); std::vector<float> sc(k); uint32_t n = 0;
    check(coltt_hnsw_search_filtered(h_, f.handle(), query.data(), 1, k, ef, mode, ids.data(), sc.data(), &n, stats));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  // the same over the walk on product-quantiser codes (coltt_hnsw_pq_search_filtered; the index carries a quantiser: coltt_hnsw_pq_attach);
  // rerank as coltt_hnsw_pq_search (0: every member of the allowed set is re-scored exactly)
  SearchResult PqSearchFiltered(const Vector& query, unsigned k, const Filter& f, unsigned ef = 0, unsigned rerank = 0, int mode = COLTT_FILTER_AUTO,
                                coltt_hnsw_filter_stats* stats = nullptr) const {
    std::vector<uint64_t> ids(k); std::vector<float> sc(k); uint32_t n = 0;
    check(coltt_hnsw_pq_search_filtered(h_, f.handle(), query.data(), 1, k, ef, rerank, mode, ids.data(), sc.data(), &n, stats));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  // a filter per query (coltt_hnsw_search_filtered_batch): answer i == SearchFiltered(queries[i], k, *filters[i], ef, mode); paths (may be
  // null) receives the path each query took
  std::vector<SearchResult> SearchFilteredBatch(const std::vector<Vector>& queries, unsigned k, const std::vector<const Filter*>& filters,
                                                unsigned ef = 0, int mode = COLTT_FILTER_AUTO, std::vector<int>* paths = nullptr,
                                                coltt_hnsw_filter_stats* stats = nullptr) const {
    const size_t nq = queries.size();
    if (filters.size() != nq) throw Error(COLTT_E_INVALID, "SearchFilteredBatch: one filter per query");
    std::vector<float> flat(nq * dim_);
    std::vector<coltt_handle_t> fh(nq);
    for (size_t i = 0; i < nq; i++) {
      if (queries[i].size() != dim_) throw Error(COLTT_E_INVALID, "SearchFilteredBatch: query of the wrong dimension");
      std::copy(queries[i].begin(), queries[i].end(), flat.begin() + i * dim_);
      fh[i] = filters[i] ? filters[i]->handle() : 0;
    }
    std::vector<uint64_t> ids(nq * k); std::vector<float> sc(nq * k); std::vector<uint32_t> n(nq); std::vector<int32_t> p(nq);
    check(coltt_hnsw_search_filtered_batch(h_, fh.data(), flat.data(), nq, k, ef, mode, ids.data(), sc.data(), n.data(), p.data(), stats));
    std::vector<SearchResult> out(nq);
    for (size_t i = 0; i < nq; i++) {
      out[i].resize(n[i]);
      for (uint32_t j = 0; j < n[i]; j++) out[i][j] = {ids[i * k + j], sc[i * k + j]};
    }
    if (paths) paths->assign(p.begin(), p.end());
    return out;
  }
  // a filter per query over the walk on product-quantiser codes (coltt_hnsw_pq_search_filtered_batch): answer i ==
  // PqSearchFiltered(queries[i], k, *filters[i], ef, rerank, mode); paths (may be null) receives the path each query took
  std::vector<SearchResult> PqSearchFilteredBatch(const std::vector<Vector>& queries, unsigned k, const std::vector<const Filter*>& filters,
                                                  unsigned ef = 0, unsigned rerank = 0, int mode = COLTT_FILTER_AUTO,
                                                  std::vector<int>* paths = nullptr, coltt_hnsw_filter_stats* stats = nullptr) const {
    const size_t nq = queries.size();
    if (filters.size() != nq) throw Error(COLTT_E_INVALID, "PqSearchFilteredBatch: one filter per query");
    std::vector<float> flat(nq * dim_);
    std::vector<coltt_handle_t> fh(nq);
    for (size_t i = 0; i < nq; i++) {
      if (queries[i].size() != dim_) throw Error(COLTT_E_INVALID, "PqSearchFilteredBatch: query of the wrong dimension");
      std::copy(queries[i].begin(), queries[i].end(), flat.begin() + i * dim_);
      fh[i] = filters[i] ? filters[i]->handle() : 0;
    }
    std::vector<uint64_t> ids(nq * k); std::vector<float> sc(nq * k); std::vector<uint32_t> n(nq); std::vector<int32_t> p(nq);
    check(coltt_hnsw_pq_search_filtered_batch(h_, fh.data(), flat.data(), nq, k, ef, rerank, mode, ids.data(), sc.data(), n.data(), p.data(), stats));
    std::vector<SearchResult> out(nq);
    for (size_t i = 0; i < nq; i++) {
      out[i].resize(n[i]);
      for (uint32_t j = 0; j < n[i]; j++) out[i][j] = {ids[i * k + j], sc[i * k + j]};
    }
    if (paths) paths->assign(p.begin(), p.end());
    return out;
  }
  // the neighbourhood blocks of the product-quantised walk (coltt_hnsw_pq_nbr_stats): State 0 = none, 1 = current, 2 = stale
  struct PqNbrStatsResult { uint64_t Builds = 0, Patches = 0, PatchedRows = 0; int State = 0; };
  PqNbrStatsResult PqNbrStats() const {
    PqNbrStatsResult r; int32_t st = 0;
    check(coltt_hnsw_pq_nbr_stats(h_, &r.Builds, &r.Patches, &r.PatchedRows, &st));
    r.State = st;
    return r;
  }
  // the blocks of slots [first, first + n) as the walk reads them (coltt_hnsw_pq_fetch_nbr): [n][mMax0][code row rounded up to 16]; test / diagnostics
  std::vector<uint8_t> PqFetchNbr(uint64_t first, uint64_t n) const {
    uint32_t m = 0;
    check(coltt_hnsw_pq_info(h_, &m, nullptr, nullptr, nullptr));
    std::vector<uint8_t> out((size_t)n * (size_t)RawConfig().m_max0 * ((m + 15u) & ~15u));
    check(coltt_hnsw_pq_fetch_nbr(h_, first, n, out.data()));
    return out;
  }
  // which kernel Search(queries[nq], k, ef) launches on this index as it is now, and how (coltt_hnsw_search_plan_host over the index's facts; no launch)
  coltt_hnsw_plan_facts PlanFacts() const { coltt_hnsw_plan_facts f; check(coltt_hnsw_search_plan_facts(h_, &f)); return f; }
  coltt_hnsw_search_plan SearchPlan(size_t nq, uint32_t k, uint32_t ef = 0, int force = 0) const {
    const coltt_hnsw_plan_facts f = PlanFacts();
    coltt_hnsw_search_plan p;
    check(coltt_hnsw_search_plan_host(&f, nq, k, ef ? ef : (uint32_t)RawConfig().ef, force, &p));
    return p;
  }
  int Len() const { uint64_t n = 0; check(coltt_hnsw_len(h_, &n)); return (int)n; }
  // the collection's size is known (bulk import, Load): every array allocated once; never shrinks, never limits an Insert
  void Reserve(uint64_t vertices, uint64_t upper_rows = 0) { check(coltt_hnsw_reserve(h_, vertices, upper_rows)); }
  // Commit(w, header) / Load(r, header) (hnsw_commit.go:69-278): the reference's big-endian stream (metadata: empty maps)
  std::vector<uint8_t> Commit(bool header = true) const {
    uint64_t n = 0;
    check(coltt_hnsw_commit(h_, header, nullptr, nullptr, 0, nullptr, 0, &n));
    std::vector<uint8_t> out(n);
    check(coltt_hnsw_commit(h_, header, nullptr, nullptr, 0, out.data(), out.size(), &n));
    return out;
  }
  uint64_t Load(const std::vector<uint8_t>& data, bool header = true) {
    uint64_t n = 0;
    check(coltt_hnsw_load(h_, header, data.data(), data.size(), &n, nullptr, nullptr, nullptr, 0));
    return n;
  }
  // RandomLevel() (hnsw.go:280-282) for the caller's uniform draw u in (0,1)
  int RandomLevel(float u) const { int32_t lv = 0; check(coltt_hnsw_random_level(h_, u, &lv)); return lv; }
  uint32_t Dim() const { return dim_; }
  coltt_hnsw_cfg RawConfig() const { coltt_hnsw_cfg c; check(coltt_hnsw_get_cfg(h_, &c)); return c; }
  ProtoConfig Config() const {   // hnsw.go:86-98
    coltt_hnsw_cfg c = RawConfig();
    return {c.algo == 0 ? "simple" : (c.algo == 1 ? "heuristic" : "diverse"), c.level_multiplier, c.ef, c.ef_construction, c.m, c.m_max, c.m_max0,
            c.extend_candidates != 0, c.keep_pruned != 0};
  }
  std::string Distance() const { return distance_ == COLTT_COSINE ? "cosine-dot" : "l2-squared"; }   // Space.Type(), space.go:69,101
  // Get(id) / GetVertex(id) (hnsw.go:169-189): the STORED (normalised) vector; ItemNotFoundError for unknown / removed ids
  Vector Get(uint64_t id) const { Vector v(dim_); check(coltt_hnsw_get(h_, id, v.data(), nullptr)); return v; }
  Vertex GetVertex(uint64_t id) const { Vertex x{id, Vector(dim_), 0}; int32_t lv = 0; check(coltt_hnsw_get(h_, id, x.Vec.data(), &lv)); x.Level = lv; return x; }
  // BytesSize() (hnsw.go:476-490): the reference's host-side estimate — pointers per vertex by level + vector bytes
  // (HNSW_VERTEX_EDGE_BYTES 12, HNSW_VERTEX_MUTEX_BYTES 24, hnsw_vertex.go:27-28); metadata bytes are the caller's to add
  uint64_t BytesSize() const {
    coltt_hnsw_cfg c = RawConfig();
    uint64_t ns = 0, nu = 0; int32_t ent = -1, el = 0;
    check(coltt_hnsw_export_raw(h_, &ns, &nu, &ent, &el, nullptr, nullptr, nullptr));
    const int maxLevel = ent >= 0 ? el : 10;
    double ptr = c.m_max0 * 12.0 + 24.0;
    for (int i = 1; i < maxLevel; i++) ptr += (c.m_max * 12.0 + 24.0) * std::exp((double)i / -(double)c.level_multiplier);
    return (uint64_t)std::floor((double)Len() * ptr) + (uint64_t)Len() * dim_ * 4;
  }
  coltt_handle_t handle() const { return h_; }

 private:
  coltt_handle_t h_ = 0; uint32_t dim_; int distance_ = COLTT_COSINE;
};

inline Hnsw::CarryResult Hnsw::CompactCarry(const std::vector<Filter*>& filters, const std::vector<AttrColumn*>& columns, uint64_t stage_bytes,
                                            std::vector<uint32_t>* new_of_old) {
  std::vector<coltt_handle_t> fh(filters.size()), ch(columns.size());
  for (size_t i = 0; i < filters.size(); i++) fh[i] = filters[i] ? filters[i]->handle() : 0;
  for (size_t i = 0; i < columns.size(); i++) ch[i] = columns[i] ? columns[i]->handle() : 0;
  CarryResult r;
  r.allowed.assign(filters.size(), 0); r.set.assign(columns.size(), 0);
  uint64_t n = 0;
  if (new_of_old) {
    check(coltt_hnsw_export_raw(h_, &n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    new_of_old->resize(n);
  }
  check(coltt_hnsw_compact_carry(h_, stage_bytes, fh.data(), fh.size(), r.allowed.data(), ch.data(), ch.size(), r.set.data(),
                                 new_of_old ? new_of_old->data() : nullptr, n, &r.stats, &r.carry));
  if (new_of_old) new_of_old->resize(r.stats.slots_before);
  for (size_t i = 0; i < filters.size(); i++) if (filters[i]) filters[i]->allowed_ = r.allowed[i];
  return r;
}

// One collection over the GPUs of a node (BASELINE.json configs[4]): ShardVertex routing (pkg/sharding/shard.go:34-41), one FLAT
// store or HNSW graph per device, per-member search + one RCCL all-gather (or, members sharing a device, host staging) + the
// local-queue-then-global-queue merge of edge/none_vectorstore.go:148-178.  Thin wrapper over coltt_group_*.
class Group {
 public:
  Group(const std::vector<int>& devices, uint32_t dim, int distance, int quantization, int kind /*COLTT_GROUP_FLAT | _HNSW*/,
        int layout = COLTT_LAYOUT_SHARD, const coltt_hnsw_cfg* cfg = nullptr, int exchange = COLTT_EXCHANGE_AUTO) : dim_(dim), kind_(kind) {
    coltt_group_opts o{}; o.kind = kind; o.layout = layout; o.exchange = exchange;
    check(coltt_group_create(devices.data(), (int)devices.size(), dim, distance, quantization, cfg, &o, &h_));
  }
  ~Group() { if (h_) coltt_group_destroy(h_); }
  Group(const Group&) = delete;
  Group& operator=(const Group&) = delete;
  int ShardOf(uint64_t id) const { int32_t s = 0; check(coltt_group_shard_of(h_, id, &s)); return s; }   // sharding.ShardVertex(id, world)
  coltt_handle_t Member(int i) const { coltt_handle_t m = 0; check(coltt_group_member(h_, i, &m)); return m; }
  uint64_t Len() const { uint64_t n = 0; check(coltt_group_len(h_, &n)); return n; }
  // ChangedVertex (FLAT groups) / Insert (HNSW groups) for n vertices, row-major vectors; returns how many this process hosts
  uint64_t ChangedVertex(const std::vector<uint64_t>& ids, const std::vector<float>& vecs) {
    if (vecs.size() != ids.size() * dim_) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    uint64_t kept = 0; check(coltt_group_upsert(h_, ids.data(), vecs.data(), ids.size(), &kept)); return kept;
  }
  uint64_t Insert(const std::vector<uint64_t>& ids, const std::vector<float>& vecs, const std::vector<int32_t>& levels, uint32_t batch = 1) {
    if (vecs.size() != ids.size() * dim_ || levels.size() != ids.size()) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    uint64_t kept = 0; check(coltt_group_insert(h_, ids.data(), vecs.data(), levels.data(), ids.size(), batch, &kept)); return kept;
  }
  void Remove(const std::vector<uint64_t>& ids) { check(coltt_group_remove(h_, ids.data(), ids.size())); }
  // one query over the whole collection (rows ascending by (score, id)); select / mode: FLAT groups, ef: HNSW groups
  SearchResult Search(const Vector& query, unsigned k, int select = COLTT_SELECT_NEAREST, int mode = COLTT_MODE_EXACT, uint32_t ef = 0) const {
    if (query.size() != dim_) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    std::vector<uint64_t> ids(k); std::vector<float> sc(k); uint32_t n = 0;
    check(coltt_group_search(h_, query.data(), 1, k, select, mode, ef, ids.data(), sc.data(), &n));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  coltt_handle_t handle() const { return h_; }

 private:
  coltt_handle_t h_ = 0; uint32_t dim_; int kind_;
};


// Product quantiser (coltt_pq_*).  Parameters = models.ProductQuantizerParameters (pkg/models/hnsw_common.go:20-33);
// method names follow the call shape of playground/hnswpq_verification.go:90-105,154,190-199 (the package it drives, pkg/hnswpq, is not in
// the reference's tree).  distance = COLTT_PQ_COSINE / _EUCLIDEAN / _DOT: which pkg/distancepq function fills the query's table.
struct ProductQuantizerParameters { int NumCentroids = 256; int NumSubVectors = 8; int TriggerThreshold = 10000; };
class ProductQuantizer {
 public:
  ProductQuantizer(uint32_t dim, int distance, const ProductQuantizerParameters& p) : dim_(dim), params_(p) {
    check(coltt_pq_create(dim, distance, (uint32_t)p.NumSubVectors, (uint32_t)p.NumCentroids, &h_));
  }
  ~ProductQuantizer() { if (h_) coltt_pq_destroy(h_); }
  ProductQuantizer(const ProductQuantizer&) = delete;
  ProductQuantizer& operator=(const ProductQuantizer&) = delete;
  // training on a sample of n = sample.size() / dim vectors (n >= NumCentroids), deterministic Lloyd iterations
  void Fit(const std::vector<float>& sample, unsigned iterations = 8) {
    if (sample.size() % dim_) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    check(coltt_pq_train(h_, sample.data(), sample.size() / dim_, iterations));
  }
  void SetCodebooks(const std::vector<float>& cb) {
    if (cb.size() != (size_t)params_.NumCentroids * dim_) throw Error(COLTT_E_INVALID, "codebooks: [NumSubVectors][NumCentroids][dim / NumSubVectors] floats expected");
    check(coltt_pq_set_codebooks(h_, cb.data()));
  }
  std::vector<float> Codebooks() const { std::vector<float> cb((size_t)params_.NumCentroids * dim_); check(coltt_pq_get_codebooks(h_, cb.data())); return cb; }
  std::vector<uint8_t> Encode(const Vector& v) const {
    if (v.size() != dim_) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    std::vector<uint8_t> c((size_t)params_.NumSubVectors); check(coltt_pq_encode(h_, v.data(), 1, c.data())); return c;
  }
  void Insert(uint64_t id, const Vector& v) {
    if (v.size() != dim_) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    check(coltt_pq_upsert(h_, &id, v.data(), 1));
  }
  void InsertMany(const std::vector<uint64_t>& ids, const float* rows) { check(coltt_pq_upsert(h_, ids.data(), rows, ids.size())); }
  void Remove(const std::vector<uint64_t>& ids) { check(coltt_pq_remove(h_, ids.data(), ids.size())); }
  uint64_t Len() const { uint64_t n = 0; check(coltt_pq_len(h_, &n)); return n; }
  // the k nearest by the asymmetric distance, ascending by (score, id)
  SearchResult Search(const Vector& query, unsigned k) const {
    if (query.size() != dim_) throw Error(COLTT_E_INVALID, "Dim Length UnmatchdError");
    std::vector<uint64_t> ids(k); std::vector<float> sc(k); uint32_t n = 0;
    check(coltt_pq_search(h_, query.data(), 1, k, ids.data(), sc.data(), &n));
    SearchResult r(n);
    for (uint32_t i = 0; i < n; i++) r[i] = {ids[i], sc[i]};
    return r;
  }
  coltt_handle_t handle() const { return h_; }

 private:
  coltt_handle_t h_ = 0; uint32_t dim_; ProductQuantizerParameters params_;
};

}  // namespace coltt
