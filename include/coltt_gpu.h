/* coltt_gpu.h — C-ABI of libcoltt_gpu.so: the MI355X-native ANN search hot path of sjy-dv/coltt.
 *
 * Drop-in boundary.  The reference has no FFI for this path (it is pure Go + Go
 * assembly); these entry points are what a cgo shim binds in order to put the GPU behind the
 * reference's own Go interfaces.  Every function cites the reference interface it replaces.
 *
 * Conventions
 *   - plain C, no torch / C++ types; all handles are opaque uint64.
 *   - the caller owns every input and output buffer; the library copies inputs before returning
 *     (cgo: no Go pointer is retained, no callbacks into Go).
 *   - return value: 0 = ok, <0 = error class (COLTT_E_*); message via coltt_last_error() (thread-local).
 *     Nothing aborts or throws across the boundary.
 *   - all entry points are thread-safe (cgo calls arrive on arbitrary OS threads).
 *   - "*_device" variants take pointers that already live in this GPU's HBM (hipMalloc'd or a
 *     torch.Tensor.data_ptr()); they exist so resident data never crosses PCIe.  The library works on its own
 *     HIP stream: a device buffer handed in must be complete (its producer stream synchronised) before the call,
 *     and results are complete when the call returns.
 */
#ifndef COLTT_GPU_H
#define COLTT_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t coltt_handle_t;

enum { COLTT_OK = 0, COLTT_E_INVALID = -1, COLTT_E_EXISTS = -2, COLTT_E_NOT_FOUND = -3,
       COLTT_E_UNSUPPORTED = -4, COLTT_E_DEVICE = -5, COLTT_E_NOMEM = -6 };

/* edgepb.Distance (idl/proto/v4/edge.proto:70-73) */
enum { COLTT_COSINE = 0, COLTT_EUCLIDEAN = 1 };
/* distance.SpaceImpl.ManhattanDistance (pkg/distance/space.go:25-29,73-79; simd/cpp/avx.cpp:34-49): exposed by the reference's kernel
 * interface, used by none of its stores — served by coltt_distance_pairs only */
enum { COLTT_MANHATTAN = 2 };
/* edgepb.Quantization (idl/proto/v4/edge.proto:75-80).  NB the reference's "BF16" is IEEE binary16
 * (pkg/compresshelper/bf16.go:233-317 == float16.go:237-321) and its "F8" decodes to 8 distinct
 * values (float8.go:233-313); both are reproduced bit-for-bit. */
enum { COLTT_Q_NONE = 0, COLTT_Q_F16 = 1, COLTT_Q_F8 = 2, COLTT_Q_BF16 = 3 };
/* top-k direction.  REFERENCE = what edge.PriorityQueue really does: min-heap + pop-min keeps the K
 * LARGEST distances (edge/priority_queue.go:39-55), returned ascending (:57-69).  NEAREST = K smallest. */
enum { COLTT_SELECT_REFERENCE = 0, COLTT_SELECT_NEAREST = 1 };
/* FLAT arithmetic.  EXACT = the reference AVX summation order, bit-identical scores
 * (pkg/distance/simd/cpp/avx.cpp:15-32,51-75).  MFMA = matrix-core candidate generation followed by an
 * EXACT re-score of the survivors: candidates are kept within a margin of twice the proven error bound of
 * the approximate score, so the candidate set is a superset of the exact top-k and ids, ranks and score
 * bits EQUAL the EXACT mode's.  Served for cosine and Euclidean, f32 / 2-byte rows, 128 <= dim <= 4096;
 * anything else (f8 rows, smaller dims, the id-list scan) silently runs EXACT — same answers. */
enum { COLTT_MODE_EXACT = 0, COLTT_MODE_MFMA = 1 };

/* ---- process / device ------------------------------------------------------------------------ */
int coltt_init(int device);                 /* selects the HIP device for the calling process      */
int coltt_device_count(void);
const char* coltt_last_error(void);
const char* coltt_version(void);
/* The COLTT_* measurement / test knobs (INTEGRATION.md "Knobs") are read from the environment ONCE, into a process-wide snapshot,
 * when the library is first used; no search call reads the environment.  A program that changes one of them later calls this. */
int coltt_policy_reload(void);

/* ---- kernels exposed one-to-one (pkg/distance, pkg/compresshelper, pkg/sharding, pkg/distancepq) --- */
/* distance.Space.Distance(a,b) for n independent pairs: a,b are row-major [n][dim] host arrays
 * (pkg/distance/space.go:61-63,77-79,93-95; metric COLTT_COSINE, COLTT_EUCLIDEAN or COLTT_MANHATTAN).  order: 0 avx (default dispatch on AVX hosts), 1 sse, 2 native
 * (space.go:40-49). */
int coltt_distance_pairs(int metric, int order, const float* a, const float* b, size_t n, uint32_t dim,
                         float* out);
/* edge.Normalize / vectorindex.Normalize (edge/vectorstore.go:173-189; core/vectorindex/metadata.go:107-123) */
int coltt_normalize(const float* in, size_t n, uint32_t dim, float* out);
/* the same function for ONE vector on the host: no device, no allocation, cannot fail for valid pointers (what the Go layer's
 * vectorindex.Normalize / edge.Normalize call once per RPC; bit-identical to coltt_normalize and to the reference) */
int coltt_normalize_host(const float* in, uint32_t dim, float* out);
/* Quantization.Lower: compresshelper.Fromfloat32 / BF16Fromfloat32 / F8Fromfloat32 per element
 * (edge/f16_quantization.go:47-53; pkg/compresshelper/float16.go:124-126, bf16.go:120-122, float8.go:120-122) */
int coltt_quant_lower(int quant, const float* in, size_t n_elems, void* out_codes);
/* Float16.Float32 / BFloat16.Float32 / Float8.Float32 (float16.go:184-187, bf16.go:180-183, float8.go:180-183) */
int coltt_quant_raise(int quant, const void* codes, size_t n_elems, float* out);
/* sharding.ShardVertex (pkg/sharding/shard.go:34-41) */
int coltt_shard_vertex(const uint64_t* ids, size_t n, uint64_t shard_count, uint64_t* out);
/* distancepq: asm.Dot / asm.SquaredEuclideanDistance (pkg/distancepq/asm/dot.s:7-55, euclidean.s:7-65);
 * kind 0 dot, 1 squared-L2, 2 cosineDistance (1-dot), 3 dotProductDistance (-dot) (distance.go:36-42);
 * one query against n rows. */
int coltt_pq_float_scan(int kind, const float* query, const float* rows, size_t n, uint32_t dim, float* out);
/* hammingDistance / jaccardDistance (pkg/distancepq/distance.go:62-84); kind 0 hamming, 1 jaccard;
 * one query of `words` uint64 against n rows. */
int coltt_pq_bit_scan(int kind, const uint64_t* query, const uint64_t* rows, size_t n, uint32_t words, float* out);

/* ---- edge FLAT store: replaces {none,f16,f8,bf16}VecSpace behind edge.vectorspace
 *      (edge/vectorstore.go:30-49; constructors selected at edge/vectorstore.go:62-85) ------------- */
int coltt_flat_create(uint32_t dim, int metric, int quant, coltt_handle_t* out);
int coltt_flat_destroy(coltt_handle_t h);
int coltt_flat_reserve(coltt_handle_t h, uint64_t n_rows);
/* ChangedVertex, vector half (edge/none_vectorstore.go:86-101; f16_vectorstore.go:87-105): applies
 * Normalize (cosine) and Lower so the stored bits equal the reference's.  Existing ids are overwritten.
 * A vector whose length != dim is the caller's error (none_vectorstore.go:86-88) — dim is fixed here. */
int coltt_flat_upsert(coltt_handle_t h, const uint64_t* ids, const float* vecs, size_t n);
/* same, vectors already in HBM; ids == NULL means ids are first_id, first_id+1, ... (append-only fast path) */
int coltt_flat_upsert_device(coltt_handle_t h, const uint64_t* ids, uint64_t first_id, const float* d_vecs, size_t n);
/* RemoveVertex, vector half (edge/none_vectorstore.go:118-124).  Unknown ids are ignored as in Go's delete(). */
int coltt_flat_remove(coltt_handle_t h, const uint64_t* ids, size_t n);
int coltt_flat_len(coltt_handle_t h, uint64_t* out);
/* stored (lowered) bits of one vertex — what SaveVertex serialises (none_vectorstore.go:308-390) */
int coltt_flat_get(coltt_handle_t h, uint64_t id, void* out_row);
/* stored rows [first_slot, first_slot + n) in scan order, and their ids — the bulk form of coltt_flat_get (what SaveVertex
 * walks); either output may be NULL */
int coltt_flat_fetch_rows(coltt_handle_t h, uint64_t first_slot, uint64_t n, void* out_rows, uint64_t* out_ids);
/* VertexSearch for a batch of queries (edge/none_vectorstore.go:129-180; f16_vectorstore.go:131-186).
 * out_ids/out_scores are [nq][k]; out_counts[q] = min(k, len).  Rows ascending by (score, id). */
int coltt_flat_search(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, int select, int mode,
                      uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
int coltt_flat_search_device(coltt_handle_t h, const float* d_queries, size_t nq, uint32_t k, int select, int mode,
                             uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_counts);
/* how many <= 256-query groups went through the matrix cores since creation, and how many of those overflowed their candidate
 * list and were re-run in exact mode (adversarial data only; the answers are the exact mode's either way) */
int coltt_flat_stats(coltt_handle_t h, uint64_t* mfma_groups, uint64_t* mfma_fallbacks);
/* Running bounds of the stored ||row||^2 over EVERYTHING the store ever held (they are not recomputed on removal), and whether the cosine
 * matrix-core path is open: it is closed for a store that ever held a row with ||row||^2 outside [1/4, 4] (a zero vector, a loaded stream
 * that was never normalised) — such a store answers COLTT_MODE_MFMA batches through the exact scan: same answers, ~25x the time at batch
 * 256.  Nothing is logged when the latch closes; this is where a caller sees it.  An empty store reports NaN bounds. */
int coltt_flat_norm_bounds(coltt_handle_t h, float* out_min, float* out_max, int32_t* out_cosine_matrix_core_open);
/* Host only, no device: would a store of this metric, quantization and dimension whose stored ||row||^2 lie in [min_norm, max_norm] (the
 * bounds coltt_flat_norm_bounds reports) answer COLTT_MODE_MFMA batches through the matrix cores (1) or through the exact scan (0)?  The
 * same function the search calls — for tests and for callers that want to know before they load.  f8_expanded: the "f8" store keeps its
 * binary16 copy (cosine only; COLTT_F8_MFMA).  Batches of 1-4 queries take the one-launch kernel whatever this says. */
int coltt_flat_mfma_eligible_host(int metric, int quant, uint32_t dim, float min_norm, float max_norm, int f8_expanded);
/* searches of <= 4 queries and k <= 64 are served by ONE kernel launch whatever `mode` says (scan in exact order, per-wave and
 * per-block k best, selection by the last block to finish): the reference's one-query-per-RPC shape (edge/edge_search.go).  Same
 * answers as both modes; this counts them (COLTT_FLAT_ONE=0 in the environment turns the path off). */
int coltt_flat_one_launch_searches(coltt_handle_t h, uint64_t* out);
/* FilterableVertexSearch (edge/none_vectorstore.go:182-253): the candidate ids come from the roaring
 * index (pkg/inverted/search.go:113-119) on the Go side; ids not present are skipped (:201). */
int coltt_flat_search_ids(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, int select,
                          const uint64_t* cand_ids, size_t n_cand,
                          uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* the same with an explicit mode: COLTT_MODE_MFMA generates candidates on the matrix cores from the GATHERED rows (batches of
 * filtered queries; same ids, ranks and score bits as COLTT_MODE_EXACT, which coltt_flat_search_ids uses) */
int coltt_flat_search_ids_mode(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, int select, int mode,
                               const uint64_t* cand_ids, size_t n_cand,
                               uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* FilterableVertexSearch for a batch of queries with a candidate list EACH — the reference serves one filtered query per RPC, every
 * RPC with its own filter expression and therefore its own id list (edge/none_vectorstore.go:182-253; pkg/inverted/search.go:113-119).
 * List l is cand_ids[list_offsets[l] .. list_offsets[l+1]); query i is searched over list list_of[i] (list_of == NULL requires
 * n_lists == nq: query i uses list i).  Several queries may name one list; a list nobody names is ignored.  Row i of the outputs
 * ([nq][k] / [nq]) EQUALS coltt_flat_search_ids(h, query i, 1, k, select, its list, its length, ...) on the same store state: the same
 * count (min(k, live distinct candidates)), the same ids ascending by (score, id), the same f32 score bits; entries past the count are
 * unspecified.  Ids that are not stored are skipped, an id repeated inside a list is scored once, an empty list gives count 0 (the
 * other rows are served), an empty store gives all counts 0, nq == 0 is not an error.
 * Errors — all checked before anything runs, no output is written: COLTT_E_NOT_FOUND unknown handle; COLTT_E_INVALID for NULL queries /
 * outputs / list_offsets with nq > 0, NULL cand_ids while the lists are not all empty, list_offsets that decrease, list_of == NULL with
 * n_lists != nq, a list_of[i] >= n_lists (coltt_last_error names the first such i), a bad select; COLTT_E_UNSUPPORTED for k == 0 or
 * k > 2048, as coltt_flat_search answers.
 * Host pointers only.  The call holds the store's lock shared for its whole duration: coltt_flat_remove moves the last row into the
 * hole, so a row's position is stable only under the lock — which is also why there is no reusable FLAT filter handle: the lists are
 * translated per call, once per list (not once per query).  Exact-order arithmetic only (queries with different row sets share no
 * GEMM).  k <= 64: one translation, one upload, ONE scan launch over ragged (query group, list chunk) tiles and one selection launch
 * for the whole batch; larger k: the same answers list by list through the shared-list path, still in this one call. */
int coltt_flat_search_ids_batch(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, int select,
                                const uint64_t* cand_ids, const uint64_t* list_offsets /*[n_lists + 1]*/, size_t n_lists,
                                const uint32_t* list_of /*[nq], or NULL when n_lists == nq*/,
                                uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* coltt_flat_search_ids_batch calls served by the one-pass path and by the k > 64 path since creation, and the (query, row) pairs the
 * one-pass path scored (the sum over its queries of their live distinct candidates); any output may be NULL */
int coltt_flat_ids_batch_stats(coltt_handle_t h, uint64_t* out_one_pass_calls, uint64_t* out_fallback_calls, uint64_t* out_pairs);
/* Host only, no device: the tile plan the one-pass path launches for lists of list_lens[l] rows (after translation), the same code
 * the search calls — for tests.  Queries are ordered by list (out_query_order[nq]: entry -> query, stable) and cut into groups of at
 * most queries_per_tile that share a list; every list is cut into chunks of chunk_rows (a positive multiple of 32).  A tile is
 * {list, s0, s1, first query entry, number of queries}: rows [s0, s1) of the list against out_query_order[first .. first + number).
 * A list of length 0 has no tile.  *out_n_tiles is the number of tiles of the plan; at most cap are written, and a plan that does not
 * fit is COLTT_E_INVALID (with *out_n_tiles set, so the caller can size the buffer). */
int coltt_flat_ids_plan_host(const uint64_t* list_lens /*[n_lists]*/, size_t n_lists, const uint32_t* list_of /*[nq] or NULL*/, size_t nq,
                             uint32_t chunk_rows, uint32_t queries_per_tile, uint32_t* out_tiles /*[cap][5]*/,
                             uint32_t* out_query_order /*[nq]*/, uint64_t cap, uint64_t* out_n_tiles);

/* SaveVertex / LoadVertex (edge/none_vectorstore.go:308-516; f16_vectorstore.go:317-532 and the f8/bf16 twins): 16 shards
 * x {u64 count, count x {u64 key, u32 vecLen, vecLen x big-endian STORED code (f32 | u16 | u8), u32 metaCount, typed
 * pairs}}.  Vector codes go straight into the HBM rows (byte-swapped on the device, no re-normalisation); metadata is
 * opaque to the library: load reports each vertex's blob position in buf, save re-emits the blobs the caller passes
 * (meta_ids[i] -> meta_blobs[i], each starting with its u32 metaCount; others are written as empty maps). */
int coltt_flat_load_vertex(coltt_handle_t h, const uint8_t* buf, uint64_t len, uint64_t* out_n, uint64_t* out_ids,
                           uint64_t* out_meta_off, uint32_t* out_meta_len, uint64_t cap_n);
int coltt_flat_save_vertex(coltt_handle_t h, const uint64_t* meta_ids, const uint8_t* const* meta_blobs,
                           const uint32_t* meta_lens, uint64_t n_meta, uint8_t* out, uint64_t cap, uint64_t* out_len);

/* ---- experimental CFLAT: multi-vector weighted FLAT scan (experimental/multi_vector_vertex.go:60-137) -------------
 * A vertex carries n_fields f32 vectors ([n][n_fields][dim] on upload; every field is normalised for cosine, :65-67).
 * MultiVertexSearch: score = sum over included fields of scoreHelper(Distance(node[f], q[f])) * (float32(ratio[f])/100)
 * (:113-119); the K LARGEST scores are kept and returned DESCENDING by (score, id) (multi_priority_queue.go:46-77). */
int coltt_cflat_create(uint32_t dim, int metric, uint32_t n_fields, coltt_handle_t* out);
int coltt_cflat_destroy(coltt_handle_t h);
int coltt_cflat_len(coltt_handle_t h, uint64_t* out);
int coltt_cflat_upsert(coltt_handle_t h, const uint64_t* ids, const float* vecs, size_t n);
int coltt_cflat_remove(coltt_handle_t h, const uint64_t* ids, size_t n);
int coltt_cflat_search(coltt_handle_t h, const float* queries, const uint32_t* ratios, const uint8_t* include, size_t nq,
                       uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* MultiVertexSearch for nq independent requests: queries [nq][n_fields][dim], ratios [nq][n_fields], include [nq][n_fields].
 * Row i of out_* equals coltt_cflat_search(h, query i, ratios i, include i, 1, k, ...) on the same store: same count, same ids,
 * same order (descending by (score, id)), same f32 score bits. */
int coltt_cflat_search_batch(coltt_handle_t h, const float* queries, const uint32_t* ratios, const uint8_t* include, size_t nq,
                             uint32_t k, uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* the stored (for cosine: normalised) fields of one vertex, [n_fields][dim] f32; COLTT_E_NOT_FOUND for an unknown id */
int coltt_cflat_get(coltt_handle_t h, uint64_t id, float* out_fields);

/* ---- core HNSW: replaces *vectorindex.Hnsw (core/vectorindex/hnsw.go:43-54) --------------------- */
typedef struct coltt_hnsw_cfg {       /* hnswConfig defaults: hnsw_config.go:135-162 */
  int32_t m;                          /* 16 */
  int32_t m_max;                      /* -1 -> m */
  int32_t m_max0;                     /* -1 -> 2m */
  int32_t ef;                         /* 20 */
  int32_t ef_construction;            /* 200 */
  int32_t algo;                       /* 0 HnswSearchSimple, 1 HnswSearchHeuristic (hnsw_config.go:27-33) — both keep the k nearest —, or
                                         COLTT_HNSW_DIVERSE (2): NOT reference behaviour, see below */
  float level_multiplier;             /* -1 -> 1/ln(m) */
  int32_t extend_candidates;          /* must be 0: the reference's extend path is undefined */
  int32_t keep_pruned;                /* 1 (dead code in the reference) */
} coltt_hnsw_cfg;

/* COLTT_HNSW_DIVERSE — an opt-in neighbour selection the reference does NOT have: its selectNeighborsHeuristic (hnsw.go:399-447) never
 * compares a candidate with the neighbours already chosen, so both of its modes build a plain k-nearest graph.  This mode applies the
 * diversity test of the HNSW paper (Algorithm 4, as hnswlib runs it) in Insert and in pruneNeighbors-on-overflow: candidates ascending
 * by (distance, slot); a candidate is chosen iff no already chosen neighbour is closer to it than the base vertex is; keep_pruned re-adds
 * the rejected ones, nearest first.  Defined in oracle/coltt_oracle.cpp (select_diverse); GPU graph == that definition bit for bit.
 * Search is unchanged (Hnsw.Search over whatever graph was built).  A graph built this way is NOT the reference's graph: the Go drop-in
 * refuses the value unless the caller opts in (go/vectorindex). */
#define COLTT_HNSW_DIVERSE 2

typedef struct coltt_hnsw_stats {     /* per search call, summed over the batch */
  uint64_t n_dist;                    /* distance evaluations */
  uint64_t n_exp;                     /* expanded candidates on level 0 */
  uint64_t n_hops;                    /* greedy hops on upper levels */
  uint64_t n_visit_resets;            /* visited-set resets (0 => traversal identical to the oracle's) */
} coltt_hnsw_stats;

/* NewHnsw(dim, distancer, options...) (hnsw.go:56-73).  quant != NONE stores 2-/1-byte codes and
 * evaluates distances as the edge quantised stores do (decode both, f32 distance) — an extension the
 * reference's core does not have (BASELINE.json configs[4]). */
int coltt_hnsw_create(uint32_t dim, int metric, int quant, const coltt_hnsw_cfg* cfg, coltt_handle_t* out);
int coltt_hnsw_destroy(coltt_handle_t h);
int coltt_hnsw_get_cfg(coltt_handle_t h, coltt_hnsw_cfg* out);
/* Hnsw.RandomLevel() (hnsw.go:280-282) for a caller-supplied uniform draw u in (0,1) — the value the shim's
 * rand.Float32() returned (gomath/rand.go:42-44: -Log(u) * levelMultiplier; math.go:52-62: float32 log, Floor through
 * float64).  The reference draws from the auto-seeded global math/rand, so the draw itself stays on the Go side.
 * u <= 0 (the reference's +Inf -> undefined int) or u >= 1 is COLTT_E_INVALID. */
int coltt_hnsw_random_level(coltt_handle_t h, float u, int32_t* out_level);
/* Load a graph built elsewhere (the oracle, Hnsw.Load's stream, another shard): slot-major arrays.
 * vectors are raw (Normalize/Lower are applied here for cosine/quant, as Insert does, hnsw.go:105-107).
 * rows = sum(level+1); row r of slot s, level l holds nbr[row_offsets[r] .. row_offsets[r+1]).  */
int coltt_hnsw_bulk_load(coltt_handle_t h, uint64_t n, const uint64_t* ids, const int32_t* levels,
                         const uint8_t* deleted, const float* vectors, const int64_t* row_offsets,
                         const int32_t* nbr, const float* nbr_dist, int32_t entry_slot);
/* Hnsw.Insert(id, value, metadata, vertexLevel) (hnsw.go:104-167); COLTT_E_EXISTS = ItemAlreadyExistsError */
int coltt_hnsw_insert(coltt_handle_t h, uint64_t id, const float* vec, int32_t level);
/* n Inserts in id order; `batch` vertices are linked against a frozen graph at a time (batch==1 is the
 * reference's sequential semantics).  d_vecs lives in HBM; ids == NULL means first_id + i. */
int coltt_hnsw_insert_batch_device(coltt_handle_t h, const uint64_t* ids, uint64_t first_id, const float* d_vecs,
                                   const int32_t* levels, size_t n, uint32_t batch);
/* Hnsw.Remove(id) (hnsw.go:191-241); COLTT_E_NOT_FOUND = ItemNotFoundError */
int coltt_hnsw_remove(coltt_handle_t h, uint64_t id);
int coltt_hnsw_len(coltt_handle_t h, uint64_t* out);
/* Hnsw.Search(ctx, query, k) for a batch (hnsw.go:243-278): ef = max(cfg.ef or ef_override, k); rows
 * ascending by distance; empty index => counts 0, not an error (hnsw.go:249-251). */
int coltt_hnsw_search(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, uint32_t ef_override,
                      uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats);
int coltt_hnsw_search_device(coltt_handle_t h, const float* d_queries, size_t nq, uint32_t k, uint32_t ef_override,
                             uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_counts, coltt_hnsw_stats* stats);
/* ---- Filtered HNSW search: an allow-list of ids — an extension the reference does NOT have ---------------------------------------
 * The reference's Core.HybridSearch (core/core.go:760-836) runs an unfiltered Hnsw.Search for 3 k candidates, looks the filter's matches
 * up among them and then returns the first k - 1 unfiltered candidates anyway; even a corrected post-filter finds nothing at a selective
 * filter.  These entry points answer "the k nearest among these ids" on the GPU.
 *
 * FILTER.  Built from a list of ids against one index; it allows the vertices that hold those ids WHEN IT IS BUILT.  Duplicate ids count
 * once; unknown or already removed ids are ignored (*out_allowed = the vertices allowed).  Slots are insertion indices and are never
 * reused, so a filter stays valid across later Inserts (not allowed by it) and Removes (tombstoned vertices are never returned).
 * coltt_hnsw_load / coltt_hnsw_bulk_load renumber the index: a filter built before them is stale and searching with it is
 * COLTT_E_INVALID; so is using a filter with another index.  The filter lives on the index's device: a slot bitmap of ceil(slots / 32)
 * words and the list of allowed slots.  Creation and searches take the index's lock shared.
 *
 * WALK (COLTT_FILTER_WALK).  Hnsw.Search at walk breadth ef_walk (= max(ef_override or cfg.ef, k), as coltt_hnsw_search) with one
 * addition.  The greedy descent and the level-0 searchLevel are the unfiltered canonical walk (oracle/coltt_oracle.cpp:
 * search_level_canon: ascending-slot neighbour order, lowerBound sampled once per pop, keys (d bits, slot)), so n_dist / n_exp / n_hops
 * equal an unfiltered search at ef_walk.  An allowed set R of capacity k receives every LIVE ALLOWED vertex whose distance the level-0
 * walk holds: the level-0 entry point and every neighbour it evaluates, admitted to the walk's result set or not.  R = the k smallest of
 * those by (d bits, slot) — a pure top-k over a set, independent of when keys arrive.  The answer is R ascending; count = |R| <= k.
 *
 * EXACT (COLTT_FILTER_EXACT).  The k nearest live allowed vertices by the index's own distance, ascending by (score bits, slot): cosine
 * normalises the query, quantised indexes lower it (as coltt_hnsw_search does), a row's score bits equal the walk's evaluation of that
 * row, tombstones are tested at search time.
 *
 * AUTO (COLTT_FILTER_AUTO, the default).  With A = the filter's allowed count, n_live = coltt_hnsw_len and ef as in WALK:
 *   ef_need = ceil(ef * n_live / A),  ef_walk = min(4096, max(ef, ef_need));
 *   EXACT when ef_need > 4096 or A <= 32 * ef_walk, else WALK at ef_walk.
 * 32 is the walk's row evaluations per unit of ef (n_dist / ef ~ 4 040 / 128 on the headline collection): below it the scan reads no
 * more rows than the walk would, and has no dependent chain (measured crossover: DESIGN.md, "Filtered search").
 *
 * An empty filter or an empty index gives counts of 0 and is not an error.  Not served: collection groups (the walk over product-quantiser codes
 * takes the same filter objects: coltt_hnsw_pq_search_filtered and coltt_hnsw_pq_search_filtered_batch below).
 *
 * A FILTER PER QUERY (coltt_hnsw_search_filtered_batch).  filters[i] is query i's filter; row i equals
 * coltt_hnsw_search_filtered(hnsw, filters[i], query i, 1, k, ef_override, mode, ...) on the same index state: the same ids, the same
 * score bits, the same count (entries past the count are unspecified).  AUTO decides per query from that query's filter (n_live is read
 * once per call); out_paths[i] (may be NULL) = the path that single call takes.  A handle may repeat; an empty filter gives its row
 * count 0 and the other rows are served.  Every handle is checked before anything runs, with the single call's codes: NULL filters
 * (nq > 0), an unknown handle, a filter of another index, a stale filter; coltt_last_error() names the first bad position.  Stats:
 * n_dist, n_exp, n_hops, n_visit_resets and n_exact_rows are the sums of the single calls'; ef_walk is the largest over the queries that
 * walk (0 if none does); path is WALK or EXACT when every query takes that path and COLTT_FILTER_AUTO (0) when the batch is mixed.
 * The call holds every filter it reads: destroying one meanwhile is safe.  One call launches at most two walks, one scan and one merge. */
#define COLTT_FILTER_AUTO 0
#define COLTT_FILTER_WALK 1
#define COLTT_FILTER_EXACT 2
typedef struct coltt_hnsw_filter_stats {   /* per call, summed over the batch */
  uint64_t n_dist, n_exp, n_hops, n_visit_resets;   /* the walk's counters (coltt_hnsw_stats); 0 when EXACT served the call */
  uint32_t ef_walk;                        /* the walk's breadth; 0 when EXACT served the call */
  int32_t path;                            /* COLTT_FILTER_WALK or COLTT_FILTER_EXACT: what served the call (what AUTO chose);
                                              a batch with a filter per query whose queries took both: COLTT_FILTER_AUTO */
  uint64_t n_exact_rows;                   /* (query, row) pairs the exact path scored */
} coltt_hnsw_filter_stats;
int coltt_hnsw_filter_create(coltt_handle_t hnsw, const uint64_t* ids, size_t n, uint64_t* out_allowed, coltt_handle_t* out);
int coltt_hnsw_filter_destroy(coltt_handle_t filter);
int coltt_hnsw_search_filtered(coltt_handle_t hnsw, coltt_handle_t filter, const float* queries, size_t nq, uint32_t k,
                               uint32_t ef_override, int mode, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                               coltt_hnsw_filter_stats* stats);
int coltt_hnsw_search_filtered_batch(coltt_handle_t hnsw, const coltt_handle_t* filters /*[nq]*/, const float* queries, size_t nq,
                                     uint32_t k, uint32_t ef_override, int mode, uint64_t* out_ids, float* out_scores,
                                     uint32_t* out_counts, int32_t* out_paths /*[nq], may be NULL*/, coltt_hnsw_filter_stats* stats);

/* FILTERED SEARCH OVER THE PRODUCT-QUANTISED WALK (coltt_hnsw_pq_search_filtered).  The filter object is the one above; one filter for the whole call.
 *
 * WALK.  With ef_walk as below, the walk is exactly coltt_hnsw_pq_search's walk at ef_walk (further down: table distance d = S_lo + S_hi, the canonical
 * neighbour order, the stale lowerBound, bounded visiting, tombstoned neighbours skipped before anything else), so n_dist, n_exp and n_hops equal an
 * unfiltered coltt_hnsw_pq_search at that ef on the same index state.  Let C be the set of LIVE ALLOWED vertices among the level-0 entry point and every
 * listed neighbour of every vertex the level-0 walk expands — a listed neighbour counts whether or not it is fresh, under the bound, or admitted, so C
 * depends only on which vertices were expanded.  R = the cap smallest members of C by (d bits, slot), cap = ef_walk when rerank == 0, else
 * min(max(rerank, k), ef_walk).  Every member of R gets the index's exact distance (the re-rank of coltt_hnsw_pq_search); the answer is the k smallest by
 * (exact score bits, slot), count = min(k, |R|).  Stats: path = WALK, ef_walk as chosen, n_exact_rows = the sum of |R| over the queries,
 * n_visit_resets = 0.
 * EXACT.  The exact path above, unchanged: the result of coltt_hnsw_search_filtered(..., COLTT_FILTER_EXACT).
 * AUTO.  The rule above word for word (ef_need, ef_walk, EXACT when ef_need > 4096 or A <= 32 * ef_walk): one filter takes the same path through either
 * entry point.
 * Errors.  No codes attached: COLTT_E_INVALID as coltt_hnsw_pq_search, checked first for every mode; an unknown, foreign or stale filter: the codes of
 * coltt_hnsw_search_filtered; ef > 4096 or an LDS need above 160 KiB: COLTT_E_UNSUPPORTED.  An empty filter or an empty index gives counts of 0 and
 * no error; nq == 0 is not an error.  Host pointers only.  Not served: device pointers, collection groups.
 *
 * A FILTER PER QUERY (coltt_hnsw_pq_search_filtered_batch).  filters[i] is query i's filter; row i equals
 * coltt_hnsw_pq_search_filtered(hnsw, filters[i], query i, 1, k, ef_override_or_0, rerank, mode, ...) on the same index state: the same ids, the same exact
 * score bits, the same count (entries past the count are unspecified).  The path is decided per query from that query's own filter by the rule above
 * (n_live is read once per call); out_paths[i] (may be NULL) = the path that single call takes.  Each walking query walks at its own ef_walk with the
 * single call's capacity of R (ef_walk when rerank == 0, else min(max(rerank, k), ef_walk)); EXACT rows are served by the exact scan of
 * coltt_hnsw_search_filtered_batch.  Stats: n_dist, n_exp, n_hops and n_exact_rows are the sums of the single calls'; n_visit_resets is 0; ef_walk is the
 * largest over the queries that walk (0 if none does); path is WALK or EXACT when every query takes that path and COLTT_FILTER_AUTO (0) when the batch is
 * mixed.  A walk whose on-chip visited set fills up is run again over the byte map, as the single call re-runs itself, and counts once.
 * Errors, all before anything runs (no output is written): no codes attached: COLTT_E_INVALID, checked first; filters == NULL with nq > 0:
 * COLTT_E_INVALID; an unknown handle, a filter of another index, a stale filter: the single call's codes, coltt_last_error() names the first bad
 * position; an unknown mode, or k == 0 with nq > 0: COLTT_E_INVALID; ef > 4096, or a query whose walk needs more than 160 KiB of LDS:
 * COLTT_E_UNSUPPORTED.  Not errors: nq == 0; an empty filter (that row's count is 0, the other rows are served); an empty index.  A handle may repeat.
 * The call holds every filter it reads (destroying one meanwhile is safe) and takes the index's lock shared.  Host pointers only.  Not served: device
 * pointers, collection groups, a rerank per query. */
int coltt_hnsw_pq_search_filtered(coltt_handle_t hnsw, coltt_handle_t filter, const float* queries, size_t nq, uint32_t k, uint32_t ef_override_or_0,
                                  uint32_t rerank, int mode /* COLTT_FILTER_* */, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                  coltt_hnsw_filter_stats* stats);
int coltt_hnsw_pq_search_filtered_batch(coltt_handle_t hnsw, const coltt_handle_t* filters /*[nq]*/, const float* queries, size_t nq,
                                        uint32_t k, uint32_t ef_override_or_0, uint32_t rerank, int mode /* COLTT_FILTER_* */,
                                        uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                                        int32_t* out_paths /*[nq], may be NULL*/, coltt_hnsw_filter_stats* stats);

/* FILTER EXPRESSIONS: AND / OR / NOT over resident filters, evaluated on the device (coltt_hnsw_filter_eval).  The reference's callers hold an
 * inverted index of per-term bitmaps and combine them per request by an AND / OR tree (pkg/inverted/search.go:26-119: evaluateSingleFilter,
 * evaluateCompositeFilter, SearchWithExpression); here a term the caller keeps hot is one filter that stays on the device (a LEAF) and a
 * request's tree is a postfix programme over a table of leaves — no id list crosses the bus and no host loop runs per id.
 * Programme.  Postfix.  A value v >= 0 pushes leaves[v]; a negative value is one of the operators below.
 * Definition.  Let n_slots be the index's slot count at the call and live(s) = slot s is not tombstoned at the call.  Leaf L has bit s = its
 * stored bit when s < L's slot count (the index's when L was built), else 0.  The result allows exactly { s < n_slots : expr(s) and live(s) }
 * and is an ordinary filter, indistinguishable from coltt_hnsw_filter_create(hnsw, the ids of that set) on the same index state: the same
 * allowed count, the same bitmap words, the same ascending slot list — so every filtered entry point (the row walk, the walk over the
 * quantiser's codes, EXACT, AUTO, both _batch calls) gives the same ids, score bits, counts, paths and stats with either.  NOT and ALL
 * therefore see vertices inserted after their operand was built; AND / OR / ANDNOT of plain leaves do not.
 * Refresh without a mutable filter: "add these ids, drop those" is the programme  old create(added) OR create(dropped) ANDNOT.  Filters stay
 * immutable: no call changes a filter another thread is searching with.
 * coltt_hnsw_filter_eval_batch: output i equals coltt_hnsw_filter_eval of programme i = progs[prog_off[i] .. prog_off[i+1]) over the shared
 * leaf table, all under one index state (the lock is taken once).  Nothing is created if any programme or handle is bad; coltt_last_error()
 * names the first bad programme and position.  One call launches two kernels and makes one host round trip (the counts that size the slot
 * lists) whatever n_out is, and its outputs share two device allocations that are freed when the last of them is destroyed.
 * coltt_hnsw_filter_ids writes the allowed ids in ascending slot order (as built) into out_ids: min(cap, allowed) of them, *out_n = allowed;
 * the ids are gathered on the device.  coltt_hnsw_filter_info: the index the filter was built for, its allowed count and the slots it covers.
 * Errors (the codes of coltt_hnsw_search_filtered where they overlap).  Unknown index or leaf handle: COLTT_E_NOT_FOUND.  A leaf of another
 * index or a stale leaf, n_prog == 0, stack underflow, a programme that does not end with exactly one value on the stack, a leaf index
 * >= n_leaves, an unknown operator, NULL out: COLTT_E_INVALID.  Stack depth above 8, n_prog above 4096: COLTT_E_UNSUPPORTED.  Not errors: an
 * empty index (the result allows nothing), an empty result, a repeated leaf handle, n_out == 0.  coltt_hnsw_filter_prog_check_host applies
 * exactly the programme rules with no device (*out_depth, may be NULL: the deepest stack); the evaluation calls it.
 * The evaluation takes the index's lock shared and holds every leaf it reads: destroying one meanwhile is safe.  Host pointers only. */
#define COLTT_FOP_AND    (-1)   /* a b -> a & b            */
#define COLTT_FOP_OR     (-2)   /* a b -> a | b            */
#define COLTT_FOP_ANDNOT (-3)   /* a b -> a & ~b           */
#define COLTT_FOP_NOT    (-4)   /* a   -> live & ~a        */
#define COLTT_FOP_ALL    (-5)   /*     -> live             */
int coltt_hnsw_filter_eval(coltt_handle_t hnsw, const int32_t* prog, size_t n_prog, const coltt_handle_t* leaves, size_t n_leaves,
                           uint64_t* out_allowed, coltt_handle_t* out);
int coltt_hnsw_filter_eval_batch(coltt_handle_t hnsw, const int32_t* progs, const uint64_t* prog_off /*[n_out+1]*/, size_t n_out,
                                 const coltt_handle_t* leaves, size_t n_leaves, uint64_t* out_allowed /*[n_out], may be NULL*/,
                                 coltt_handle_t* out /*[n_out]*/);
int coltt_hnsw_filter_ids(coltt_handle_t filter, uint64_t* out_ids, uint64_t cap, uint64_t* out_n);
int coltt_hnsw_filter_info(coltt_handle_t filter, coltt_handle_t* out_index, uint64_t* out_allowed, uint64_t* out_slots);
int coltt_hnsw_filter_prog_check_host(const int32_t* prog, size_t n_prog, size_t n_leaves, uint32_t* out_depth);   /* no device */

/* ATTRIBUTE COLUMNS AND PREDICATES: comparison leaves produced on the device (coltt_hnsw_attr_set, coltt_hnsw_filter_eval_attr).  The
 * reference's filter language has six comparison operators (pkg/inverted/filter.go:24-31); for every one but OpEqual it walks every distinct
 * value of the field and ORs that value's bitmap (pkg/inverted/search.go:36-45).  A predicate such as price < 37.5 on a high-cardinality
 * field has no hot term to keep resident as a leaf; here a numeric field is a COLUMN beside the index, one value per slot, and a comparison
 * over it stands in a filter programme wherever a resident filter can.
 * Column.  Belongs to one index and lives on that index's device: an 8-byte value per slot (COLTT_ATTR_I64: int64_t, COLTT_ATTR_F64: double),
 * a "set" bitmap of one bit per slot, and the slots it covers = the index's slot count at the last coltt_hnsw_attr_set.  A slot never set, and
 * a slot at or past the coverage (a vertex inserted after the last attr_set), is UNSET; an unset slot satisfies no comparison, as a vertex
 * without the field is in no bitmap of that field in the reference.
 * coltt_hnsw_attr_set maps ids to live slots exactly as coltt_hnsw_filter_create does (dense ids and explicit ids); unknown and removed ids
 * are ignored, *out_applied (may be NULL) = the vertices set.  An id repeated within one call takes its LAST value.  A NaN value in an F64
 * column is COLTT_E_INVALID, checked for the whole call before anything is written (a departure from the reference, whose compareValues calls
 * NaN equal to everything).  The call grows the column to the index's capacity when the index has outgrown it.  Update in place: the
 * reference's Core.Update is Remove + Insert under the same id, which gives the vertex a NEW slot: that slot is unset until the caller sets
 * the id again.  coltt_hnsw_attr_get: out_values[i] (8 bytes each) and out_set[i] (1 / 0; either may be NULL) for ids[i]; an unknown or
 * removed id and an unset slot give value 0, flag 0.  coltt_hnsw_attr_info (every out may be NULL): the index, the type, the slots covered
 * and the slots that hold a value (those of vertices removed since included).
 * Staleness.  A column records the index's generation as a filter does: after coltt_hnsw_load, coltt_hnsw_bulk_load or a coltt_hnsw_compact
 * that renumbered the slots it is stale and every use but info and destroy is COLTT_E_INVALID; the caller sets it again by ids — or lists it
 * in coltt_hnsw_compact_carry, which renumbers it with the index ("HNSW compaction" below).
 * Locking.  attr_set takes the index's lock shared and the column's own lock exclusive and returns after its device work is complete;
 * attr_get and an evaluation hold the columns they read shared, so an evaluation sees a column wholly before or wholly after a concurrent
 * attr_set.  Destroying a column an evaluation holds is safe.
 * Predicate.  { column, op, reserved = 0, value }: the column's type decides which member of value is read (mixed int / float comparison
 * is the caller's conversion).  Predicate P over column C has bit s = set_C(s) and cmp(value_C[s], operand) when s is below C's covered slots,
 * else 0 — the rule a leaf has for the slots it does not cover.  I64 compares as signed 64-bit integers, never through a double; F64 as IEEE
 * doubles (-0.0 == +0.0, infinities ordered as usual).  COLTT_CMP_SET: the slot has a value; the operand is ignored.
 * Programme.  The language of "Filter expressions" above: a value v >= 0 pushes leaves[v] when v < n_leaves and predicate v - n_leaves
 * otherwise; the operators are COLTT_FOP_*; the rules are coltt_hnsw_filter_prog_check_host over n_leaves + n_preds leaves (the calls use
 * it).  Everything else is the definition above word for word: the result allows { s < n_slots : expr(s) and live(s) } and is an ordinary
 * filter, indistinguishable from coltt_hnsw_filter_create over the ids of that set — the same allowed count, bitmap words and ascending slot
 * list, so the same filter_ids, filter_info and every search answer, path and stat.  NOT and ALL see unset slots and newer vertices, a bare
 * predicate does not.  _eval_attr_batch: output i equals _eval_attr of programme i over the shared leaf and predicate tables under one index
 * state.  One call launches two kernels and makes one host round trip whatever n_out and n_preds are.
 * Errors, all before anything is created (the codes of coltt_hnsw_filter_eval where they overlap; coltt_last_error names the first bad
 * predicate or programme position).  Unknown index, leaf or column handle: COLTT_E_NOT_FOUND.  A column of another index, a stale column,
 * an unknown op, reserved != 0, a NaN operand of an F64 column (unless the op is COLTT_CMP_SET), NULL preds with n_preds > 0:
 * COLTT_E_INVALID.  Not errors: n_out == 0; n_preds == 0 (the call equals coltt_hnsw_filter_eval / _eval_batch); an empty index; an empty
 * result; a repeated column or predicate.  Host pointers only.
 * coltt_attr_cmp_host (no device) is the comparison itself, the function the kernel compiles: 1 or 0 for is_set && cmp(*value, *operand), or
 * COLTT_E_INVALID for an unknown type or op, a NaN operand or value of type F64, or a NULL operand / value where one is read (operand: every
 * op but SET; value: is_set != 0).
 * Not carried through Commit / Load (columns go stale, as filters do); through a compaction only by coltt_hnsw_compact_carry; no string
 * columns (dictionary-encode to I64). */
#define COLTT_ATTR_I64 0
#define COLTT_ATTR_F64 1
#define COLTT_CMP_EQ 0   /* the order of the reference's FilterOp, pkg/inverted/filter.go:24-31 */
#define COLTT_CMP_NE 1
#define COLTT_CMP_GT 2
#define COLTT_CMP_GE 3
#define COLTT_CMP_LT 4
#define COLTT_CMP_LE 5
#define COLTT_CMP_SET 6  /* the slot has a value; the operand is ignored */
typedef struct coltt_attr_pred {
  coltt_handle_t column;
  int32_t op;            /* COLTT_CMP_* */
  int32_t reserved;      /* 0 */
  union { int64_t i64; double f64; } value;   /* the operand, in the column's type */
} coltt_attr_pred;
int coltt_hnsw_attr_create(coltt_handle_t hnsw, int type, coltt_handle_t* out);
int coltt_hnsw_attr_destroy(coltt_handle_t column);
int coltt_hnsw_attr_set(coltt_handle_t column, const uint64_t* ids, const void* values /* n x 8 bytes, the column's type */, size_t n,
                        uint64_t* out_applied);
int coltt_hnsw_attr_get(coltt_handle_t column, const uint64_t* ids, size_t n, void* out_values, uint8_t* out_set);
int coltt_hnsw_attr_info(coltt_handle_t column, coltt_handle_t* out_index, int32_t* out_type, uint64_t* out_slots, uint64_t* out_set);
int coltt_hnsw_filter_eval_attr(coltt_handle_t hnsw, const int32_t* prog, size_t n_prog, const coltt_handle_t* leaves, size_t n_leaves,
                                const coltt_attr_pred* preds, size_t n_preds, uint64_t* out_allowed, coltt_handle_t* out);
int coltt_hnsw_filter_eval_attr_batch(coltt_handle_t hnsw, const int32_t* progs, const uint64_t* prog_off /*[n_out+1]*/, size_t n_out,
                                      const coltt_handle_t* leaves, size_t n_leaves, const coltt_attr_pred* preds, size_t n_preds,
                                      uint64_t* out_allowed /*[n_out], may be NULL*/, coltt_handle_t* out /*[n_out]*/);
int coltt_attr_cmp_host(int type, int op, const void* operand, const void* value, int is_set);   /* no device: 1, 0, or a negative error */

/* Capacity for n_slots vertices (and n_upper_rows upper-level adjacency rows; 0 = the expectation for this index's M) in ONE allocation per
 * array, before the inserts.  Optional — Insert grows the arrays by half their size when they are full — but an index whose final size is
 * known should reserve it: growth copies every array (30 GB of rows at 10 M x 768 f32), and arrays allocated once from an empty heap get the
 * largest contiguous physical fragments, which the random row reads of a search feel in their TLB miss rate. */
int coltt_hnsw_reserve(coltt_handle_t h, uint64_t n_slots, uint64_t n_upper_rows);

/* HNSW COMPACTION: reclaim the slots of removed vertices on the device (coltt_hnsw_compact) — an extension the reference does not have.
 * coltt_hnsw_remove only sets a tombstone: the vertex keeps its row, its derived rows, its adjacency rows and its id, other vertices may keep edges to
 * it, and every walk tests the tombstone bitmap per neighbour from then on.  The reference's write path makes that the normal case (Core.Update,
 * core/core.go:471-564, is Remove + Insert under the same id), so a collection updated in place only grows.  This call drops the tombstoned slots in
 * place, without a second copy of the collection and without the host.
 * Definition.  Let live(s) = slot s is not tombstoned and new(s) = the number of live slots below s.  After the call the index holds exactly the live
 * vertices, vertex s at slot new(s).  Its stored row bytes, norm, id, level and every derived per-slot datum (binary16 shadow, 8-bit shadow code row and
 * (scale, error norm), the quantiser's code row) are the bytes they were.  Each of its adjacency rows, level 0 and upper, is the old row with the
 * tombstoned entries dropped and the survivors renamed by new() — still ascending, padded with 0xffffffff — and the per-edge companions (stored
 * distances, neighbour norms, neighbour (scale, error norm) pairs) re-packed in step.  upper_off is recomputed (the upper rows of dead vertices are
 * gone), the entrypoint is new(entrypoint), no slot is tombstoned, the slot count is the live count.  Capacities are unchanged: nothing is reallocated,
 * nothing shrinks, the freed tail is what later Inserts fill.
 * new() is monotone, neighbour order and every tie-break of a search are "ascending slot" / (distance bits, slot), and every walk skips a tombstoned
 * neighbour before anything else — so ids, score bits, counts, n_dist, n_exp and n_hops of every search are what they were before the call, and the
 * stream of coltt_hnsw_commit (live vertices in ascending slot order per shard, dead neighbours skipped) is byte for byte the one committed before it.
 * Ids.  An index in dense-id mode (ids == NULL at every insert) that loses a slot becomes an explicit-id index; later
 * coltt_hnsw_insert_batch_device(ids == NULL, first_id, ...) calls keep working on it.
 * Derived state.  The neighbourhood blocks of the product-quantised walk are left stale, as coltt_hnsw_load leaves them: the next walk that reads them
 * rebuilds.  The slots are renumbered, so filters built before the call are stale (COLTT_E_INVALID), exactly as after coltt_hnsw_load: rebuild them
 * from their ids, or have them renumbered with the index by coltt_hnsw_compact_carry (below).  Slot-indexed tables of the caller (the metadata blobs of coltt_hnsw_commit) are renumbered by out_new_of_old.
 * No-op.  An index without tombstones is left alone: nothing is launched, filters stay valid, the stats report slots_after == slots_before and the map
 * is the identity.  An index whose vertices are all dead becomes the empty index and accepts Inserts afterwards.
 * out_new_of_old (may be NULL) receives new(s) for the slots s before the call, 0xffffffff for a tombstoned one; cap_map < the slot count with a
 * non-NULL pointer is COLTT_E_INVALID, checked before anything runs.  An index whose entrypoint is itself a tombstone while live vertices remain
 * (Remove elects the removed entrypoint's closest listed neighbour without asking whether it is alive, hnsw.go:197-217) is refused with
 * COLTT_E_UNSUPPORTED and left as it is: its walks start from a vertex that would be dropped.
 * How.  In place through a staging block of stage_bytes_or_0 bytes (0 = 64 MiB), allocated for the call and freed by it.  Destination rows are swept in
 * ascending chunks of max(64, stage_bytes / row bytes) rows per array; a chunk's sources are gathered whole into the block and then copied to their
 * destinations — new(s) <= s, so a chunk's destinations can only overlap its own sources or those of earlier chunks.  The slots below the first tombstone
 * do not move; their adjacency rows are re-packed where they are.  Besides the block the call allocates 4 bytes per live slot and upper row and 4 bytes per
 * 32 slots (the source lists and the per-word rank table the renaming reads); the plan itself is coltt_hnsw_compact_map_host over the host mirrors.
 * Locking and failure.  The call takes the index's lock exclusive: searches wait and then see the compacted index.  A refused allocation leaves the
 * index as it was (COLTT_E_NOMEM).  A device failure part-way leaves the EMPTY index, never a half-moved one, and returns the device error. */
typedef struct coltt_hnsw_compact_stats {
  uint64_t slots_before, slots_after;            /* slots_after == coltt_hnsw_len */
  uint64_t upper_rows_before, upper_rows_after;
  uint64_t edges_dropped;                        /* adjacency entries of live vertices that named a tombstoned slot, all levels */
  uint64_t rows_moved;                           /* live slots whose number changed */
  uint64_t bytes_moved;                          /* bytes the move kernels wrote, staging included */
  float    ms;                                   /* device time of the call (hipEvents on the mutation stream) */
} coltt_hnsw_compact_stats;
int coltt_hnsw_compact(coltt_handle_t h, uint64_t stage_bytes_or_0, uint32_t* out_new_of_old /*[cap_map], may be NULL*/, uint64_t cap_map,
                       coltt_hnsw_compact_stats* stats /*may be NULL*/);
/* host only, no device: the plan the call above uses.  del_bits: bit s % 32 of word s / 32 = slot s is tombstoned (NULL = none).  out_new_of_old [n_slots]
 * (dead = 0xffffffff), out_new_upper_off [live] indexed by NEW slot (0xffffffff for a vertex of level 0), the totals; every output may be NULL. */
int coltt_hnsw_compact_map_host(const uint32_t* del_bits, uint64_t n_slots, const int32_t* levels, uint32_t* out_new_of_old,
                                uint32_t* out_new_upper_off, uint64_t* out_live, uint64_t* out_upper_rows);
/* CARRYING RESIDENT FILTERS AND ATTRIBUTE COLUMNS THROUGH A COMPACTION (coltt_hnsw_compact_carry).  coltt_hnsw_compact leaves every filter and every
 * column stale; a column's values exist on the device only, and a hot term's filter costs a coltt_hnsw_filter_create to replay.  This call is the same
 * compaction — the same code path, the same stats, map, refusals and failure behaviour — after which the LISTED objects are valid at the new generation
 * under the same handles.  Objects that are not listed go stale as before.
 * Definition (live and new() as above).  A carried filter F' covers new(F.slots) slots — the live slots that were below F's coverage — has bit new(s)
 * = F's bit s for every live s below F.slots, allowed = |F and live|, and as its list the ascending slots of that set.  It agrees with
 * coltt_hnsw_filter_create(h, the ids of F and live) on the compacted index in every observable but coltt_hnsw_filter_info's out_slots: the allowed count,
 * coltt_hnsw_filter_ids, its value as a leaf of any programme, and every filtered entry point (the row walk, the walk over the quantiser's codes, EXACT,
 * AUTO, both _batch calls): ids, score bits, counts, paths and stats.  A carried column covers new(covered) slots, holds at slot new(s) the value and
 * the set bit slot s held, has n_set = |set and live| and keeps its type: coltt_hnsw_attr_get by id and every predicate over it answer for the live
 * vertices as before the call.
 * out_allowed[i] / out_set[i] (may be NULL) = the allowed count of filters[i] / the set count of columns[i] after the call.  A handle may appear more than
 * once in a list: the object is carried once.  carry->filters / columns: the distinct objects listed.
 * No-op and empty.  On an index without tombstones nothing is launched; the listed objects are validated all the same and stay valid.  On an index whose
 * vertices are all dead the result is the empty index, carried filters are valid empty filters and carried columns cover 0 slots.
 * Errors, all checked before anything changes.  An unknown handle: COLTT_E_NOT_FOUND.  An object of another index, a stale object, a NULL list with
 * n > 0: COLTT_E_INVALID; coltt_last_error() names the list and the position.  A short map and a tombstoned entrypoint are refused as by
 * coltt_hnsw_compact; the objects stay valid in both cases.
 * How.  One kernel (filter_carry.hpp) packs the bits at the tombstoned slots away — per bitmap word a pext by the word's live mask, placed at the bit
 * position the rank table names — for all carried filters and the "set" bitmaps of all carried columns in one launch; the filters' slot lists and the
 * counts come from the list kernel of coltt_hnsw_filter_eval; a column's values move with the index's own per-slot arrays through the staging block.
 * The carry reads what the compaction already holds on the device (tombstones, rank table, old_of_new): no id and no value crosses the bus.
 * Failure.  Every allocation of the carry (the new bitmaps and the lists, sized by the OLD allowed counts) is made before the first kernel:
 * COLTT_E_NOMEM leaves the index and the objects as they were.  The carried filters are written out of place into one slab per call and swapped into the
 * objects after the stream has synchronised; a device failure leaves the empty index, as coltt_hnsw_compact does, and the listed objects stale — no
 * filter is ever half-written.  A carried filter that was an output of a coltt_hnsw_filter_eval_batch leaves that call's shared allocations to its
 * siblings, which go stale unless they are listed too.
 * Locking.  Handles are looked up first, then the index's lock is taken exclusive, then every listed column's own lock exclusive (index before column: the
 * order of coltt_hnsw_attr_set).  coltt_hnsw_filter_info reads a filter under the index's shared lock: it sees the pair (allowed, slots) of before or of
 * after the call, never a mix.  Not carried: anything through Commit / Load / BulkLoad.  Not served: collection groups. */
typedef struct coltt_hnsw_carry_stats {
  uint64_t filters, columns;                             /* distinct objects carried */
  uint64_t bitmap_words, list_entries, column_values;    /* written for them */
  float ms;                                              /* device time of the carry launches alone */
} coltt_hnsw_carry_stats;
int coltt_hnsw_compact_carry(coltt_handle_t h, uint64_t stage_bytes_or_0,
                             const coltt_handle_t* filters, size_t n_filters, uint64_t* out_allowed /*[n_filters], may be NULL*/,
                             const coltt_handle_t* columns, size_t n_columns, uint64_t* out_set /*[n_columns], may be NULL*/,
                             uint32_t* out_new_of_old /*[cap_map], may be NULL*/, uint64_t cap_map,
                             coltt_hnsw_compact_stats* stats /*may be NULL*/, coltt_hnsw_carry_stats* carry /*may be NULL*/);
/* host only, no device: the definition of a carried bitmap.  bits: n_words words over the old slots (words past it read as 0); del_bits as above (NULL =
 * none).  out_bits [ceil(live / 32)]: bit new(s) = bit s for every live s; *out_allowed = the bits set in it; *out_live = live.  Every output may be NULL. */
int coltt_hnsw_carry_bits_host(const uint32_t* bits, uint64_t n_words, const uint32_t* del_bits, uint64_t n_slots,
                               uint32_t* out_bits, uint64_t* out_allowed, uint64_t* out_live);
/* the very kernels of the carry on caller-supplied bitmaps (host pointers), no index: n_bitmaps bitmaps of n_words words each, on the default device.
 * out_bits [n_bitmaps][ceil(live / 32)]; out_allowed [n_bitmaps]; out_lists (may be NULL): bitmap p's ascending new slots at out_lists + list_off[p]. */
int coltt_hnsw_carry_bits_device(const uint32_t* bits, uint64_t n_bitmaps, uint64_t n_words, const uint32_t* del_bits, uint64_t n_slots,
                                 uint32_t* out_bits, uint64_t* out_allowed /*[n_bitmaps]*/, uint32_t* out_lists /*may be NULL*/, const uint64_t* list_off);
/* Round 4: indexes whose rows are f32 / 2-byte codes of a byte length that is a multiple of 128 (dim 128, 256, 512, 768, 1024, 1536 ...)
 * keep a second, line-transposed copy of their rows (derived data, like the adjacency-carried norms) and evaluate the level-0
 * distances of a search with EIGHT lanes per row over it — whole 128-byte lines per load instruction — in the reference's summation
 * order: same ids, score bits and counters (coltt_amd/csrc/rows8.hpp).  COLTT_ROWS8=0 (at create) keeps an index without the copy,
 * COLTT_EV8=0 (per call) searches the pair-owned rows.  This reports how many search launches the eight-lane core served and whether
 * the copy is complete. */
int coltt_hnsw_rows8_searches(coltt_handle_t h, uint64_t* out_launches, int32_t* out_has_copy);
/* The level-0 row filter of f32 cosine indexes (an internal of the search kernels: same ids, score bits and traversal counters with and without it).
 * A line-transposed f32 cosine index with dim % 256 == 0 keeps a binary16 shadow of its rows (dim * 2 bytes per slot of device memory; none with
 * COLTT_ROW_SHADOW=0 at create, or when its allocation failed); once a traversal's result set is full, a neighbour the shadow PROVES to be no
 * closer than the set's worst member is rejected without reading its f32 row.  COLTT_ROW_FILTER = 0 / 1 forces it off / on per call, default: on for
 * row arrays far larger than the caches at ef <= 128 (the ef > 128 kernels take it with COLTT_ROW_FILTER=1 only).  Cumulative per index over the filtered
 * launches: evaluations the filter rejected, f32 rows read at level 0, shadow rows read (a neighbour the shadow cannot reject reads both), launches; *out_has_shadow = the index has its shadow.  Any out pointer may be NULL.
 * Two kinds of shadow exist.  The 8-BIT one (the default): one signed code byte per element (dim bytes per slot) with a scale and the exact norm of
 * what the codes miss per slot, the pair repeated per level-0 edge beside the neighbours' norms (8 bytes per slot + 8 bytes per edge); the bound charges
 * that stored error norm (coltt_amd/csrc/row_filter8.hpp).  The BINARY16 one: dim * 2 bytes per slot (row_filter.hpp).
 * COLTT_ROW_SHADOW_BITS = 8 / 16 / both (at create; default 8) says which an index keeps; COLTT_ROW_FILTER_BITS = 8 / 16 / 8i (per call) which a filtered
 * launch reads — 8i: the 8-bit shadow against the query quantised once per traversal, phase A an exact integer sum (row_filter8i.hpp); unset: 8i where the
 * index keeps the 8-bit shadow, else 16; the kind an index does not keep is served by the one it does.  *out_has_shadow is non-zero when any
 * shadow is kept: 8, 16 or 24 (both).  The shadow-row counter counts rows of whichever kind the launches read. */
int coltt_hnsw_row_filter_stats(coltt_handle_t h, uint64_t* out_rejected, uint64_t* out_f32_rows, uint64_t* out_shadow_rows, uint64_t* out_launches, int32_t* out_has_shadow);
/* The same for the greedy descent of the 8-bit row-filter walks (COLTT_ROW_FILTER_UPPER=1): cumulative shadow rows read, evaluations rejected and f32 rows
 * read at the levels ABOVE 0 (the entrypoint's own row is not among them), and the launches that ran the filtered descent.  The counters of
 * coltt_hnsw_row_filter_stats keep their level-0 meaning.  Any pointer may be NULL. */
int coltt_hnsw_row_filter_stats_ex(coltt_handle_t h, uint64_t* out_upper_shadow_rows, uint64_t* out_upper_rejected, uint64_t* out_upper_f32_rows, uint64_t* out_upper_launches);
/* The visited set of the level-0 walks (an internal of the search kernels: same answers and counters whichever serves).  Walks with ef <= 128 keep it in
 * LDS: an open-addressed table of 32-bit slots (32 KiB, four traversals per CU with 768-d f32 rows), or — the row-filter walk over the quantised query on an
 * index of at most 2^24 slots — an exact two-choice table of 16-bit entries with a 16-word stash (coltt_amd/csrc/vis16.hpp: 16 KiB, seven traversals per CU).
 * COLTT_VIS16=0 (per call) keeps the 32-bit table.  A traversal that outgrows either re-runs the call on the kernel that resets and re-seeds its table.
 * *out_kind: the visited set of the LAST search launch (0 HBM byte map, 32, 16; -1 before the first); *out_waves_per_cu / *out_grid: the traversals that launch
 * kept resident per CU and its grid; *out_launches16: launches on the 16-bit table so far; *out_stash_max / *out_visited_max: the fullest stash and the most
 * vertices one traversal of that last launch visited (0 unless it ran on the 16-bit table).
 * Any out pointer may be NULL. */
int coltt_hnsw_visited_stats(coltt_handle_t h, int32_t* out_kind, uint32_t* out_waves_per_cu, uint32_t* out_grid, uint64_t* out_launches16, uint64_t* out_stash_max, uint64_t* out_visited_max);
/* Which kernel a coltt_hnsw_search call launches, and how ("The search plan").  The search decides it once per call, in one function of the
 * index facts below, the knob snapshot (COLTT_*; coltt_policy_reload) and (nq, k, ef, force); coltt_hnsw_search_plan_host runs that function with no
 * device.  Nothing else about an index influences the plan. */
typedef struct coltt_hnsw_plan_facts {
  uint32_t dim; int32_t metric, quant;
  uint32_t m_max0;
  uint64_t stride;        /* bytes per stored row */
  uint64_t slots;
  int32_t r8;             /* the rows are stored line-transposed (COLTT_ROWS8 at create) */
  int32_t shadow8, shadow16;   /* the row-filter shadows the index keeps */
  int32_t vis_ready;      /* the HBM visited workspace exists (it is made by the first search that wants it) */
  uint32_t vis_regions;   /* ... and its regions: at most that many traversals of one launch */
} coltt_hnsw_plan_facts;
enum { COLTT_PLAN_LATENCY = 0, COLTT_PLAN_WALK2 = 1, COLTT_PLAN_ONE_WAVE = 2 };   /* coltt_hnsw_search_plan.family */
typedef struct coltt_hnsw_search_plan {
  int32_t family;         /* COLTT_PLAN_*: the 256-thread latency kernel, the hnsw_walk2.hpp walks, the one-wave walk */
  uint32_t ef, ef_pad;    /* max(ef, k), and rounded up to 64 */
  uint32_t hcap;          /* words of the 32-bit LDS visited table (64 with the HBM map) */
  uint64_t lds;           /* dynamic LDS bytes per workgroup */
  int32_t vis_kind;       /* the visited set: 0 HBM byte map, 32 / 16 the LDS table of 32-bit / 16-bit entries */
  int32_t w2;             /* COLTT_PLAN_WALK2: the walk variant (OPT bits | 8 deep profile), else -1 */
  uint32_t bloom_words;   /* ... its Bloom filter (HBM map only), 0 none */
  int32_t r8;             /* the kernel reads line-transposed rows */
  int32_t ev8;            /* COLTT_PLAN_WALK2: the eight-lane distance core */
  int32_t nt;             /* ... with non-temporal row loads */
  int32_t filter;         /* ... and the level-0 row filter: 0 none, 16, 8, 80 (8i) */
  uint32_t upper;         /* ... the filter launch's prologue: bit 0 filtered descent, bit 1 cacheable descent loads */
  uint32_t v16_bits, v16_limit;   /* vis_kind 16: log2 of the bucket count, the capacity rule's limit */
  uint32_t per_cu, grid;  /* traversals resident per CU by the grid rule; the grid before visited regions are leased */
  int32_t rows8_launch;   /* the launch counts in coltt_hnsw_rows8_searches */
  int32_t lat_seq, lat_helpers;   /* COLTT_PLAN_LATENCY: the sequential walk; helper workgroups per walking one (batches <= 8 queries) */
} coltt_hnsw_search_plan;
/* The plan of a search of nq queries for k answers at ef_override (>= 1; the index's default ef is not among the facts) over an index with these facts,
 * under the current knob snapshot.  force: 0, or what a call re-run after a visited-table overflow passes (1 not the latency kernel, 3 nor the walk over the
 * LDS table).  Returns what the search would: COLTT_E_UNSUPPORTED with its message for ef > 4096, LDS beyond 160 KiB, a walk variant that is not compiled. */
int coltt_hnsw_search_plan_host(const coltt_hnsw_plan_facts* facts, size_t nq, uint32_t k, uint32_t ef_override, int force, coltt_hnsw_search_plan* out);
/* The facts of a live index as its next search would read them. */
int coltt_hnsw_search_plan_facts(coltt_handle_t h, coltt_hnsw_plan_facts* out_facts);
/* Read-back of the 8-bit shadow for tests and tools: the codes of slots [first_slot, first_slot + n) in natural element order ([n][dim]), their
 * (scale, error norm) pairs ([n][2] floats) and the pairs carried by their level-0 adjacency rows ([n][m_max0][2] floats, zeros at empty positions).
 * Any out pointer may be NULL; COLTT_E_UNSUPPORTED when the index keeps no 8-bit shadow. */
int coltt_hnsw_fetch_shadow8(coltt_handle_t h, uint64_t first_slot, uint64_t n, int8_t* out_codes, float* out_meta, float* out_adj_meta);
/* The row filter's evaluator on chosen pairs, for tests and tools: one wave per query makes ONE call of the level-0 walk's own chunk evaluation
 * (hnsw_walk2.hpp: Group8FilterEval::filtered) on the up to 32 slots slots[q][0..32) (0xFFFFFFFF = no fresh neighbour at that position; a slot may
 * repeat) with lower_bound[q] and full_at_pop (0 | 1), over the shadow of `bits` (8 | 16) bits, with non-temporal row loads or not (nt 1 | 0).
 * The queries are prepared as coltt_hnsw_search prepares them.  out_r [nq][32]: what the walk would have been handed per position — the exact kernel's
 * distance, or the certified lower bound of a rejected neighbour, 0 where not fresh; out_qnorm [nq] / out_rnorm [nq][32]: the squared norms the bound
 * was formed from; out_counts [nq][3]: evaluations rejected, f32 rows read, shadow rows read.  lower_bound = +3e38 rejects nothing (every distance
 * exact), -3e38 rejects every certified pair (every bound).  COLTT_E_UNSUPPORTED when the index does not keep the shadow asked for. */
int coltt_hnsw_row_filter_probe(coltt_handle_t h, const float* queries, size_t nq, const uint32_t* slots, const float* lower_bound, int bits, int nt,
                                int full_at_pop, float* out_r, float* out_qnorm, float* out_rnorm, uint32_t* out_counts);
/* The same probe; bits may also be 80: the 8-bit shadow against the quantised query ("8i").  For that kind out_isum [nq][32] receives the integer sum
 * sum qh_i c_i phase A formed for every fresh position of a full_at_pop call (0 elsewhere) and out_qte [nq][2] the query's (scale t, error norm e_q);
 * both may be NULL and are left untouched by the other kinds. */
int coltt_hnsw_row_filter_probe_ex(coltt_handle_t h, const float* queries, size_t nq, const uint32_t* slots, const float* lower_bound, int bits, int nt,
                                   int full_at_pop, float* out_r, float* out_qnorm, float* out_rnorm, uint32_t* out_counts, int64_t* out_isum, float* out_qte);
/* graph export in the bulk_load layout (what Hnsw.Commit serialises, hnsw_commit.go:69-162).
 * Call with NULL arrays to get sizes.  With any array non-NULL, *n_slots / *n_rows / *n_edges are IN-OUT: on entry the
 * capacities of the caller's arrays (slots: ids, levels, deleted; rows + 1: row_offsets; edges: nbr, nbr_dist) — normally the
 * sizes the first call returned — and if an Insert has grown the index past them in between, nothing is written, the needed
 * sizes are returned and the call fails with COLTT_E_INVALID (retry with larger arrays). */
int coltt_hnsw_export(coltt_handle_t h, uint64_t* n_slots, uint64_t* n_rows, uint64_t* n_edges, uint64_t* ids,
                      int32_t* levels, uint8_t* deleted, int64_t* row_offsets, int32_t* nbr, float* nbr_dist,
                      int32_t* entry_slot);
/* Hnsw.Commit(w, header) (core/vectorindex/hnsw_commit.go:69-162): the reference's big-endian stream — [config
 * (hnsw_config.go:179-203), u32 dim, u8 distIdx], u64 entrypoint id, 16 FNV shards of {u64 id, i32 level, dim x f32,
 * metadata}, then per vertex {u64 id, per level (top down) u32 n, n x (u64 neighbour id, f32 distance)}; removed
 * vertices and edges to them are skipped.  meta_blobs[slot]/meta_lens[slot] = the vertex's Metadata already in stream
 * encoding (metadata.go:31-74: u16 pairs, {u8 keylen, key, u16 vallen, msgpack}); NULL => empty maps.  n_meta = the length
 * of both arrays: slots >= n_meta (vertices inserted after the caller sized them) get empty metadata, never an out-of-bounds read.
 * out == NULL => only *out_len is computed.
 * Quantised indexes: a binary16 ("f16" / "bf16") index writes the f32 values its codes stand for; coltt_hnsw_load into an index of the
 * same quantisation encodes them back to the same codes (binary16 encode(decode(c)) == c), so Commit -> Load is bit-identical and the
 * stream stays in the reference's format.  "f8" indexes return COLTT_E_UNSUPPORTED (that codec does not survive decode -> encode). */
int coltt_hnsw_commit(coltt_handle_t h, int header, const uint8_t* const* meta_blobs, const uint32_t* meta_lens, uint64_t n_meta,
                      uint8_t* out, uint64_t cap, uint64_t* out_len);
/* level of the entrypoint (what Hnsw.BytesSize needs, hnsw.go:476-490), -1 for an empty index: no device traffic */
int coltt_hnsw_entry_level(coltt_handle_t h, int32_t* out_level);
/* Hnsw.Load(r, header) (hnsw_commit.go:164-278) straight into the HBM layout: vectors are byte-swapped on the device
 * and NOT re-normalised (as in the reference).  Slots follow stream order.  out_ids / out_meta_off / out_meta_len
 * (capacity cap_n, may be NULL) receive each vertex's id and the position of its metadata blob inside buf, so the
 * caller can decode the msgpack values itself. */
int coltt_hnsw_load(coltt_handle_t h, int header, const uint8_t* buf, uint64_t len, uint64_t* out_n, uint64_t* out_ids,
                    uint64_t* out_meta_off, uint32_t* out_meta_len, uint64_t cap_n);
/* the adjacency exactly as it lives in HBM: adj0 [n][m_max0], upper_off [n], adjU [n_upper][m_max],
 * padded with 0xffffffff.  NULL arrays => sizes only. */
int coltt_hnsw_export_raw(coltt_handle_t h, uint64_t* n_slots, uint64_t* n_upper_rows, int32_t* entry_slot,
                          int32_t* entry_level, uint32_t* adj0, uint32_t* upper_off, uint32_t* adjU);
/* Hnsw.Get(id) / Hnsw.GetVertex(id) (hnsw.go:169-189): the stored (normalised / lowered) vector and the level of one live
 * vertex; COLTT_E_NOT_FOUND = ItemNotFoundError.  Either output may be NULL. */
int coltt_hnsw_get(coltt_handle_t h, uint64_t id, void* out_row, int32_t* out_level);
/* the same read-back for a slot range (bulk): the stored row bytes. */
int coltt_hnsw_fetch_rows(coltt_handle_t h, uint64_t first_slot, uint64_t n, void* out_rows);
/* last kernel timing of the handle's search stream, measured with hipEvents (milliseconds) */
int coltt_last_kernel_ms(coltt_handle_t h, float* out_ms);
/* the FLAT half of the call above (coltt_last_kernel_ms forwards a FLAT store's handle here); exported, hence declared */
int coltt_last_kernel_ms_flat(coltt_handle_t h, float* out_ms);

/* ---- collection groups: ONE collection partitioned over the GPUs of a node (BASELINE.json north_star) ----
 * The reference has no multi-device code; its sharding rule and merge shape are the ones `highCpu` uses for its 16
 * in-process map shards: vertex `id` lives on shard sharding.ShardVertex(id, world) (pkg/sharding/shard.go:34-41), every
 * shard is searched with a local queue, the local results are merged into one queue (edge/none_vectorstore.go:148-178).
 * SHARD layout: each member is an ordinary FLAT store / HNSW index on its own GPU; a search = per-member search on per-member
 * streams + ONE all-gather of packed {u64 id, f32 score, u32 valid} records (RCCL over xGMI; ncclCommInitAll in one process,
 * ncclCommInitRank with one process per GPU) + host-side merge in the canonical (score, id) order.  REPLICA layout: every
 * member holds everything, a query batch is split across members, nothing is exchanged.
 * RCCL is dlopen'ed on first use (no link-time dependency).  EXCHANGE_HOST / AUTO on a group whose members share one device
 * (RCCL refuses a device twice) moves the records through pinned host memory instead; the merge is on the host either way. */
enum { COLTT_GROUP_FLAT = 0, COLTT_GROUP_HNSW = 1 };
enum { COLTT_LAYOUT_SHARD = 0, COLTT_LAYOUT_REPLICA = 1 };
enum { COLTT_EXCHANGE_AUTO = 0, COLTT_EXCHANGE_RCCL = 1, COLTT_EXCHANGE_HOST = 2,
       COLTT_EXCHANGE_SHM = 3 /* processes of ONE box: POSIX shared memory + a process-shared barrier (coltt_shm_*) */ };
#define COLTT_UNIQUE_ID_BYTES 128
typedef struct coltt_group_opts {
  int32_t kind;               /* COLTT_GROUP_FLAT (edge vectorspace) | COLTT_GROUP_HNSW (core vectorindex)                  */
  int32_t layout;             /* COLTT_LAYOUT_SHARD | COLTT_LAYOUT_REPLICA                                                  */
  int32_t exchange;           /* COLTT_EXCHANGE_AUTO | _RCCL (fail if unavailable) | _HOST (one process) | _SHM (processes of a box) */
  int32_t world_size;         /* shards in the whole collection; 0 => n_devices (single process)                            */
  int32_t rank_base;          /* shard number of devices[0]; this process hosts shards rank_base .. rank_base+n_devices-1   */
  const uint8_t* unique_id;   /* COLTT_UNIQUE_ID_BYTES from coltt_group_unique_id(), the same in every process; NULL if one */
} coltt_group_opts;
int coltt_group_unique_id(uint8_t* out /*[COLTT_UNIQUE_ID_BYTES]*/);   /* ncclGetUniqueId, or random bytes when librccl is absent (SHM only) */
/* All-gather between the processes of one box through POSIX shared memory (host-only: no device call) — the transport of
 * COLTT_EXCHANGE_SHM groups, same packed records and same merge as the RCCL path; exported so the multi-process rendezvous,
 * barrier and chunking can be exercised without a GPU.  Every process passes the same unique_id, world and bytes_per_rank; it
 * hosts ranks rank_base .. rank_base + n_local - 1.  open() returns once all `world` ranks have attached (timeout:
 * COLTT_SHM_TIMEOUT_S, default 120 s).  allgather: local = n_local x bytes, out = world x bytes (rank-major), bytes <= bytes_per_rank
 * and equal in every process; collective — every process must make the same sequence of calls. */
int coltt_shm_open(const uint8_t* unique_id, int world, int n_local, int rank_base, uint64_t bytes_per_rank, coltt_handle_t* out);
int coltt_shm_allgather(coltt_handle_t h, const void* local, uint64_t bytes, void* out);
int coltt_shm_close(coltt_handle_t h);
int coltt_group_create(const int* devices, int n_devices, uint32_t dim, int metric, int quant, const coltt_hnsw_cfg* cfg,
                       const coltt_group_opts* opts, coltt_handle_t* out);
int coltt_group_destroy(coltt_handle_t h);
int coltt_group_info(coltt_handle_t h, int32_t* n_local, int32_t* world, int32_t* exchange_in_use, int32_t* rank_base);
/* the i-th local member's own handle (a coltt_flat_* / coltt_hnsw_* handle): device-resident ingest goes straight to it */
int coltt_group_member(coltt_handle_t h, int i, coltt_handle_t* out);
int coltt_group_shard_of(coltt_handle_t h, uint64_t id, int32_t* out_shard);
/* ChangedVertex (FLAT) / Insert (HNSW) routed by ShardVertex(id, world).  A process is OFFERED every vertex and keeps those
 * whose shard it hosts (*out_kept); a replica group gives every vertex to every member. */
int coltt_group_upsert(coltt_handle_t h, const uint64_t* ids, const float* vecs, size_t n, uint64_t* out_kept);
int coltt_group_insert(coltt_handle_t h, const uint64_t* ids, const float* vecs, const int32_t* levels, size_t n, uint32_t batch,
                       uint64_t* out_kept);
int coltt_group_remove(coltt_handle_t h, const uint64_t* ids, size_t n);
int coltt_group_len(coltt_handle_t h, uint64_t* out);   /* vertices hosted by THIS process (replica: of one member) */
/* VertexSearch / Hnsw.Search over the whole collection; results on the host, rows ascending by (score, id).
 * select / mode: FLAT only; ef_override: HNSW only.  In a multi-process group every process must make the same call. */
int coltt_group_search(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, int select, int mode, uint32_t ef_override,
                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* same, the query batch already resident on every local member's device: d_queries_per_member[i] -> [nq][dim] f32 */
int coltt_group_search_device(coltt_handle_t h, const float* const* d_queries_per_member, size_t nq, uint32_t k, int select, int mode,
                              uint32_t ef_override, uint64_t* out_ids, float* out_scores, uint32_t* out_counts);
/* Streaming form of a SHARD-layout search (the exchange "issued on a comm stream and overlapped with the next batch";
 * the shape of the reference's local-queue-then-merge scan, edge/none_vectorstore.go:148-178, with the merge taken off the critical
 * path).  _begin returns when every local member has searched the batch and the batch's exchange (pack + ONE all-gather + D2H on the
 * members' comm streams) and host merge have been queued behind the earlier batches'; _end blocks until the merged answers are in the
 * out arrays handed to _begin (they must stay valid until then — also when the group is destroyed with the batch in flight: destroy drains
 * its queue first) and returns that batch's status.  Exactly one of queries (host) /
 * d_queries_per_member (device) is non-NULL.  At most 3 batches are between their search and the end of their merge (a 4th _begin waits for a slot); a ticket that is never
 * ended is dropped when the group is destroyed.  Multi-process groups: every process
 * makes the same _begin calls in the same order (the collectives are issued in ticket order). */
int coltt_group_search_begin(coltt_handle_t h, const float* queries, const float* const* d_queries_per_member, size_t nq, uint32_t k,
                             int select, int mode, uint32_t ef_override, uint64_t* out_ids, float* out_scores, uint32_t* out_counts,
                             uint64_t* out_ticket);
int coltt_group_search_end(coltt_handle_t h, uint64_t ticket);
/* cumulative wall-clock of this group's finished shard-search batches: out4 = {batches, search_ms (stage A: the members' searches),
 * exchange_ms (pack + all-gather + D2H), merge_ms (host merge)} */
int coltt_group_timing(coltt_handle_t h, double* out4);
/* the host-side final merge on its own (no device needed): recs = [world][nq][k] packed 16-byte records {u64 id, f32 score,
 * u32 valid}, each shard's valid records ascending by (score, id); nearest != 0: the k smallest of the union, else the k
 * largest (edge.PriorityQueue semantics), both returned ascending. */
int coltt_group_merge_host(const void* recs, int world, size_t nq, uint32_t k, int nearest, uint64_t* out_ids, float* out_scores,
                           uint32_t* out_counts);
/* Failure of ONE rank's shard search (round 6).  The `valid` word of a packed record carries, above bit 0, the STATUS of the rank that
 * packed it (bits 8..31; 0 = its shard search succeeded).  A rank whose search fails still takes part in the batch's exchange, with a
 * block of status records: no peer is left waiting in an all-gather that never comes (the shape of a failing shard goroutine that still
 * signals its WaitGroup, edge/none_vectorstore.go:148-178), every rank returns an error for THAT batch (coltt_group_search /
 * _search_end) and the group stays usable.  The RCCL exchange is waited for with a deadline (COLTT_EXCHANGE_TIMEOUT_S, default 120 s):
 * a peer that died or never made the call turns into an error, and the group refuses further shard searches.
 * This helper (no device needed) returns the first rank of recs = [world][per] records whose block carries a status, or -1. */
int coltt_group_first_failed_rank_host(const void* recs, int world, size_t per, uint32_t* out_status);
/* sharding.ShardVertex on the host (pkg/sharding/shard.go:34-41): the routing rule of a group, no device needed */
uint64_t coltt_shard_vertex_host(uint64_t id, uint64_t shard_count);

/* ---- product-quantised store: codebooks, Encode, the per-query distance table and the ADC scan -----------
 * The reference declares the parameters (models.ProductQuantizerParameters, pkg/models/hnsw_common.go:20-33: NumCentroids in
 * [2,256] -> one uint8 code per sub-vector, NumSubVectors >= 2) and ships the arithmetic (pkg/distancepq/distance.go:30-42 over
 * asm/dot.s:7-55 and asm/euclidean.s:7-65), but the package that drove them (pkg/hnswpq, imported by
 * playground/hnswpq_verification.go:29; call shape :69-73, 90-105, 154, 190-199) is not in its tree.  These entry points are what a
 * binding of that package's quantiser would call; their results are DEFINED from the distancepq arithmetic (oracle/coltt_oracle.cpp,
 * "Product quantiser"):
 *   Encode  code[j] = argmin_c SquaredEuclideanDistance(x_j, centroid[j][c])  (strict <, c ascending, from MaxFloat32)
 *   LUT     lut[j][c] = distFn(q_j, centroid[j][c]);   score = sum over j = 0..m-1 of lut[j][code[j]], f32, in j order
 *   top-k   the k smallest by (score bits, id), ascending.
 * metric = which distancepq function is distFn: */
enum { COLTT_PQ_COSINE = 0 /* cosineDistance = 1 - Dot */, COLTT_PQ_EUCLIDEAN = 1 /* euclideanDistance = SQUARED L2 */,
       COLTT_PQ_DOT = 2 /* dotProductDistance = -Dot */ };
int coltt_pq_create(uint32_t dim, int metric, uint32_t num_subvectors, uint32_t num_centroids, coltt_handle_t* out);
int coltt_pq_destroy(coltt_handle_t h);
/* codebooks trained elsewhere: [num_subvectors][num_centroids][dim / num_subvectors] f32, row-major.  Refused once rows are stored. */
int coltt_pq_set_codebooks(coltt_handle_t h, const float* codebooks);
int coltt_pq_get_codebooks(coltt_handle_t h, float* out_codebooks);
/* the quantiser's training step on a sample of n >= num_centroids vectors (TriggerThreshold, hnsw_common.go:29-32): deterministic
 * Lloyd iterations — centroid c of sub-space j starts as sub-vector j of sample vector c; assignment = Encode; update = f32 sum in
 * sample order / float32(count); an empty cluster keeps its centroid.  Refused once rows are stored. */
int coltt_pq_train(coltt_handle_t h, const float* vecs, size_t n, uint32_t iterations);
/* Encode without storing: out_codes [n][num_subvectors] */
int coltt_pq_encode(coltt_handle_t h, const float* vecs, size_t n, uint8_t* out_codes);
/* store vectors (encoded on the GPU) / ready codes under ids; existing ids are overwritten; codes >= num_centroids are refused */
int coltt_pq_upsert(coltt_handle_t h, const uint64_t* ids, const float* vecs, size_t n);
int coltt_pq_upsert_device(coltt_handle_t h, const uint64_t* ids, uint64_t first_id, const float* d_vecs, size_t n);
int coltt_pq_upsert_codes(coltt_handle_t h, const uint64_t* ids, const uint8_t* codes, size_t n);
int coltt_pq_remove(coltt_handle_t h, const uint64_t* ids, size_t n);
int coltt_pq_len(coltt_handle_t h, uint64_t* out);
/* stored codes of rows [first_slot, first_slot + n) in scan order ([n][num_subvectors]) and their ids; either output may be NULL */
int coltt_pq_fetch_codes(coltt_handle_t h, uint64_t first_slot, uint64_t n, uint8_t* out_codes, uint64_t* out_ids);
/* the distance table of one query: out_lut [num_subvectors][num_centroids] */
int coltt_pq_lut(coltt_handle_t h, const float* query, float* out_lut);
/* ADC search of a batch: out_ids / out_scores [nq][k], out_counts[q] = min(k, len); rows ascending by (score, id) */
int coltt_pq_search(coltt_handle_t h, const float* queries, size_t nq, uint32_t k, uint64_t* out_ids, float* out_scores,
                    uint32_t* out_counts);
int coltt_pq_search_device(coltt_handle_t h, const float* d_queries, size_t nq, uint32_t k, uint64_t* d_out_ids, float* d_out_scores,
                           uint32_t* d_out_counts);
/* hipEvent times of the most recent search of this store: the whole call's kernels, and the scan launch over the last (largest)
 * segment alone — the kernel the roofline of the PQ leg is quoted on — with the number of rows that launch covered */
int coltt_pq_last_kernel_ms(coltt_handle_t h, float* out_search_ms, float* out_scan_ms, uint64_t* out_scan_rows);


/* ---- product-quantised HNSW: Hnsw.Search over the quantiser's codes with an exact re-rank ------------------------------------
 * The reference's only PQ call shape (playground/hnswpq_verification.go:69-105: hnswpq.NewProductQuantizationHnsw(), m = 32, 256
 * centroids, pre-train, Fit, search on the codes; UPDATE-LOG.md:190-194) — its package pkg/hnswpq is absent, so this is a DEFINITION
 * (oracle/coltt_oracle.cpp "Product-quantised HNSW"), assembled from the pinned pieces: the graph and traversal of
 * core/vectorindex/hnsw.go:243-278,320-389 and the quantiser above (pkg/distancepq/distance.go:30-42):
 *   codes    Encode(stored row as the index's distance sees it), one row-major code per slot, kept up to date by Insert / Load
 *   d(q, v)  = S_lo + S_hi, the f32 sums (j order, from +0.0) of float32(binary16(lut[j][code_v[j]])) over the first ceil(P / 2) and the remaining
 *            16-byte pieces of the code row (P = ceil(m / 16)): the quantiser's table over the query the index's distance sees (normalised /
 *            lowered), every entry rounded to binary16 (nearest even) — d only ranks, and a 2-byte table doubles the walk's resident traversals
 *   walk     Hnsw.Search with d in place of Distance() (entrypoint, upper levels, searchLevel(ef)); ties by (d bits, slot).  Bounded visiting:
 *            once the result set is full, a neighbour whose d is not below lowerBound is skipped before the visited test (it can never be
 *            admitted: the bound only falls) — the result sets are exactly the unbounded walk's, n_dist counts what passed the bound and was fresh
 *   re-rank  the min(max(rerank, k), |result set|) nearest by d (rerank = 0: the whole result set) are re-scored with the index's
 *            exact-order distance; the k smallest by (exact score, slot) are returned with their exact scores.
 * attach snapshots the (trained) quantiser's codebooks — later changes to `pq` do not reach the index — and encodes every stored row.
 * Supported: f32 / binary16 rows; euclideanDistance tables on any index, cosineDistance tables on a cosine index; <= 128 sub-vectors. */
int coltt_hnsw_pq_attach(coltt_handle_t hnsw, coltt_handle_t pq);
int coltt_hnsw_pq_info(coltt_handle_t hnsw, uint32_t* out_num_subvectors, uint32_t* out_num_centroids, int32_t* out_pq_metric, uint64_t* out_coded_slots);
/* codes of slots [first_slot, first_slot + n): out_codes [n][num_subvectors] */
int coltt_hnsw_pq_fetch_codes(coltt_handle_t hnsw, uint64_t first_slot, uint64_t n, uint8_t* out_codes);
/* Neighbourhood blocks of the product-quantised walk: how often they were built whole, how often and how far patched.
 * state: 0 = none (never built / off / not affordable), 1 = current, 2 = stale (the next walk that reads them rebuilds).
 * builds = whole-array builds, patches = mutating calls (Insert / InsertBatchDevice / Remove) that re-gathered the blocks of the level-0 rows they
 * rewrote instead of leaving the array stale, patched_rows = blocks those calls rewrote.  Outputs may be NULL. */
int coltt_hnsw_pq_nbr_stats(coltt_handle_t hnsw, uint64_t* out_builds, uint64_t* out_patches,
                            uint64_t* out_patched_rows, int32_t* out_state);
/* The blocks of slots [first_slot, first_slot + n) as the walk reads them: [n][mMax0][row_bytes], row_bytes = the code
 * row rounded up to 16 (padding and absent neighbours are zero).  COLTT_E_UNSUPPORTED unless state == 1.  Test / diagnostics. */
int coltt_hnsw_pq_fetch_nbr(coltt_handle_t hnsw, uint64_t first_slot, uint64_t n, uint8_t* out_blocks);
/* stats: n_dist = table-distance evaluations that counted (entrypoint, upper levels, every fresh neighbour while the set fills, afterwards the fresh
 * neighbours under the bound), n_exp / n_hops as Hnsw.Search; *out_n_exact (may be NULL) = exact re-rank evaluations */
int coltt_hnsw_pq_search(coltt_handle_t hnsw, const float* queries, size_t nq, uint32_t k, uint32_t ef_override_or_0, uint32_t rerank,
                         uint64_t* out_ids, float* out_scores, uint32_t* out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact);
int coltt_hnsw_pq_search_device(coltt_handle_t hnsw, const float* d_queries, size_t nq, uint32_t k, uint32_t ef_override_or_0, uint32_t rerank,
                                uint64_t* d_out_ids, float* d_out_scores, uint32_t* d_out_counts, coltt_hnsw_stats* stats, uint64_t* out_n_exact);

#ifdef __cplusplus
}
#endif
#endif /* COLTT_GPU_H */
