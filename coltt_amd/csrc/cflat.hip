// cflat.hip — experimental CFLAT on the GPU: multi-vector weighted FLAT scan
// (experimental/multi_vector_vertex.go:60-137).
//
// A vertex carries n_fields vectors; a query supplies one vector, a ratio and an include flag per field; the score is
//   sum over included fields of scoreHelper(Distance(node[f], q[f])) * (float32(ratio[f]) / 100)        (:113-119)
// accumulated in f32 in field order; the K LARGEST scores are kept and returned DESCENDING
// (experimental/multi_priority_queue.go:46-77).  Distances use the same pair-owned exact-order code as everything else.
// HBM layout: one row array per field sharing slots (rows[f][cap][stride], norms[f][cap]); removal swaps the last slot in.
#include <algorithm>

#include "common.hpp"
#include "exact.hpp"
#include "prep.hpp"
#include "select.hpp"

using namespace coltt;
using namespace coltt::dev;

namespace {

constexpr int CF_MAX_FIELDS = 8;

struct CFields { const uint8_t* rows[CF_MAX_FIELDS]; const float* norms[CF_MAX_FIELDS]; };

// scoreHelper (edge/edge_helper.go:143-148 / experimental twin)
template <int METRIC> __device__ __forceinline__ float score_helper(float d) {
  if constexpr (METRIC == M_COS) return ((2.0f - d) / 2.0f) * 100.0f;
  else return (float)fmax(0.0, (double)(100.0f - d));
}

// Candidate slots for the lanes `mine` of a wave that pass for ONE request (every lane calls it; `mine` is the same in all lanes that
// share the counter): the first of them adds their number to the request's counter and each takes its place behind the base.  One atomic
// per wave and request: the first segment of a chain has no threshold yet, and one atomic per ROW on a single address made that
// segment (65 526 serialised atomics per request, ~0.4 ms) most of a search.  The order inside the list is free: the selection sorts.
__device__ __forceinline__ uint32_t cflat_claim(uint32_t* counter, bool pass, unsigned long long mine, int lane) {
  const int leader = mine ? __builtin_ctzll(mine) : lane;
  uint32_t base = 0;
  if (pass && lane == leader) base = atomicAdd(counter, (uint32_t)__builtin_popcountll(mine));
  base = (uint32_t)__shfl((int)base, leader, 64);
  return base + (uint32_t)__builtin_popcountll(mine & ((1ull << lane) - 1ull));
}

// one query per launch (the reference RPC is single-query); each wave owns 32 vertices per iteration
template <int METRIC>
__global__ __launch_bounds__(256) void cflat_scan_kernel(CFields F, size_t stride, uint64_t n, int nf, int dim, const float* __restrict__ q_eff,
                                                        const float* __restrict__ qnorms, const float* __restrict__ weight /* ratio/100 or <0 = excluded */,
                                                        const uint32_t* __restrict__ thr, unsigned long long* __restrict__ cand,
                                                        uint32_t* __restrict__ cnt, uint32_t cap, uint64_t begin, uint64_t end) {
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [nf][dim]
  for (int i = threadIdx.x; i < nf * dim; i += blockDim.x) qs[i] = q_eff[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane & 1, p = lane >> 1;
  const uint32_t th = thr[0];
  const uint64_t ngroups = (end - begin + 31) / 32;
  for (uint64_t g = (uint64_t)blockIdx.x * 4 + wave; g < ngroups; g += (uint64_t)gridDim.x * 4) {
    uint64_t pos = begin + g * 32 + p;
    bool valid = pos < end;
    uint64_t slot = valid ? pos : begin;
    float score = 0.f;
    for (int f = 0; f < nf; f++) {
      const float w = weight[f];
      if (w < 0.f) continue;  // IncludeOrNot == false
      float rn = METRIC == M_COS ? F.norms[f][slot] : 0.f;
      float d = pair_distance<METRIC, Q_NONE, 4>(F.rows[f] + slot * stride, qs + (size_t)f * dim, dim, qnorms[f], rn, half);
      score += score_helper<METRIC>(d) * w;
    }
    uint32_t sk = score_key(score);
    const bool pass = valid && half == 0 && sk >= th;
    const uint32_t idx = cflat_claim(&cnt[0], pass, __ballot(pass), lane);
    if (pass && idx < cap) cand[idx] = ((unsigned long long)sk << 32) | (uint32_t)slot;
  }
}

// n = n_fields of one request, or nq * n_fields of a batch
__global__ void cflat_weights_kernel(const uint32_t* ratio, const uint8_t* include, uint64_t n, float* w) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = include[i] ? div_rn((float)ratio[i], 100.0f) : -1.0f;  // float32(Ratio) / 100
}

// ---------------------------------------------------------------------------------------------------
// A group of up to QB requests per pass over the rows (coltt_cflat_search_batch).  The prepared queries of the group sit in LDS as
// [QB][nf][dim]; a lane pair owns a row and reads each field of it ONCE for all QB requests: the accumulation is flat_scan_kernel's
// (four f32 accumulators per request and half, multiply then add, in element order) and the per-request arithmetic behind it —
// pair_hsum, scalar tail, cos_epilogue / go_sqrt, score_helper, two roundings into the score, in field order — is cflat_scan_kernel's,
// so a request's score bits do not depend on what else is in its group.
// The two lanes of a pair hold the same QB sums after pair_hsum; from there half h carries on with the requests 2j + h alone: the f64
// square roots and divisions of the epilogue, which cost more than the sums of a 128-wide field, are done once per pair, not twice.
// ---------------------------------------------------------------------------------------------------
template <int METRIC, int QB>
__global__ __launch_bounds__(256) void cflat_scan_batch_kernel(CFields F, size_t stride, int nf, int dim, const float* __restrict__ q_eff /* [nq_grp][nf][dim] */,
                                                              const float* __restrict__ qnorms /* [nq_grp][nf] */, const float* __restrict__ weight /* [nq_grp][nf] */,
                                                              int nq_grp, const uint32_t* __restrict__ thr, unsigned long long* __restrict__ cand,
                                                              uint32_t* __restrict__ cnt, uint32_t cap, uint64_t begin, uint64_t end) {
  static_assert(QB >= 2 && QB % 2 == 0, "the halves of a pair share the requests of a group");
  extern __shared__ __attribute__((aligned(16))) float qs[];  // [QB][nf][dim], dim % 4 == 0; unfilled requests are zero
  __shared__ float s_w[QB * CF_MAX_FIELDS], s_qn[QB * CF_MAX_FIELDS];  // [QB][CF_MAX_FIELDS]; weight -1 = excluded (and every unfilled slot)
  const int per = nf * dim;
  for (int i = threadIdx.x; i < QB * (per >> 2); i += blockDim.x)
    reinterpret_cast<f32x4*>(qs)[i] = i < nq_grp * (per >> 2) ? reinterpret_cast<const f32x4*>(q_eff)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < QB * CF_MAX_FIELDS; i += blockDim.x) {
    const int q = i / CF_MAX_FIELDS, f = i - q * CF_MAX_FIELDS;
    const bool filled = q < nq_grp && f < nf;
    s_w[i] = filled ? weight[q * nf + f] : -1.0f;
    s_qn[i] = filled ? qnorms[q * nf + f] : 0.f;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane & 1, p = lane >> 1;
  uint32_t fmask = 0;   // fields that some request of the group includes: the others are never read
  for (int f = 0; f < nf; f++)
    for (int q = 0; q < QB; q++) if (s_w[q * CF_MAX_FIELDS + f] >= 0.f) fmask |= 1u << f;
  uint32_t th[QB / 2];   // of this lane's requests 2j + half
#pragma unroll
  for (int j = 0; j < QB / 2; j++) th[j] = 2 * j + half < nq_grp ? thr[2 * j + half] : 0xffffffffu;
  const int n8 = dim >> 3;
  constexpr int U = 4;   // 16-byte loads per lane in flight (x2 with the prefetched next batch), as in flat_scan_kernel
  const int nb = n8 / U;
  const uint64_t ngroups = (end - begin + 31) / 32;
  for (uint64_t g = (uint64_t)blockIdx.x * 4 + wave; g < ngroups; g += (uint64_t)gridDim.x * 4) {
    const uint64_t pos = begin + g * 32 + p;
    const bool valid = pos < end;
    const uint64_t slot = valid ? pos : begin;
    float score[QB / 2];
#pragma unroll
    for (int j = 0; j < QB / 2; j++) score[j] = 0.f;
    for (int f = 0; f < nf; f++) {
      if (!((fmask >> f) & 1u)) continue;
      const uint8_t* row = F.rows[f] + slot * stride;
      const float* qf = qs + (size_t)f * dim;   // request q's vector of this field: qf + q * per
      float rn = 0.f;
      if constexpr (METRIC == M_COS) rn = F.norms[f][slot];
      f32x4 acc[QB];
#pragma unroll
      for (int q = 0; q < QB; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 cur[U], nxt[U];
      if (nb > 0) {
#pragma unroll
        for (int u = 0; u < U; u++) cur[u] = load_raw4<Q_NONE>(row, 8 * u + 4 * half);
      }
      for (int b = 0; b < nb; b++) {
        if (b + 1 < nb) {
#pragma unroll
          for (int u = 0; u < U; u++) nxt[u] = load_raw4<Q_NONE>(row, 8 * ((b + 1) * U + u) + 4 * half);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          const float* qp = qf + 8 * (b * U + u) + 4 * half;
          const f32x4 rc = cur[u];
#pragma unroll
          for (int q = 0; q < QB; q++) {
            f32x4 qq = *reinterpret_cast<const f32x4*>(qp + q * per);
            if constexpr (METRIC == M_COS) { f32x4 pr = qq * rc; acc[q] = acc[q] + pr; }
            else { f32x4 d = qq - rc; f32x4 pr = d * d; acc[q] = acc[q] + pr; }
          }
        }
#pragma unroll
        for (int u = 0; u < U; u++) cur[u] = nxt[u];
      }
      for (int t = nb * U; t < n8; t++) {
        const f32x4 r = load4<Q_NONE>(row, 8 * t + 4 * half);
        const float* qp = qf + 8 * t + 4 * half;
#pragma unroll
        for (int q = 0; q < QB; q++) {
          f32x4 qq = *reinterpret_cast<const f32x4*>(qp + q * per);
          if constexpr (METRIC == M_COS) { f32x4 pr = qq * r; acc[q] = acc[q] + pr; }
          else { f32x4 d = qq - r; f32x4 pr = d * d; acc[q] = acc[q] + pr; }
        }
      }
      float sum[QB / 2];
#pragma unroll
      for (int j = 0; j < QB / 2; j++) {   // every lane takes part in every pair_hsum (DPP): nothing below this loop may run before it
        const float s0 = pair_hsum(acc[2 * j], half), s1 = pair_hsum(acc[2 * j + 1], half);
        sum[j] = half ? s1 : s0;
      }
#pragma unroll
      for (int j = 0; j < QB / 2; j++) {
        const int q = 2 * j + half;
        float s = sum[j];
        for (int e = n8 * 8; e < dim; e++) {  // scalar tail
          const float r = load1<Q_NONE>(row, e);
          if constexpr (METRIC == M_COS) s += qf[q * per + e] * r;
          else { float d = qf[q * per + e] - r; s += d * d; }
        }
        const float w = s_w[q * CF_MAX_FIELDS + f];
        if (w < 0.f) continue;  // IncludeOrNot == false for this request: its query vector (NaN, Inf, anything) never reaches the score
        float d;
        if constexpr (METRIC == M_COS) d = cos_epilogue(s, s_qn[q * CF_MAX_FIELDS + f], rn);
        else d = go_sqrt(s);
        score[j] += score_helper<METRIC>(d) * w;
      }
    }
#pragma unroll
    for (int j = 0; j < QB / 2; j++) {
      const int q = 2 * j + half;
      const uint32_t sk = score_key(score[j]);
      const bool pass = valid && q < nq_grp && sk >= th[j];
      const unsigned long long m = __ballot(pass);
      if (!m) continue;   // wave-uniform
      const uint32_t idx = cflat_claim(&cnt[q], pass, m & (half ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull), lane);   // even lanes: request 2j, odd: 2j + 1
      if (pass && idx < cap) cand[(size_t)q * cap + idx] = ((unsigned long long)sk << 32) | (uint32_t)slot;
    }
  }
}

struct CFlat : Object {
  uint32_t dim = 0, nf = 0; int metric = 0; size_t stride = 0;
  uint64_t n = 0, cap = 0;
  DevBuf rows[CF_MAX_FIELDS], norms[CF_MAX_FIELDS], ids;
  std::unordered_map<uint64_t, uint32_t> id2slot; std::vector<uint64_t> h_ids;
  hipStream_t stream = nullptr;
  DevBuf w_raw, w_q, w_qn, w_misc, w_cand, w_out_ids, w_out_sc, w_out_cnt;
  DevBuf w_field, w_slots;   // bulk upsert: one gathered field of a chunk, and its slot | source-row lists
  DevBuf w_w, w_out;         // batch search: the weights [nq][nf], and ids | scores | counts packed for one copy back
  ~CFlat() override { if (stream) (void)hipStreamDestroy(stream); }
  int reserve(uint64_t need) {
    if (need <= cap) return COLTT_OK;
    uint64_t nc = std::max<uint64_t>({need, cap + cap / 2, 1024});
    for (uint32_t f = 0; f < nf; f++) { COLTT_TRY(rows[f].reserve(nc * stride, true, stream)); COLTT_TRY(norms[f].reserve(nc * 4, true, stream)); }
    COLTT_TRY(ids.reserve(nc * 8, true, stream));
    cap = nc;
    return COLTT_OK;
  }
  CFields fields() const {
    CFields F{};
    for (uint32_t f = 0; f < nf; f++) { F.rows[f] = rows[f].as<uint8_t>(); F.norms[f] = norms[f].as<float>(); }
    return F;
  }
};

// strided gather of one field out of the [..][nf][dim] upload: row j of `out` is field f of upload row src[j]
__global__ void cflat_take_field_kernel(const float* __restrict__ all, const uint32_t* __restrict__ src, uint64_t n, int nf, int f, int dim, float* __restrict__ out) {
  uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * (uint64_t)dim) return;
  uint64_t j = t / dim; int e = (int)(t - j * dim);
  out[t] = all[((uint64_t)src[j] * nf + f) * (uint64_t)dim + e];
}

constexpr size_t CF_UPSERT_CHUNK_BYTES = 64u << 20;   // of raw vectors per upload

// Requests per pass over the rows, and the LDS their query tile may take: the largest width of {2, 4, 8, 16} whose tile
// width x n_fields x dim x 4 bytes fits the budget; a request that does not fit even twice goes through cflat_scan_kernel, one at a
// time.  Measured: profiles/cflat_batch.md.
constexpr int CF_QB_MAX = 16;
constexpr size_t CF_TILE_BUDGET = 128 * 1024;
inline int cflat_group_width(size_t per_bytes) {
  for (int qb = CF_QB_MAX; qb >= 2; qb >>= 1)
    if ((size_t)qb * per_bytes <= CF_TILE_BUDGET) return qb;
  return 1;
}

struct CScanArgs {
  const float* q_eff; const float* qn; const float* w; int g;   // the g prepared requests of a group
  uint32_t* cnt; uint32_t* thr; unsigned long long* cand; uint32_t cap;
};

template <int METRIC, int QB>
int launch_scan_batch(CFlat* c, const CFields& F, const CScanArgs& a, uint32_t grid, uint64_t b, uint64_t e) {
  const size_t lds = (size_t)QB * c->nf * c->dim * 4;
  auto kern = cflat_scan_batch_kernel<METRIC, QB>;
  if (lds > 32 * 1024) COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, 256, lds, c->stream>>>(F, c->stride, (int)c->nf, (int)c->dim, a.q_eff, a.qn, a.w, a.g, a.thr, a.cand, a.cnt, a.cap, b, e);
  return COLTT_OK;
}
template <int METRIC>
int launch_scan_one(CFlat* c, const CFields& F, const CScanArgs& a, uint32_t grid, uint64_t b, uint64_t e) {
  const size_t lds = (size_t)c->nf * c->dim * 4;
  auto kern = cflat_scan_kernel<METRIC>;
  if (lds > 48 * 1024) COLTT_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  kern<<<grid, 256, lds, c->stream>>>(F, c->stride, c->n, (int)c->nf, (int)c->dim, a.q_eff, a.qn, a.w, a.thr, a.cand, a.cnt, a.cap, b, e);
  return COLTT_OK;
}
// rows [b, e) against the a.g requests of a group: the single-request kernel for one, else the narrowest batch instance that holds them
template <int METRIC>
int launch_scan(CFlat* c, const CFields& F, const CScanArgs& a, uint64_t b, uint64_t e) {
  const uint64_t groups = (e - b + 31) / 32;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + 3) / 4, 2048);
  if (a.g <= 1) COLTT_TRY(launch_scan_one<METRIC>(c, F, a, grid, b, e));
  else if (a.g <= 2) COLTT_TRY((launch_scan_batch<METRIC, 2>(c, F, a, grid, b, e)));
  else if (a.g <= 4) COLTT_TRY((launch_scan_batch<METRIC, 4>(c, F, a, grid, b, e)));
  else if (a.g <= 8) COLTT_TRY((launch_scan_batch<METRIC, 8>(c, F, a, grid, b, e)));
  else COLTT_TRY((launch_scan_batch<METRIC, 16>(c, F, a, grid, b, e)));
  COLTT_HIP(hipGetLastError());  // a refused launch (LDS tile too large) must not read as an empty answer
  return COLTT_OK;
}

// One group of prepared requests over the whole store: segments of at most cap - k vertices can never overflow a candidate list; the
// selection after each segment hands every request's own threshold to the next.  Results ASCENDING in out_*[g][k]; nothing here waits.
int search_group(CFlat* c, const CFields& F, const CScanArgs& a, uint32_t* ovf, uint32_t k, uint64_t* oi, float* os, uint32_t* oc) {
  init_group_kernel<<<1, 256, 0, c->stream>>>(a.cnt, a.thr, ovf, 0);
  const uint64_t seg = a.cap - std::min<uint32_t>(k, a.cap / 2);
  for (uint64_t b = 0; b < c->n || b == 0; b += seg) {
    const uint64_t e = std::min<uint64_t>(c->n, b + seg);
    if (e > b) {
      if (c->metric == COLTT_COSINE) COLTT_TRY(launch_scan<M_COS>(c, F, a, b, e));
      else COLTT_TRY(launch_scan<M_L2>(c, F, a, b, e));
    }
    flat_select_kernel<<<a.g, 256, 0, c->stream>>>(a.cand, a.cnt, a.thr, a.cap, k, 0, c->ids.as<uint64_t>(), 0, ovf, oi, os, oc);
  }
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

}  // namespace

extern "C" {

int coltt_cflat_create(uint32_t dim, int metric, uint32_t n_fields, coltt_handle_t* out) {
  if (!out) return fail(COLTT_E_INVALID, "cflat_create: out is NULL");
  if (dim == 0 || dim > 4096 || dim % 4) return fail(COLTT_E_INVALID, "cflat_create: dim %u must be a multiple of 4 in [4,4096]", dim);
  if (n_fields == 0 || n_fields > CF_MAX_FIELDS) return fail(COLTT_E_INVALID, "cflat_create: n_fields %u outside [1,%d]", n_fields, CF_MAX_FIELDS);
  if (metric != COLTT_COSINE && metric != COLTT_EUCLIDEAN) return fail(COLTT_E_INVALID, "cflat_create: bad metric %d", metric);
  if ((size_t)n_fields * dim * 4 > 150 * 1024) return fail(COLTT_E_UNSUPPORTED, "cflat_create: n_fields x dim too large for the LDS query tile");
  COLTT_DEVICE(-1);
  auto c = std::make_shared<CFlat>();
  c->dim = dim; c->nf = n_fields; c->metric = metric; c->stride = ((size_t)dim * 4 + 15) & ~(size_t)15;
  COLTT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  c->device = default_device();
  *out = Registry::get().add(c);
  return COLTT_OK;
}

int coltt_cflat_destroy(coltt_handle_t h) {
  if (!Registry::get().erase(h)) return fail(COLTT_E_NOT_FOUND, "cflat_destroy: unknown handle");
  return COLTT_OK;
}

int coltt_cflat_len(coltt_handle_t h, uint64_t* out) {
  auto c = lookup<CFlat>(h);
  if (!c || !out) return fail(COLTT_E_NOT_FOUND, "cflat_len: unknown handle");
  WriteLock g(c->rw);
  *out = c->n;
  return COLTT_OK;
}

/* ChangedVertex (experimental/multi_vector_vertex.go:60-75): vecs is [n][n_fields][dim]; every field is normalised for cosine.
 * The reference takes one vertex per call; n of them in input order leave the store that this leaves: a new id takes the next slot
 * when it first appears, and the last occurrence of a repeated id is the one stored. */
int coltt_cflat_upsert(coltt_handle_t h, const uint64_t* ids, const float* vecs, size_t n) {
  auto c = lookup<CFlat>(h);
  if (!c) return fail(COLTT_E_NOT_FOUND, "cflat_upsert: unknown handle");
  if (n == 0) return COLTT_OK;
  if (!ids || !vecs) return fail(COLTT_E_INVALID, "cflat_upsert: NULL input");
  WriteLock g(c->rw);
  COLTT_DEVICE(c->device);
  const size_t per = (size_t)c->nf * c->dim;
  const size_t chunk = std::max<size_t>(1, CF_UPSERT_CHUNK_BYTES / (per * 4));
  std::unordered_map<uint64_t, uint32_t> last;   // id -> its entry in the lists below, within the chunk
  std::vector<uint32_t> lists;                   // slots[m] | src[m]: every slot once, so no two workgroups of a launch write one row
  for (size_t o = 0; o < n; o += chunk) {
    const size_t cn = std::min(chunk, n - o);
    // slots in first-appearance order; of an id repeated within the chunk only the last occurrence is written (chunks are applied
    // in order, so across chunks the later one overwrites)
    const uint64_t n0 = c->n;
    last.clear(); lists.clear();
    std::vector<uint32_t> slots, src;
    for (size_t i = 0; i < cn; i++) {
      const uint64_t id = ids[o + i];
      auto seen = last.find(id);
      if (seen != last.end()) { src[seen->second] = (uint32_t)i; continue; }
      uint32_t slot;
      auto it = c->id2slot.find(id);
      if (it != c->id2slot.end()) slot = it->second;
      else { slot = (uint32_t)c->h_ids.size(); c->id2slot[id] = slot; c->h_ids.push_back(id); }
      last[id] = (uint32_t)slots.size();
      slots.push_back(slot); src.push_back((uint32_t)i);
    }
    const size_t m = slots.size();
    const uint64_t n1 = c->h_ids.size();
    auto undo = [&]() { for (uint64_t s = n0; s < n1; s++) c->id2slot.erase(c->h_ids[s]); c->h_ids.resize(n0); };   // a failed chunk stores nothing
    lists = slots; lists.insert(lists.end(), src.begin(), src.end());
    int rc = c->reserve(n1);   // the capacity grows once per chunk
    if (rc == COLTT_OK) rc = c->w_raw.reserve(cn * per * 4);
    if (rc == COLTT_OK) rc = c->w_field.reserve(m * (size_t)c->dim * 4);
    if (rc == COLTT_OK) rc = c->w_slots.reserve(2 * m * 4);
    if (rc != COLTT_OK) { undo(); return rc; }
    auto run = [&]() -> int {
      COLTT_HIP(hipMemcpyAsync(c->w_raw.p, vecs + o * per, cn * per * 4, hipMemcpyHostToDevice, c->stream));
      COLTT_HIP(hipMemcpyAsync(c->w_slots.p, lists.data(), 2 * m * 4, hipMemcpyHostToDevice, c->stream));
      if (n1 > n0) COLTT_HIP(hipMemcpyAsync(c->ids.as<uint64_t>() + n0, c->h_ids.data() + n0, (n1 - n0) * 8, hipMemcpyHostToDevice, c->stream));
      const uint32_t* d_slots = c->w_slots.as<uint32_t>(); const uint32_t* d_src = d_slots + m;
      for (uint32_t f = 0; f < c->nf; f++) {
        cflat_take_field_kernel<<<ceil_div(m * (uint64_t)c->dim, 256), 256, 0, c->stream>>>(c->w_raw.as<float>(), d_src, m, (int)c->nf, (int)f, (int)c->dim, c->w_field.as<float>());
        launch_prep_rows<Q_NONE>(c->stream, c->w_field.as<float>(), m, (int)c->dim, c->metric == COLTT_COSINE, d_slots, 0, c->rows[f].as<uint8_t>(), c->stride);
        row_norms_kernel<Q_NONE><<<ceil_div(m * 2, 256), 256, 0, c->stream>>>(c->rows[f].as<uint8_t>(), c->stride, d_slots, 0, m, (int)c->dim, c->norms[f].as<float>());
      }
      COLTT_HIP(hipGetLastError());
      COLTT_HIP(hipStreamSynchronize(c->stream));
      return COLTT_OK;
    };
    rc = run();
    if (rc != COLTT_OK) { (void)hipStreamSynchronize(c->stream); undo(); return rc; }
    c->n = n1;
  }
  return COLTT_OK;
}

/* RemoveVertex (multi_vector_vertex.go:77-83) */
int coltt_cflat_remove(coltt_handle_t h, const uint64_t* ids, size_t n) {
  auto c = lookup<CFlat>(h);
  if (!c) return fail(COLTT_E_NOT_FOUND, "cflat_remove: unknown handle");
  if (n && !ids) return fail(COLTT_E_INVALID, "cflat_remove: NULL ids");
  WriteLock g(c->rw);
  COLTT_DEVICE(c->device);
  for (size_t i = 0; i < n; i++) {
    auto it = c->id2slot.find(ids[i]);
    if (it == c->id2slot.end()) continue;
    uint32_t s = it->second; uint64_t last = c->n - 1;
    c->id2slot.erase(it);
    if (s != last) {
      for (uint32_t f = 0; f < c->nf; f++) {
        uint8_t* R = c->rows[f].as<uint8_t>();
        COLTT_HIP(hipMemcpyAsync(R + (size_t)s * c->stride, R + (size_t)last * c->stride, c->stride, hipMemcpyDeviceToDevice, c->stream));
        COLTT_HIP(hipMemcpyAsync(c->norms[f].as<float>() + s, c->norms[f].as<float>() + last, 4, hipMemcpyDeviceToDevice, c->stream));
      }
      uint64_t moved = c->h_ids[last]; c->h_ids[s] = moved; c->id2slot[moved] = s;
      COLTT_HIP(hipMemcpyAsync(c->ids.as<uint64_t>() + s, &c->h_ids[s], 8, hipMemcpyHostToDevice, c->stream));
    }
    c->h_ids.pop_back(); c->n--;
    COLTT_HIP(hipStreamSynchronize(c->stream));
  }
  return COLTT_OK;
}

int coltt_cflat_get(coltt_handle_t h, uint64_t id, float* out_fields) {
  auto c = lookup<CFlat>(h);
  if (!c) return fail(COLTT_E_NOT_FOUND, "cflat_get: unknown handle");
  if (!out_fields) return fail(COLTT_E_INVALID, "cflat_get: NULL buffer");
  WriteLock g(c->rw);
  COLTT_DEVICE(c->device);
  auto it = c->id2slot.find(id);
  if (it == c->id2slot.end()) return fail(COLTT_E_NOT_FOUND, "NodeID: %llu is not found", (unsigned long long)id);
  for (uint32_t f = 0; f < c->nf; f++)
    COLTT_HIP(hipMemcpyAsync(out_fields + (size_t)f * c->dim, c->rows[f].as<uint8_t>() + (size_t)it->second * c->stride, (size_t)c->dim * 4, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));
  return COLTT_OK;
}

/* MultiVertexSearch (multi_vector_vertex.go:85-137): queries is [nq][n_fields][dim]; ratios / include are per field.
 * Rows of out_* are DESCENDING by (score, id). */
int coltt_cflat_search(coltt_handle_t h, const float* queries, const uint32_t* ratios, const uint8_t* include, size_t nq, uint32_t k,
                       uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
  auto c = lookup<CFlat>(h);
  if (!c) return fail(COLTT_E_NOT_FOUND, "cflat_search: unknown handle");
  if (nq == 0) return COLTT_OK;
  if (!queries || !ratios || !include || !out_ids || !out_scores || !out_counts) return fail(COLTT_E_INVALID, "cflat_search: NULL buffer");
  if (k == 0 || k > K_MAX) return fail(COLTT_E_UNSUPPORTED, "cflat_search: k=%u outside [1,%u]", k, K_MAX);
  WriteLock g(c->rw);
  COLTT_DEVICE(c->device);
  const size_t per = (size_t)c->nf * c->dim;
  const uint32_t cap = std::max<uint32_t>(65536u, 8u * k);
  COLTT_TRY(c->w_raw.reserve(per * 4)); COLTT_TRY(c->w_q.reserve(per * 4)); COLTT_TRY(c->w_qn.reserve(c->nf * 4 + 256));
  COLTT_TRY(c->w_misc.reserve(4096)); COLTT_TRY(c->w_cand.reserve((size_t)cap * 8));
  COLTT_TRY(c->w_out_ids.reserve((size_t)k * 8)); COLTT_TRY(c->w_out_sc.reserve((size_t)k * 4)); COLTT_TRY(c->w_out_cnt.reserve(4));
  uint32_t* cnt = c->w_misc.as<uint32_t>(); uint32_t* thr = cnt + 256; uint32_t* ovf = cnt + 512;
  uint32_t* d_ratio = cnt + 600; uint8_t* d_inc = reinterpret_cast<uint8_t*>(cnt + 640); float* d_w = reinterpret_cast<float*>(cnt + 700);
  COLTT_HIP(hipMemcpyAsync(d_ratio, ratios, c->nf * 4, hipMemcpyHostToDevice, c->stream));
  COLTT_HIP(hipMemcpyAsync(d_inc, include, c->nf, hipMemcpyHostToDevice, c->stream));
  cflat_weights_kernel<<<1, 64, 0, c->stream>>>(d_ratio, d_inc, c->nf, d_w);
  const CFields F = c->fields();
  const CScanArgs a{c->w_q.as<float>(), c->w_qn.as<float>(), d_w, 1, cnt, thr, c->w_cand.as<unsigned long long>(), cap};
  std::vector<uint64_t> hi(k); std::vector<float> hs(k);
  for (size_t qi = 0; qi < nq; qi++) {
    COLTT_HIP(hipMemcpyAsync(c->w_raw.p, queries + qi * per, per * 4, hipMemcpyHostToDevice, c->stream));
    // included fields are normalised for cosine (multi_vector_vertex.go:96-100); excluded ones are never read
    launch_prep_queries<Q_NONE>(c->stream, c->w_raw.as<float>(), c->nf, (int)c->dim, c->metric == COLTT_COSINE, c->w_q.as<float>());
    query_norms_kernel<<<1, 64, 0, c->stream>>>(c->w_q.as<float>(), c->nf, (int)c->dim, c->w_qn.as<float>());
    COLTT_TRY(search_group(c.get(), F, a, ovf, k, c->w_out_ids.as<uint64_t>(), c->w_out_sc.as<float>(), c->w_out_cnt.as<uint32_t>()));
    uint32_t hc = 0;
    COLTT_HIP(hipMemcpyAsync(&hc, c->w_out_cnt.p, 4, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipMemcpyAsync(hi.data(), c->w_out_ids.p, (size_t)k * 8, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipMemcpyAsync(hs.data(), c->w_out_sc.p, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    COLTT_HIP(hipStreamSynchronize(c->stream));
    out_counts[qi] = hc;
    for (uint32_t j = 0; j < hc; j++) { out_ids[qi * k + j] = hi[hc - 1 - j]; out_scores[qi * k + j] = hs[hc - 1 - j]; }  // ascending -> descending
  }
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

/* nq MultiVertexSearch requests, each with its own ratios and include flags, in passes over the rows shared by a group of requests */
int coltt_cflat_search_batch(coltt_handle_t h, const float* queries, const uint32_t* ratios, const uint8_t* include, size_t nq, uint32_t k,
                             uint64_t* out_ids, float* out_scores, uint32_t* out_counts) {
  auto c = lookup<CFlat>(h);
  if (!c) return fail(COLTT_E_NOT_FOUND, "cflat_search_batch: unknown handle");
  if (nq == 0) return COLTT_OK;
  if (!queries || !ratios || !include || !out_ids || !out_scores || !out_counts) return fail(COLTT_E_INVALID, "cflat_search_batch: NULL buffer");
  if (k == 0 || k > K_MAX) return fail(COLTT_E_UNSUPPORTED, "cflat_search_batch: k=%u outside [1,%u]", k, K_MAX);
  WriteLock g(c->rw);
  COLTT_DEVICE(c->device);
  if (c->n == 0) { std::fill(out_counts, out_counts + nq, 0u); return COLTT_OK; }
  const size_t per = (size_t)c->nf * c->dim, nw = nq * c->nf;
  const uint32_t cap = std::max<uint32_t>(65536u, 8u * k);
  const int qb = cflat_group_width(per * 4);
  // one upload: queries [nq][nf][dim] f32 | ratios [nq][nf] u32 | include [nq][nf] u8
  const size_t off_ratio = nq * per * 4, off_inc = off_ratio + nw * 4, in_bytes = off_inc + nw;
  std::vector<uint8_t> h_in(in_bytes);
  std::memcpy(h_in.data(), queries, off_ratio); std::memcpy(h_in.data() + off_ratio, ratios, nw * 4); std::memcpy(h_in.data() + off_inc, include, nw);
  // one copy back: ids [nq][k] u64 | scores [nq][k] f32 | counts [nq] u32, every row ascending
  const size_t off_sc = nq * k * 8, off_cnt = off_sc + nq * k * 4, out_bytes = off_cnt + nq * 4;
  COLTT_TRY(c->w_raw.reserve(in_bytes)); COLTT_TRY(c->w_q.reserve(nq * per * 4)); COLTT_TRY(c->w_qn.reserve(nw * 4 + 256)); COLTT_TRY(c->w_w.reserve(nw * 4));
  COLTT_TRY(c->w_misc.reserve(4096)); COLTT_TRY(c->w_cand.reserve((size_t)qb * cap * 8)); COLTT_TRY(c->w_out.reserve(out_bytes));
  uint32_t* cnt = c->w_misc.as<uint32_t>(); uint32_t* thr = cnt + 256; uint32_t* ovf = cnt + 512;
  uint8_t* d_in = c->w_raw.as<uint8_t>(); uint8_t* d_out = c->w_out.as<uint8_t>();
  COLTT_HIP(hipMemcpyAsync(d_in, h_in.data(), in_bytes, hipMemcpyHostToDevice, c->stream));
  cflat_weights_kernel<<<ceil_div(nw, 256), 256, 0, c->stream>>>(reinterpret_cast<const uint32_t*>(d_in + off_ratio), d_in + off_inc, nw, c->w_w.as<float>());
  // every field of every request is normalised for cosine; an excluded one (whatever it holds) is never read by the scan
  launch_prep_queries<Q_NONE>(c->stream, reinterpret_cast<const float*>(d_in), nw, (int)c->dim, c->metric == COLTT_COSINE, c->w_q.as<float>(), c->w_qn.as<float>());
  const CFields F = c->fields();
  for (size_t q0 = 0; q0 < nq; q0 += qb) {
    const int gq = (int)std::min<size_t>(qb, nq - q0);
    const CScanArgs a{c->w_q.as<float>() + q0 * per, c->w_qn.as<float>() + q0 * c->nf, c->w_w.as<float>() + q0 * c->nf, gq, cnt, thr, c->w_cand.as<unsigned long long>(), cap};
    COLTT_TRY(search_group(c.get(), F, a, ovf, k, reinterpret_cast<uint64_t*>(d_out) + q0 * k, reinterpret_cast<float*>(d_out + off_sc) + q0 * k,
                           reinterpret_cast<uint32_t*>(d_out + off_cnt) + q0));
  }
  std::vector<uint8_t> h_out(out_bytes);
  COLTT_HIP(hipMemcpyAsync(h_out.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
  COLTT_HIP(hipStreamSynchronize(c->stream));
  const uint64_t* hi = reinterpret_cast<const uint64_t*>(h_out.data()); const float* hs = reinterpret_cast<const float*>(h_out.data() + off_sc);
  const uint32_t* hc = reinterpret_cast<const uint32_t*>(h_out.data() + off_cnt);
  for (size_t q = 0; q < nq; q++) {
    out_counts[q] = hc[q];
    for (uint32_t j = 0; j < hc[q]; j++) { out_ids[q * k + j] = hi[q * k + hc[q] - 1 - j]; out_scores[q * k + j] = hs[q * k + hc[q] - 1 - j]; }  // ascending -> descending
  }
  COLTT_HIP(hipGetLastError());
  return COLTT_OK;
}

}  // extern "C"
