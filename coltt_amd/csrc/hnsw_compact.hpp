// hnsw_compact.hpp — coltt_hnsw_compact (include/coltt_gpu.h, "HNSW compaction"): the plan and the kernels.
//
// The plan is a monotone renumbering: new(s) = live slots below s.  new(s) <= s, so when the destination rows [j0, j1) are written the only rows
// they can overwrite are sources of destinations below j1 — a chunk [j0, j1) is first GATHERED whole into a bounded staging block (sources
// old_of_new[j0 .. j1), all >= j0) and then copied to its destinations (a contiguous run), the two launches in stream order; chunks ascend.
// Nothing here reads a row after a destination at or past it has been written, so the move needs no second copy of the collection.
//   compact_gather_kernel   rows of any byte length listed by source index -> the staging block, one 16- / 8- / 4-byte access per lane, coalesced per row
//   compact_copy_kernel     the staging block -> its destinations (a contiguous run), the same access width
//   compact_adj_kernel      adjacency rows: one wave per row drops the tombstoned entries, renames the survivors by the per-word rank table, packs them by
//                           ballot + prefix popcount (monotone: still ascending), pads; the per-edge companions move in step.  Writes into the staging
//                           block, or in place for the rows below the first one that moves (out position <= in position within a row)
// The old tombstone bitmap and the rank table are read by every launch and written by none.
#pragma once
#include <algorithm>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace coltt {
namespace compact {

constexpr uint32_t NONE = 0xffffffffu;

// The plan, host only.  del_bits: bit s of word s / 32 = slot s is tombstoned (NULL: none is); levels (may be NULL when neither upper output is asked for).
// out_new_of_old[s] = live slots below s, NONE for a tombstoned s; out_new_upper_off[new(s)] = upper rows owned by the live slots below s (NONE for a vertex
// of level 0); *out_live, *out_upper_rows = the totals.  Every output may be NULL.
inline void map_host(const uint32_t* del_bits, uint64_t n, const int32_t* levels, uint32_t* out_new_of_old, uint32_t* out_new_upper_off,
                     uint64_t* out_live, uint64_t* out_upper_rows) {
  uint64_t live = 0, up = 0;
  for (uint64_t s = 0; s < n; s++) {
    const bool dead = del_bits && ((del_bits[s >> 5] >> (s & 31)) & 1u);
    if (dead) { if (out_new_of_old) out_new_of_old[s] = NONE; continue; }
    if (out_new_of_old) out_new_of_old[s] = (uint32_t)live;
    const int32_t lv = levels ? levels[s] : 0;
    if (out_new_upper_off) out_new_upper_off[live] = lv > 0 ? (uint32_t)up : NONE;
    if (lv > 0) up += (uint64_t)lv;
    live++;
  }
  if (out_live) *out_live = live;
  if (out_upper_rows) *out_upper_rows = up;
}

template <int VB> struct Piece;
template <> struct Piece<16> { typedef uint4 T; };
template <> struct Piece<8> { typedef uint2 T; };
template <> struct Piece<4> { typedef uint32_t T; };

// stage[i] = src row src_list[i], i < m: thread t moves piece t % ppr of row t / ppr (ppr = row_bytes / VB pieces per row)
template <int VB>
__global__ __launch_bounds__(256) void compact_gather_kernel(const uint8_t* __restrict__ src, size_t row_bytes, uint32_t ppr,
                                                             const uint32_t* __restrict__ src_list, uint64_t pieces, uint8_t* __restrict__ stage) {
  typedef typename Piece<VB>::T T;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pieces) return;
  const uint64_t i = t / ppr; const uint32_t pc = (uint32_t)(t - i * ppr);
  reinterpret_cast<T*>(stage)[t] = *reinterpret_cast<const T*>(src + (size_t)src_list[i] * row_bytes + (size_t)pc * VB);
}

template <int VB>
__global__ __launch_bounds__(256) void compact_copy_kernel(const uint8_t* __restrict__ stage, uint8_t* __restrict__ dst, uint64_t pieces) {
  typedef typename Piece<VB>::T T;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= pieces) return;
  reinterpret_cast<T*>(dst)[t] = reinterpret_cast<const T*>(stage)[t];
}

// a dense-id index that loses slots: ids[j] = base + old_of_new[j]
__global__ void compact_dense_ids_kernel(uint64_t* __restrict__ ids, const uint32_t* __restrict__ old_of_new, uint64_t live, uint64_t base) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < live) ids[j] = base + old_of_new[j];
}

struct AdjJob {
  const uint32_t* src_ids; const float* src_d; const float* src_n; const float2* src_m;   // the rows as they are (src_n / src_m: level 0 only, may be NULL)
  uint32_t* dst_ids; float* dst_d; float* dst_n; float2* dst_m;                           // destination row r is row dst_row0 + r of these
  const uint32_t* src_list;      // [m] the source row of destination row r
  uint64_t dst_row0;
  uint32_t m, W;
  const uint32_t* del_bits;      // the OLD tombstones, [ceil(n_slots / 32)]
  const uint32_t* rank;          // [ceil(n_slots / 32)] live slots below slot 32 w
  uint32_t n_slots;
  unsigned long long* dropped;   // += entries that named a tombstoned slot
};

// One wave per row, 64 entries per step.  In place (dst == src, dst_row0 + r == src_list[r]) a step's stores land at positions <= the positions it loaded
// and only after its loads have returned (the positions come from the ballot over the loaded entries); the padding is written after the last step.
// A wave strides over the rows of the launch and adds its dropped count once at its end: one atomic per row on the one counter serialised the launch
// (150 000 of them cost about 0.5 ms of a 2.2 ms call at 1 M slots, 10 % dead).
__global__ __launch_bounds__(256) void compact_adj_kernel(AdjJob a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * (blockDim.x >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  uint32_t drop = 0;
  for (uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); r < a.m; r += waves) {
    const size_t so = (size_t)a.src_list[r] * a.W, dof = (size_t)(a.dst_row0 + r) * a.W;
    uint32_t out = 0;
    for (uint32_t b = 0; b < a.W; b += 64) {
      const uint32_t p = b + lane;
      const bool in = p < a.W;
      const uint32_t e = in ? a.src_ids[so + p] : NONE;
      const float d = in ? a.src_d[so + p] : 0.f;
      const float nn = (in && a.src_n) ? a.src_n[so + p] : 0.f;
      const float2 mm = (in && a.src_m) ? a.src_m[so + p] : float2{0.f, 0.f};
      bool keep = false; uint32_t ne = NONE;
      if (e < a.n_slots) {   // (NONE is not below n_slots)
        const uint32_t w = a.del_bits[e >> 5], bit = 1u << (e & 31);
        keep = (w & bit) == 0u;
        ne = a.rank[e >> 5] + (uint32_t)__popc(~w & (bit - 1u));
      }
      const unsigned long long km = __ballot(keep);
      drop += (uint32_t)__popcll(__ballot(e != NONE && !keep));
      if (keep) {
        const size_t q = dof + out + (uint32_t)__popcll(km & below);
        a.dst_ids[q] = ne; a.dst_d[q] = d;
        if (a.dst_n) a.dst_n[q] = nn;
        if (a.dst_m) a.dst_m[q] = mm;
      }
      out += (uint32_t)__popcll(km);
    }
    for (uint32_t p = out + lane; p < a.W; p += 64) {
      a.dst_ids[dof + p] = NONE; a.dst_d[dof + p] = 0.f;
      if (a.dst_n) a.dst_n[dof + p] = 0.f;
      if (a.dst_m) a.dst_m[dof + p] = float2{0.f, 0.f};
    }
  }
  if (lane == 0 && drop) atomicAdd(a.dropped, (unsigned long long)drop);
}
// the grid of a launch over m rows: four rows per workgroup, at most 2048 workgroups (eight per CU) striding over the rest
inline unsigned adj_grid(uint64_t m) { return (unsigned)std::min<uint64_t>((m + 3) / 4, 2048); }

inline int width_of(size_t row_bytes) { return row_bytes % 16 == 0 ? 16 : row_bytes % 8 == 0 ? 8 : 4; }

// rows src_list[0 .. m) of `src` -> stage (packed)
inline void launch_gather(hipStream_t s, const uint8_t* src, size_t row_bytes, const uint32_t* src_list, uint64_t m, uint8_t* stage) {
  const int vb = width_of(row_bytes);
  const uint32_t ppr = (uint32_t)(row_bytes / vb);
  const uint64_t pieces = m * ppr;
  const unsigned grid = (unsigned)((pieces + 255) / 256);
  if (vb == 16) compact_gather_kernel<16><<<grid, 256, 0, s>>>(src, row_bytes, ppr, src_list, pieces, stage);
  else if (vb == 8) compact_gather_kernel<8><<<grid, 256, 0, s>>>(src, row_bytes, ppr, src_list, pieces, stage);
  else compact_gather_kernel<4><<<grid, 256, 0, s>>>(src, row_bytes, ppr, src_list, pieces, stage);
}
// stage (packed, `bytes` long, a multiple of the access width `vb`) -> dst
inline void launch_copy(hipStream_t s, const uint8_t* stage, uint8_t* dst, uint64_t bytes, int vb) {
  const uint64_t pieces = bytes / vb;
  const unsigned grid = (unsigned)((pieces + 255) / 256);
  if (vb == 16) compact_copy_kernel<16><<<grid, 256, 0, s>>>(stage, dst, pieces);
  else if (vb == 8) compact_copy_kernel<8><<<grid, 256, 0, s>>>(stage, dst, pieces);
  else compact_copy_kernel<4><<<grid, 256, 0, s>>>(stage, dst, pieces);
}

}  // namespace compact
}  // namespace coltt
