// tools/isa/walks.hip — scratch translation unit for ISA inspection: the walk kernels whose expansion chain the round's instruction work is about.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fno-gpu-flush-denormals-to-zero --cuda-device-only -S \
//         -I coltt_amd/csrc -I include tools/isa/walks.hip -o /tmp/walks.s && python tools/isa_loops.py /tmp/walks.s
// Not part of the library (coltt_amd/build.py compiles coltt_amd/csrc/*.hip only).
#include "hnsw_kernels.hpp"
namespace coltt {
namespace kern {
#ifndef WALKS_SET
#define WALKS_SET 15
#endif
#if WALKS_SET & 1   // the headline: 10 M x 768 f32, ef 128 (LDS-visited, eight-lane core)
template __global__ void hnsw_search2_kernel<0, 0, 1, 4, 1, false, true, false>(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
    uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*);
#endif
#if WALKS_SET & 2   // the operating point: 10 M x 768 f16, ef 1024 (HBM-visited, delta set, Bloom filter, eight-lane core)
template __global__ void hnsw_search2_kernel<0, 1, 2, 7, 0, false, true, false>(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
    uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*);
#endif
#if WALKS_SET & 4   // the walk over product-quantiser codes (64 x 32 quantiser: LS = 5, NP = 4; 32 x 256: LS = 8, NP = 2), gathered code rows | neighbourhood blocks
#define PQK(LS, NP, NBR) template __global__ void hnsw_pq_search_kernel<2, 0, LS, NP, NBR>(GraphView, int32_t, int32_t, const unsigned short*, const uint8_t*, const uint8_t*, uint32_t, uint32_t, uint32_t, uint32_t, \
    uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*, FilterView, uint32_t);
PQK(5, 0, false)
PQK(5, 4, false)
PQK(5, 4, true)
PQK(8, 2, true)
#undef PQK
#endif
#if WALKS_SET & 8   // single-query latency: 768 x f32 (24 lines), 768 x f16 (12 lines), natural-order rows
#define LATK(Q, TP, SEQ) template __global__ void hnsw_search_lat_kernel<0, Q, TP, SEQ>(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, \
    uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*, unsigned long long*, int);
LATK(0, 24, false)
LATK(1, 12, false)
LATK(0, -1, false)
LATK(0, 0, false)
LATK(0, -1, true)
#undef LATK
#endif
#if WALKS_SET & 16  // the non-temporal twins of the headline and the operating-point walks (collections far larger than the caches)
template __global__ void hnsw_search2_kernel<0, 0, 1, 4, 1, false, true, false, true>(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
    uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*);
template __global__ void hnsw_search2_kernel<0, 1, 2, 7, 0, false, true, false, true>(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
    uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*);
#endif
#if WALKS_SET & 96   // every shipped instance of the walk over product-quantiser codes — the (LS, NP) dispatch of launch_pq_walk x {LDS hash, byte map + gather,
                     // byte map + neighbourhood blocks} — 32: unfiltered, 64: the FILTER instances (coltt_hnsw_pq_search_filtered)
#define PQF(OPT, VIS, LS, NP, NBR, F) template __global__ void hnsw_pq_search_kernel<OPT, VIS, LS, NP, NBR, F>(GraphView, int32_t, int32_t, const unsigned short*, const uint8_t*, const uint8_t*, uint32_t, uint32_t, \
    uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, uint32_t*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*, FilterView, uint32_t);
#define PQF3(LS, NP, F) PQF(0, 1, LS, NP, false, F) PQF(2, 0, LS, NP, false, F) PQF(2, 0, LS, NP, true, F)
#define PQF_ALL(F) PQF3(5, 4, F) PQF3(4, 4, F) PQF3(8, 2, F) PQF3(8, 6, F) PQF3(4, 0, F) PQF3(5, 0, F) PQF3(8, 0, F) PQF3(0, 0, F)
#if WALKS_SET & 32
PQF_ALL(false)
#endif
#if WALKS_SET & 64
PQF_ALL(true)
#endif
#undef PQF_ALL
#undef PQF3
#undef PQF
#endif
#if WALKS_SET & 128   // the row-filter twins of the headline walk (non-temporal loads): 8-bit shadow with the f32 query, binary16 shadow, 8-bit shadow with
                      // the quantised query (integer phase A, row_filter8i.hpp), that kind's ef > 128 twin (walk variant 7), and the headline over the
                      // 16-bit visited set (vis16.hpp; VIS_LDS16 = 2: two waves per SIMD)
#define RFK(PROF, OPT, VIS, BITS) template __global__ void hnsw_search2_rowfilter_kernel<PROF, OPT, VIS, true, BITS>(GraphView, int32_t, int32_t, const float*, const float*, uint32_t, uint32_t, uint32_t, \
    uint32_t, uint32_t, uint32_t*, uint64_t*, float*, uint32_t*, unsigned long long*, uint8_t*, size_t, uint32_t*, uint32_t);
RFK(1, 4, 1, 8)
RFK(1, 4, 1, 16)
RFK(1, 4, 1, 80)
RFK(2, 7, 0, 80)
RFK(1, 4, 2, 80)
#undef RFK
#endif
}  // namespace kern
}  // namespace coltt
