// The C++ FilteredBatcher (include/coltt_batcher.hpp) against direct single-query calls, over an index the caller already holds:
// `threads` callers, caller t with filter filters[t], each issuing `per_thread` one-query filtered searches (AUTO) either straight to
// coltt_hnsw_search_filtered or through one FilteredBatcher around coltt_hnsw_search_filtered_batch.  Built as a shared object and
// called in-process by tools/hnsw_filter_batch_probe.py (handles are per process), which compiles it with
//   g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tools/filter_batcher_qps.cpp -o <tmp>/qps.so -L coltt_amd -lcoltt_gpu
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

#include "coltt_batcher.hpp"

extern "C" int filter_batcher_qps(coltt_handle_t h, uint32_t dim, const coltt_handle_t* filters, const float* queries, int threads, int per_thread,
                                  uint32_t k, int batched, double* out_qps, unsigned long long* out_batches) {
  std::atomic<int> bad{0};
  std::unique_ptr<coltt::FilteredBatcher> b;
  if (batched)
    b.reset(new coltt::FilteredBatcher(dim, (size_t)threads, std::chrono::microseconds(200),
                                       [h](const coltt_handle_t* f, const float* q, size_t nq, uint32_t kk, uint64_t* ids, float* sc, uint32_t* cnt) {
                                         return coltt_hnsw_search_filtered_batch(h, f, q, nq, kk, 0, COLTT_FILTER_AUTO, ids, sc, cnt, nullptr, nullptr);
                                       }));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++) th.emplace_back([&, t] {
    std::vector<uint64_t> ids(k); std::vector<float> sc(k);
    for (int m = 0; m < per_thread; m++) {
      const float* q = queries + ((size_t)t * per_thread + m) * dim;
      if (batched) { if (b->SearchFiltered(q, k, filters[t]).rc != 0) bad++; }
      else {
        uint32_t n = 0;
        if (coltt_hnsw_search_filtered(h, filters[t], q, 1, k, 0, COLTT_FILTER_AUTO, ids.data(), sc.data(), &n, nullptr) != 0) bad++;
      }
    }
  });
  for (auto& x : th) x.join();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out_qps = (double)threads * per_thread / s;
  *out_batches = b ? b->batches() : 0ull;
  return bad.load() ? -1 : 0;
}
