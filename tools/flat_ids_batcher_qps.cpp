// The C++ IdsBatcher (include/coltt_batcher.hpp) against direct single-query calls, over a FLAT store the caller already holds:
// `threads` callers, caller t with its own candidate list cand[off[t] .. off[t+1]), each issuing `per_thread` one-query filtered
// searches either straight to coltt_flat_search_ids or through one IdsBatcher around FlatIdsBackend (coltt_flat_search_ids_batch).
// Built as a shared object and called in-process by tools/flat_ids_batch_probe.py (handles are per process), which compiles it with
//   g++ -std=c++17 -O2 -shared -fPIC -pthread -I include tools/flat_ids_batcher_qps.cpp -o <tmp>/qps.so -L coltt_amd -lcoltt_gpu
#include <atomic>
#include <chrono>
#include <memory>
#include <thread>
#include <vector>

#include "coltt_batcher.hpp"

extern "C" int flat_ids_batcher_qps(coltt_handle_t h, uint32_t dim, const uint64_t* cand, const uint64_t* off, const float* queries, int threads,
                                    int per_thread, uint32_t k, int select, int batched, double* out_qps, unsigned long long* out_batches) {
  std::atomic<int> bad{0};
  std::unique_ptr<coltt::IdsBatcher> b;
  if (batched) b.reset(new coltt::IdsBatcher(dim, (size_t)threads, std::chrono::microseconds(200), coltt::FlatIdsBackend(h, select)));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  for (int t = 0; t < threads; t++) th.emplace_back([&, t] {
    std::vector<uint64_t> ids(k); std::vector<float> sc(k);
    const uint64_t* l = cand + off[t]; const size_t nl = (size_t)(off[t + 1] - off[t]);
    for (int m = 0; m < per_thread; m++) {
      const float* q = queries + ((size_t)t * per_thread + m) * dim;
      if (batched) { if (b->SearchIds(q, k, l, nl).rc != 0) bad++; }
      else {
        uint32_t n = 0;
        if (coltt_flat_search_ids(h, q, 1, k, select, l, nl, ids.data(), sc.data(), &n) != 0) bad++;
      }
    }
  });
  for (auto& x : th) x.join();
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out_qps = (double)threads * per_thread / s;
  *out_batches = b ? b->batches() : 0ull;
  return bad.load() ? -1 : 0;
}
