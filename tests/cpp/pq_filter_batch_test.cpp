// Filtered searches over the product-quantised walk with a filter per query from a compiled C++ consumer: coltt::FilteredBatcher
// (include/coltt_batcher.hpp) over coltt::PqFilteredBackend and coltt_hnsw_pq_search_filtered_batch.  16 caller threads, each with its own
// Filter: every answer equals a direct PqSearchFiltered, and the batcher coalesces.  Also Hnsw::PqSearchFilteredBatch against per-query
// PqSearchFiltered.  Run by tests/test_gpu_hnsw_pq_filter_batch.py.
#include <atomic>
#include <cstdio>
#include <memory>
#include <random>

#include "coltt_batcher.hpp"
#include "coltt_gpu.hpp"

static std::atomic<int> fails{0};
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static bool same(const coltt::SearchResult& a, const std::vector<coltt::BatchItem>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (a[i].Id != b[i].Id || std::memcmp(&a[i].Score, &b[i].Score, 4) != 0) return false;
  return true;
}

int main() {
  if (coltt_init(0) != COLTT_OK) { std::printf("no device: %s\n", coltt_last_error()); return 77; }
  const int d = 32, n = 3000, k = 10, T = 16;
  const unsigned rerank = 12;
  std::mt19937 g(13);
  std::normal_distribution<float> nd(0.f, 1.f);
  coltt::Hnsw h(d, COLTT_EUCLIDEAN);
  std::vector<float> sample;
  for (int i = 0; i < n; i++) {
    std::vector<float> x(d); for (auto& v : x) v = nd(g);
    if (i < 1000) sample.insert(sample.end(), x.begin(), x.end());
    h.Insert(i, x, h.RandomLevel(std::uniform_real_distribution<float>(1e-6f, 1.f)(g)));
  }
  coltt::ProductQuantizerParameters pp; pp.NumCentroids = 32; pp.NumSubVectors = 16;
  coltt::ProductQuantizer pq(d, COLTT_PQ_EUCLIDEAN, pp);
  pq.Fit(sample, 4);
  if (coltt_hnsw_pq_attach(h.handle(), pq.handle()) != COLTT_OK) { std::printf("attach: %s\n", coltt_last_error()); return 1; }
  std::vector<std::unique_ptr<coltt::Hnsw::Filter>> flt;
  for (int t = 0; t < T; t++) {   // selectivities from 50 % to 0.5 %: AUTO walks some and scans others
    std::vector<uint64_t> ids;
    const int step = 2 + (t % 8) * 28;
    for (int i = t % step; i < n; i += step) ids.push_back(i);
    flt.emplace_back(new coltt::Hnsw::Filter(h, ids));
  }
  std::vector<std::vector<float>> Q(T, std::vector<float>(d));
  for (auto& q : Q) for (auto& v : q) v = nd(g);
  // the mirror's batch call, row by row against the single call
  {
    std::vector<const coltt::Hnsw::Filter*> fp;
    for (auto& f : flt) fp.push_back(f.get());
    std::vector<int> paths;
    auto rows = h.PqSearchFilteredBatch(Q, k, fp, 0, rerank, COLTT_FILTER_AUTO, &paths);
    EXPECT(rows.size() == (size_t)T && paths.size() == (size_t)T);
    int walks = 0, exacts = 0;
    for (int t = 0; t < T; t++) {
      coltt_hnsw_filter_stats st{};
      auto r = h.PqSearchFiltered(Q[t], k, *flt[t], 0, rerank, COLTT_FILTER_AUTO, &st);
      EXPECT(paths[t] == st.path);
      walks += paths[t] == COLTT_FILTER_WALK; exacts += paths[t] == COLTT_FILTER_EXACT;
      std::vector<coltt::BatchItem> b;
      for (auto& it : rows[t]) b.push_back({it.Id, it.Score});
      EXPECT(same(r, b));
    }
    EXPECT(walks > 0 && exacts > 0);
  }
  // the batcher over the ready-made backend, 16 callers with their own filters
  coltt::FilteredBatcher b(d, 16, std::chrono::microseconds(3000), coltt::PqFilteredBackend(h.handle(), rerank));
  const int M = 4;
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++) th.emplace_back([&, t] {
    for (int m = 0; m < M; m++) {
      coltt::BatchAnswer a = b.SearchFiltered(Q[t].data(), k, flt[t]->handle());
      EXPECT(a.rc == 0);
      EXPECT(same(h.PqSearchFiltered(Q[t], k, *flt[t], 0, rerank), a.items));
    }
  });
  for (auto& x : th) x.join();
  EXPECT(b.queries() == (uint64_t)T * M);
  EXPECT(b.batches() < b.queries());
  std::printf("batches %llu for %llu callers' queries, largest %zu\n", (unsigned long long)b.batches(), (unsigned long long)b.queries(), b.largest_batch());
  std::printf("%s\n", fails.load() ? "pq filter batch FAILED" : "pq filter batch ok");
  return fails.load() ? 1 : 0;
}
