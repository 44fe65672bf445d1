// Filtered searches with a filter per query from a compiled C++ consumer: coltt::FilteredBatcher (include/coltt_batcher.hpp) over
// coltt::Hnsw (include/coltt_gpu.hpp) and coltt_hnsw_search_filtered_batch.  64 caller threads, each with its own Filter: every answer
// equals a direct SearchFiltered, the batcher coalesces, a caller holding a stale filter gets its error while the others are served.
// Also Hnsw::SearchFilteredBatch against per-query SearchFiltered.  Run by tests/test_gpu_hnsw_filter_batch.py.
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
  const int d = 32, n = 3000, k = 10, T = 64;
  std::mt19937 g(11);
  std::normal_distribution<float> nd(0.f, 1.f);
  coltt::Hnsw h(d, COLTT_EUCLIDEAN);
  for (int i = 0; i < n; i++) {
    std::vector<float> x(d); for (auto& v : x) v = nd(g);
    h.Insert(i, x, h.RandomLevel(std::uniform_real_distribution<float>(1e-6f, 1.f)(g)));
  }
  // a filter built before a Load is stale; the callers' filters are built after it
  coltt::Hnsw::Filter stale(h, {1, 2, 3});
  h.Load(h.Commit());
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
    auto rows = h.SearchFilteredBatch(Q, k, fp, 0, COLTT_FILTER_AUTO, &paths);
    EXPECT(rows.size() == (size_t)T && paths.size() == (size_t)T);
    int walks = 0, exacts = 0;
    for (int t = 0; t < T; t++) {
      coltt_hnsw_filter_stats st{};
      auto r = h.SearchFiltered(Q[t], k, *flt[t], 0, COLTT_FILTER_AUTO, &st);
      EXPECT(paths[t] == st.path);
      walks += paths[t] == COLTT_FILTER_WALK; exacts += paths[t] == COLTT_FILTER_EXACT;
      std::vector<coltt::BatchItem> b;
      for (auto& it : rows[t]) b.push_back({it.Id, it.Score});
      EXPECT(same(r, b));
    }
    EXPECT(walks > 0 && exacts > 0);
  }
  // the batcher, 64 callers with their own filters
  const coltt_handle_t hh = h.handle();
  coltt::FilteredBatcher b(d, 64, std::chrono::microseconds(3000),
                           [hh](const coltt_handle_t* f, const float* q, size_t nq, uint32_t kk, uint64_t* ids, float* sc, uint32_t* cnt) {
                             return coltt_hnsw_search_filtered_batch(hh, f, q, nq, kk, 0, COLTT_FILTER_AUTO, ids, sc, cnt, nullptr, nullptr);
                           });
  const int M = 4;
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++) th.emplace_back([&, t] {
    for (int m = 0; m < M; m++) {
      coltt::BatchAnswer a = b.SearchFiltered(Q[t].data(), k, flt[t]->handle());
      EXPECT(a.rc == 0);
      EXPECT(same(h.SearchFiltered(Q[t], k, *flt[t]), a.items));
    }
  });
  for (auto& x : th) x.join();
  EXPECT(b.queries() == (uint64_t)T * M);
  EXPECT(b.batches() < (uint64_t)T * M);
  std::printf("batches %llu for %llu callers' queries, largest %zu\n", (unsigned long long)b.batches(), (unsigned long long)b.queries(), b.largest_batch());
  // one caller holds the stale filter: it gets COLTT_E_INVALID, the others are served
  std::vector<std::thread> th2;
  std::atomic<int> ok{0}, bad_rc{0};
  for (int t = 0; t < 16; t++) th2.emplace_back([&, t] {
    const coltt_handle_t f = t == 7 ? stale.handle() : flt[t]->handle();
    coltt::BatchAnswer a = b.SearchFiltered(Q[t].data(), k, f);
    if (t == 7) bad_rc = a.rc;
    else if (a.rc == 0 && same(h.SearchFiltered(Q[t], k, *flt[t]), a.items)) ok++;
  });
  for (auto& x : th2) x.join();
  EXPECT(bad_rc.load() == COLTT_E_INVALID);
  EXPECT(ok.load() == 15);
  std::printf("%s\n", fails.load() ? "filter batch FAILED" : "filter batch ok");
  return fails.load() ? 1 : 0;
}
