// coltt::FilteredBatcher (include/coltt_batcher.hpp) on a mock backend: many caller threads, each with its own filter handle — every
// caller gets exactly the rows of ITS (query, filter), one backend call carries several filters, batches never mix different k,
// coalescing really happens, and after a batch-level error only the callers whose own filter is bad get the error.  No GPU needed.
#include <atomic>
#include <cstdio>
#include <set>

#include "coltt_batcher.hpp"

static std::atomic<int> fails{0};
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static const coltt_handle_t BAD = 0xbad;   // the mock's "destroyed filter": any call that carries it fails as a whole

int main() {
  const uint32_t dim = 8;
  std::atomic<size_t> max_seen{0}, calls{0}, max_filters{0};
  std::mutex km; std::set<uint32_t> ks_in_call;   // the k of every backend call (one per call)
  // answer for (query tag, filter f): ids f * 1e6 + tag * 1000 + j, scores tag + j / 16; count = min(k, (tag + f) % 7 + 1)
  auto backend = [&](const coltt_handle_t* f, const float* q, size_t nq, uint32_t k, uint64_t* ids, float* sc, uint32_t* cnt) -> int {
    calls++;
    size_t m = max_seen.load(); while (nq > m && !max_seen.compare_exchange_weak(m, nq)) {}
    std::set<coltt_handle_t> fs(f, f + nq);
    size_t mf = max_filters.load(); while (fs.size() > mf && !max_filters.compare_exchange_weak(mf, fs.size())) {}
    { std::lock_guard<std::mutex> g(km); ks_in_call.insert(k); }
    std::this_thread::sleep_for(std::chrono::microseconds(300));   // a "kernel": callers pile up meanwhile
    if (fs.count(BAD)) return COLTT_E_NOT_FOUND;                    // all-or-nothing validation, as coltt_hnsw_search_filtered_batch
    for (size_t i = 0; i < nq; i++) {
      const uint32_t tag = (uint32_t)q[i * dim];
      const uint32_t n = std::min<uint32_t>(k, (uint32_t)((tag + f[i]) % 7 + 1));
      cnt[i] = n;
      for (uint32_t j = 0; j < n; j++) { ids[i * k + j] = f[i] * 1000000ull + (uint64_t)tag * 1000 + j; sc[i * k + j] = (float)tag + (float)j / 16.f; }
    }
    return 0;
  };
  auto expect_rows = [&](const coltt::BatchAnswer& a, uint32_t tag, coltt_handle_t f, uint32_t k) {
    EXPECT(a.rc == 0);
    EXPECT(a.items.size() == std::min<uint32_t>(k, (uint32_t)((tag + f) % 7 + 1)));
    for (size_t j = 0; j < a.items.size(); j++) {
      EXPECT(a.items[j].Id == f * 1000000ull + (uint64_t)tag * 1000 + j);
      EXPECT(a.items[j].Score == (float)tag + (float)j / 16.f);
    }
  };
  {
    coltt::FilteredBatcher b(dim, 16, std::chrono::microseconds(2000), backend);
    const int T = 48, M = 30;
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t] {
      for (int m = 0; m < M; m++) {
        const uint32_t tag = (uint32_t)(t * 1000 + m);
        const uint32_t k = (t % 3 == 0) ? 3u : 5u;                  // two different k in flight at once
        const coltt_handle_t f = 100 + (coltt_handle_t)t;           // each caller its own filter
        float q[dim]; for (uint32_t e = 0; e < dim; e++) q[e] = (float)tag + (float)e;
        expect_rows(b.SearchFiltered(q, k, f), tag, f, k);
      }
    });
    for (auto& x : th) x.join();
    EXPECT(b.queries() == (uint64_t)T * M);
    EXPECT(max_seen.load() <= 16 && b.largest_batch() <= 16);
    EXPECT(b.batches() < (uint64_t)T * M / 2);                      // coalescing happened
    EXPECT(max_filters.load() >= 4);                                // one backend call carried several filters
    EXPECT(b.retried_batches() == 0);
    { std::lock_guard<std::mutex> g(km); EXPECT(ks_in_call == std::set<uint32_t>({3u, 5u})); }
    std::printf("batches %llu for %llu queries, largest %zu, most filters in one call %zu\n", (unsigned long long)b.batches(),
                (unsigned long long)b.queries(), b.largest_batch(), max_filters.load());

  }
  {
    // one caller with a bad filter among good ones: the batch fails as a whole, is re-issued per query, only that caller gets the error.
    // max_batch 12 and a long max_wait: the twelve callers ride in one batch
    coltt::FilteredBatcher b(dim, 12, std::chrono::milliseconds(2000), backend);
    const size_t c0 = calls.load();
    std::vector<std::thread> th2;
    std::atomic<int> bad_rc{1}, good{0};
    for (int t = 0; t < 12; t++) th2.emplace_back([&, t] {
      const uint32_t tag = (uint32_t)(90000 + t);
      const coltt_handle_t f = t == 5 ? BAD : 200 + (coltt_handle_t)t;
      float q[dim]; for (uint32_t e = 0; e < dim; e++) q[e] = (float)tag;
      coltt::BatchAnswer a = b.SearchFiltered(q, 4, f);
      if (t == 5) { bad_rc = a.rc; EXPECT(a.items.empty()); }
      else { expect_rows(a, tag, f, 4); good++; }
    });
    for (auto& x : th2) x.join();
    EXPECT(bad_rc.load() == COLTT_E_NOT_FOUND);
    EXPECT(good.load() == 11);
    EXPECT(b.batches() == 1 && b.retried_batches() == 1);
    EXPECT(calls.load() == c0 + 1 + 12);
    // a lone bad caller gets the backend's error straight away
    float q[dim] = {7, 0, 0, 0, 0, 0, 0, 0};
    coltt::BatchAnswer a = b.SearchFiltered(q, 4, BAD);
    EXPECT(a.rc == COLTT_E_NOT_FOUND && a.items.empty());
    // k == 0 answers empty without calling the backend
    const size_t c1 = calls.load();
    a = b.SearchFiltered(q, 0, 300);
    EXPECT(a.rc == 0 && a.items.empty() && calls.load() == c1);
  }
  std::printf(fails.load() ? "FAILED %d checks\n" : "filtered batcher ok\n", fails.load());
  return fails.load() ? 1 : 0;
}
