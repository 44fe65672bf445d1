// Filtered search through the C++ mirror (include/coltt_gpu.hpp: Hnsw::Filter, Hnsw::SearchFiltered): every answer is allowed, EXACT
// equals a host brute force over the allowed ids (same ids, ascending scores), AUTO and WALK return k, a removed id is never returned.
// Run by tests/test_gpu_hnsw_filter.py.
#include <algorithm>
#include <cstdio>
#include <random>
#include <set>

#include "coltt_gpu.hpp"

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

int main() {
  if (coltt_init(0) != COLTT_OK) { std::printf("no device: %s\n", coltt_last_error()); return 77; }
  const int d = 32, n = 2000, k = 10;
  std::mt19937 g(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<std::vector<float>> X(n, std::vector<float>(d));
  coltt::Hnsw h(d, COLTT_EUCLIDEAN);
  for (int i = 0; i < n; i++) { for (auto& x : X[i]) x = nd(g); h.Insert(i, X[i], h.RandomLevel(std::uniform_real_distribution<float>(1e-6f, 1.f)(g))); }
  std::vector<uint64_t> ids;
  for (int i = 0; i < n; i += 4) ids.push_back(i);
  coltt::Hnsw::Filter f(h, ids);
  EXPECT(f.Allowed() == ids.size());
  h.Remove(0);
  const std::set<uint64_t> ok(ids.begin() + 1, ids.end());
  for (int t = 0; t < 8; t++) {
    std::vector<float> q(d); for (auto& x : q) x = nd(g);
    for (int mode : {COLTT_FILTER_AUTO, COLTT_FILTER_WALK, COLTT_FILTER_EXACT}) {
      coltt_hnsw_filter_stats st{};
      auto r = h.SearchFiltered(q, k, f, 64, mode, &st);
      EXPECT((int)r.size() == k);
      for (auto& it : r) EXPECT(ok.count(it.Id));
      for (size_t i = 1; i < r.size(); i++) EXPECT(r[i - 1].Score <= r[i].Score);
      EXPECT(mode == COLTT_FILTER_AUTO || st.path == mode);
      if (mode == COLTT_FILTER_EXACT) {   // host brute force: the same ids (L2 here: ties are measure-zero on normal data)
        std::vector<std::pair<float, uint64_t>> all;
        for (uint64_t id : ok) { float s = 0; for (int j = 0; j < d; j++) { float e = q[j] - X[id][j]; s += e * e; } all.push_back({s, id}); }
        std::sort(all.begin(), all.end());
        for (int i = 0; i < k; i++) EXPECT(r[i].Id == all[i].second);
      }
    }
  }
  std::printf("%s\n", fails ? "filter FAILED" : "filter ok");
  return fails ? 1 : 0;
}
