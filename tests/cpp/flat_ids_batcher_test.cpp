// coltt::IdsBatcher (include/coltt_batcher.hpp) over FlatIdsBackend = coltt_flat_search_ids_batch on the GPU: 32 caller threads, each a
// filtered RPC with its OWN candidate id list (edge/none_vectorstore.go:182-253) — every caller's answer equals its own direct
// coltt_flat_search_ids call (ids and score bits), callers really ride in shared batches, and a caller with k = 0 or one whose
// backend call is refused does not disturb the others.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <random>

#include "coltt_batcher.hpp"
#include "coltt_gpu.hpp"

static std::atomic<int> fails{0};
#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

int main() {
  if (coltt_init(0) != COLTT_OK) { std::printf("no device: %s\n", coltt_last_error()); return 77; }
  const int d = 64, n = 20000, NQ = 64, T = 32;
  std::mt19937 g(777);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::vector<float> X((size_t)n * d), Q((size_t)NQ * d);
  for (auto& x : X) x = nd(g);
  for (auto& x : Q) x = nd(g);
  for (int i = 100; i < 160; i++) std::memcpy(&X[(size_t)i * d], &X[(size_t)7 * d], d * 4);   // ties: the ids decide
  std::memcpy(&Q[0], &X[(size_t)7 * d], d * 4);
  std::vector<uint64_t> ids(n);
  for (int i = 0; i < n; i++) ids[i] = ((uint64_t)i * 2654435761ull) % (1ull << 33);          // slot order != id order
  coltt::VecSpace f(d, COLTT_COSINE, COLTT_Q_F16);
  f.ChangedVertices(ids, X.data());
  // every caller its own list: 40 .. 6000 stored ids in random order, a few unknown ones, the tied rows in every other list
  std::vector<std::vector<uint64_t>> lists(T);
  for (int t = 0; t < T; t++) {
    std::uniform_int_distribution<int> len(40, 6000), pick(0, n - 1);
    const int m = t == 3 ? 0 : len(g);                       // one caller's filter matches nothing
    for (int i = 0; i < m; i++) lists[t].push_back(ids[pick(g)]);
    for (int i = 0; i < 3 && m; i++) lists[t].push_back(10000000000000ull + (uint64_t)i);
    if (t % 2 == 0 && m) for (int i = 100; i < 160; i++) lists[t].push_back(ids[i]);
  }
  const int sel = COLTT_SELECT_NEAREST;
  auto direct = [&](int qi, uint32_t k, const std::vector<uint64_t>& l) { std::vector<uint64_t> id(k); std::vector<float> sc(k); uint32_t c = 0;
    coltt::check(coltt_flat_search_ids(f.handle(), &Q[(size_t)qi * d], 1, k, sel, l.data(), l.size(), id.data(), sc.data(), &c));
    std::vector<coltt::BatchItem> r(c); for (uint32_t i = 0; i < c; i++) r[i] = {id[i], sc[i]}; return r; };
  auto same = [](const std::vector<coltt::BatchItem>& a, const std::vector<coltt::BatchItem>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) if (a[i].Id != b[i].Id || std::memcmp(&a[i].Score, &b[i].Score, 4) != 0) return false;
    return true; };
  // ---- 1. 32 callers with their own lists and mixed k; one of them asks for k = 0, one for a k the library refuses
  {
    coltt::IdsBatcher b(d, 32, std::chrono::microseconds(2000), coltt::FlatIdsBackend(f.handle(), sel));
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t] {
      for (int it = 0; it < 6; it++) {
        const int qi = t == 0 ? 0 : (t * 6 + it) % NQ;
        if (t == 9) { coltt::BatchAnswer a = b.SearchIds(&Q[(size_t)qi * d], 0, lists[t]); EXPECT(a.rc == COLTT_OK && a.items.empty()); continue; }
        if (t == 17) { coltt::BatchAnswer a = b.SearchIds(&Q[(size_t)qi * d], 5000, lists[t]); EXPECT(a.rc == COLTT_E_UNSUPPORTED && a.items.empty()); continue; }
        const uint32_t k = t % 3 == 0 ? 3u : (t % 3 == 1 ? 10u : 70u);     // 70: the call's k > 64 path
        coltt::BatchAnswer a = b.SearchIds(&Q[(size_t)qi * d], k, lists[t]);
        EXPECT(a.rc == COLTT_OK && same(a.items, direct(qi, k, lists[t])));
        if (t == 3) EXPECT(a.items.empty());
      }
    });
    for (auto& x : th) x.join();
    EXPECT(b.queries() == (uint64_t)T * 6);
    EXPECT(b.largest_batch() > 1 && b.largest_batch() <= 32);
    EXPECT(b.retried_batches() == 0);
    std::printf("ids batcher: %llu batches for %llu queries, largest %zu\n", (unsigned long long)b.batches(), (unsigned long long)b.queries(), b.largest_batch());
    uint64_t one = 0, fb = 0, pairs = 0;
    coltt::check(coltt_flat_ids_batch_stats(f.handle(), &one, &fb, &pairs));
    EXPECT(one > 0 && fb > 0 && pairs > 0);
  }
  // ---- 2. a backend call refused as a whole (one caller's list carries an id the backend rejects): re-issued per query, only that
  //         caller sees the error.  max_batch 12 and a long max_wait: the twelve callers ride in one batch
  {
    const uint64_t POISON = 0xdeadull << 40;
    auto real = coltt::FlatIdsBackend(f.handle(), sel);
    std::atomic<size_t> calls{0};
    coltt::IdsBatcher b(d, 12, std::chrono::milliseconds(2000),
      [&](const float* q, size_t nq, uint32_t k, const uint64_t* c, const uint64_t* off, uint64_t* id, float* sc, uint32_t* cnt) {
        calls++;
        for (uint64_t i = off[0]; i < off[nq]; i++) if (c[i] == POISON) return (int)COLTT_E_INVALID;
        return real(q, nq, k, c, off, id, sc, cnt);
      });
    std::vector<std::thread> th;
    std::atomic<int> bad_rc{1}, good{0};
    for (int t = 0; t < 12; t++) th.emplace_back([&, t] {
      std::vector<uint64_t> l = lists[t + 4];
      if (t == 5) l.push_back(POISON);
      coltt::BatchAnswer a = b.SearchIds(&Q[(size_t)t * d], 10, l);
      if (t == 5) { bad_rc = a.rc; EXPECT(a.items.empty()); }
      else { EXPECT(a.rc == COLTT_OK && same(a.items, direct(t, 10, lists[t + 4]))); good++; }
    });
    for (auto& x : th) x.join();
    EXPECT(bad_rc.load() == COLTT_E_INVALID && good.load() == 11);
    EXPECT(b.batches() == 1 && b.retried_batches() == 1 && calls.load() == 13);
  }
  // ---- 3. the C++ wrapper: VecSpace::FilterableVertexSearchBatch, shared lists through list_of
  {
    std::vector<coltt::Vector> targets;
    for (int i = 0; i < 5; i++) targets.emplace_back(&Q[(size_t)i * d], &Q[(size_t)(i + 1) * d]);
    const std::vector<std::vector<uint64_t>> two = {lists[0], lists[1]};
    const std::vector<uint32_t> lo = {1, 0, 0, 1, 0};
    auto r = f.FilterableVertexSearchBatch(two, targets, 10, sel, lo);
    EXPECT(r.size() == 5);
    for (int i = 0; i < 5; i++) {
      auto w = direct(i, 10, two[lo[i]]);
      EXPECT(r[i].size() == w.size());
      for (size_t j = 0; j < w.size() && j < r[i].size(); j++) EXPECT(r[i][j].Id == w[j].Id && std::memcmp(&r[i][j].Score, &w[j].Score, 4) == 0);
    }
  }
  std::printf(fails.load() ? "FAILED %d checks\n" : "flat ids batcher ok\n", fails.load());
  return fails.load() ? 1 : 0;
}
