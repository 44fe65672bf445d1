// coltt_batcher.hpp — the RPC micro-batcher of SURVEY.md §8f.4 as compiled code (header-only C++17).
//
// The reference serves ONE query per RPC (core/core.go:633-695, edge/edge.go:610-690), each on its own goroutine; a GPU wants
// batches.  Callers on any number of threads call Search(query, k) and block; a collector thread flushes when max_batch
// queries are waiting or max_wait elapsed since the first of them, issues ONE batched search and hands every caller its own
// rows.  Queries are grouped by k: HNSW uses ef = max(cfg.ef, k), so answers for different k are not prefixes of one another
// in general.  Same semantics as go/colttgpu/batcher.go (the Go source the maintainer compiles); this one is exercised by
// tests/cpp/batcher_test.cpp on a mock backend (CPU) and over coltt::Hnsw on the GPU.
//
// Backend = any callable  int(const float* queries, size_t nq, uint32_t k, uint64_t* ids, float* scores, uint32_t* counts)
// returning COLTT_OK or an error code, e.g. a lambda around coltt_hnsw_search / coltt_flat_search.
//
// FilteredBatcher: the same collector for filtered searches, each caller with its own filter handle (coltt_hnsw_filter_create).  One
// batch mixes any number of filters; its backend takes one handle per query, e.g. a lambda around coltt_hnsw_search_filtered_batch, or
// PqFilteredBackend(index, rerank) for the walk over product-quantiser codes (coltt_hnsw_pq_search_filtered_batch).
//
// IdsBatcher: the collector for FLAT filtered searches, each caller with its own candidate id list (the reference's
// FilterableVertexSearch RPC); its backend takes one list per query: FlatIdsBackend(store, select) = coltt_flat_search_ids_batch.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "coltt_gpu.h"

namespace coltt {

struct BatchItem { uint64_t Id; float Score; };
struct BatchAnswer { int rc = 0; std::vector<BatchItem> items; };

class Batcher {
 public:
  using Backend = std::function<int(const float*, size_t, uint32_t, uint64_t*, float*, uint32_t*)>;

  Batcher(uint32_t dim, size_t max_batch, std::chrono::microseconds max_wait, Backend backend)
      : dim_(dim), max_batch_(max_batch ? max_batch : 1), max_wait_(max_wait), backend_(std::move(backend)),
        worker_([this] { loop(); }) {}
  ~Batcher() {
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
    cv_.notify_all();
    worker_.join();
  }
  Batcher(const Batcher&) = delete;
  Batcher& operator=(const Batcher&) = delete;

  // blocks until the batch this query rode in has been answered; the query is copied before returning to the collector
  BatchAnswer Search(const float* query, uint32_t k) {
    auto p = std::make_shared<Pending>();
    p->q.assign(query, query + dim_);
    p->k = k;
    std::future<BatchAnswer> f = p->done.get_future();
    {
      std::lock_guard<std::mutex> g(mu_);
      queue_.push_back(p);
    }
    cv_.notify_all();
    return f.get();
  }

  // statistics (for tests / tuning)
  uint64_t batches() const { std::lock_guard<std::mutex> g(mu_); return n_batches_; }
  uint64_t queries() const { std::lock_guard<std::mutex> g(mu_); return n_queries_; }
  size_t largest_batch() const { std::lock_guard<std::mutex> g(mu_); return largest_; }

 private:
  struct Pending { std::vector<float> q; uint32_t k = 0; std::promise<BatchAnswer> done; };

  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
      if (queue_.empty()) { if (stop_) return; continue; }
      // the first waiting query opens a batch for its k; wait for company until the batch is full or max_wait elapsed
      const uint32_t k = queue_.front()->k;
      const auto deadline = std::chrono::steady_clock::now() + max_wait_;
      while (!stop_ && count_k(k) < max_batch_) {
        if (cv_.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
      std::vector<std::shared_ptr<Pending>> batch;
      for (auto it = queue_.begin(); it != queue_.end() && batch.size() < max_batch_;) {
        if ((*it)->k == k) { batch.push_back(*it); it = queue_.erase(it); } else ++it;
      }
      n_batches_++; n_queries_ += batch.size(); if (batch.size() > largest_) largest_ = batch.size();
      lk.unlock();
      flush(batch, k);
      lk.lock();
    }
  }
  size_t count_k(uint32_t k) const { size_t c = 0; for (auto& p : queue_) c += p->k == k; return c; }

  void flush(std::vector<std::shared_ptr<Pending>>& batch, uint32_t k) {
    const size_t nq = batch.size();
    std::vector<float> flat(nq * dim_);
    for (size_t i = 0; i < nq; i++) std::memcpy(flat.data() + i * dim_, batch[i]->q.data(), dim_ * sizeof(float));
    std::vector<uint64_t> ids(nq * (size_t)(k ? k : 1));
    std::vector<float> sc(nq * (size_t)(k ? k : 1));
    std::vector<uint32_t> cnt(nq, 0);
    const int rc = k ? backend_(flat.data(), nq, k, ids.data(), sc.data(), cnt.data()) : 0;
    for (size_t i = 0; i < nq; i++) {
      BatchAnswer a; a.rc = rc;
      if (rc == 0) {
        const uint32_t n = cnt[i] < k ? cnt[i] : k;
        a.items.resize(n);
        for (uint32_t j = 0; j < n; j++) a.items[j] = {ids[i * k + j], sc[i * k + j]};
      }
      batch[i]->done.set_value(std::move(a));
    }
  }

  const uint32_t dim_; const size_t max_batch_; const std::chrono::microseconds max_wait_; Backend backend_;
  mutable std::mutex mu_; std::condition_variable cv_; std::deque<std::shared_ptr<Pending>> queue_;
  bool stop_ = false; uint64_t n_batches_ = 0, n_queries_ = 0; size_t largest_ = 0;
  std::thread worker_;  // last member: started after everything else is initialised
};

// The micro-batcher for filtered searches (coltt_hnsw_search_filtered_batch): callers bring their own filter, batches are grouped by k
// only.  Backend = int(const coltt_handle_t* filters, const float* queries, size_t nq, uint32_t k, uint64_t* ids, float* scores,
// uint32_t* counts).  The batch call validates every handle before it runs anything, so one caller's bad filter (destroyed, stale, of
// another index) fails the whole call: the batch is then re-issued one query at a time, and only the callers whose own call fails get
// its error.
class FilteredBatcher {
 public:
  using Backend = std::function<int(const coltt_handle_t*, const float*, size_t, uint32_t, uint64_t*, float*, uint32_t*)>;

  FilteredBatcher(uint32_t dim, size_t max_batch, std::chrono::microseconds max_wait, Backend backend)
      : dim_(dim), max_batch_(max_batch ? max_batch : 1), max_wait_(max_wait), backend_(std::move(backend)),
        worker_([this] { loop(); }) {}
  ~FilteredBatcher() {
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
    cv_.notify_all();
    worker_.join();
  }
  FilteredBatcher(const FilteredBatcher&) = delete;
  FilteredBatcher& operator=(const FilteredBatcher&) = delete;

  // blocks until answered; the query is copied before returning to the collector
  BatchAnswer SearchFiltered(const float* query, uint32_t k, coltt_handle_t filter) {
    auto p = std::make_shared<Pending>();
    p->q.assign(query, query + dim_);
    p->k = k; p->filter = filter;
    std::future<BatchAnswer> f = p->done.get_future();
    {
      std::lock_guard<std::mutex> g(mu_);
      queue_.push_back(p);
    }
    cv_.notify_all();
    return f.get();
  }

  // statistics (for tests / tuning); retried_batches: batches the backend refused as a whole and that were re-issued per query
  uint64_t batches() const { std::lock_guard<std::mutex> g(mu_); return n_batches_; }
  uint64_t queries() const { std::lock_guard<std::mutex> g(mu_); return n_queries_; }
  size_t largest_batch() const { std::lock_guard<std::mutex> g(mu_); return largest_; }
  uint64_t retried_batches() const { std::lock_guard<std::mutex> g(mu_); return n_retried_; }

 private:
  struct Pending { std::vector<float> q; uint32_t k = 0; coltt_handle_t filter = 0; std::promise<BatchAnswer> done; };

  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
      if (queue_.empty()) { if (stop_) return; continue; }
      const uint32_t k = queue_.front()->k;
      const auto deadline = std::chrono::steady_clock::now() + max_wait_;
      while (!stop_ && count_k(k) < max_batch_) {
        if (cv_.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
      std::vector<std::shared_ptr<Pending>> batch;
      for (auto it = queue_.begin(); it != queue_.end() && batch.size() < max_batch_;) {
        if ((*it)->k == k) { batch.push_back(*it); it = queue_.erase(it); } else ++it;
      }
      n_batches_++; n_queries_ += batch.size(); if (batch.size() > largest_) largest_ = batch.size();
      lk.unlock();
      flush(batch, k);
      lk.lock();
    }
  }
  size_t count_k(uint32_t k) const { size_t c = 0; for (auto& p : queue_) c += p->k == k; return c; }

  // hands one caller its answer: rc, and on success the first min(cnt, k) of ids / sc
  static void answer(std::shared_ptr<Pending>& p, int rc, uint32_t k, const uint64_t* ids, const float* sc, uint32_t cnt) {
    BatchAnswer a; a.rc = rc;
    if (rc == 0) {
      const uint32_t n = cnt < k ? cnt : k;
      a.items.resize(n);
      for (uint32_t j = 0; j < n; j++) a.items[j] = {ids[j], sc[j]};
    }
    p->done.set_value(std::move(a));
  }

  void flush(std::vector<std::shared_ptr<Pending>>& batch, uint32_t k) {
    const size_t nq = batch.size();
    if (k == 0) { for (auto& p : batch) answer(p, 0, 0, nullptr, nullptr, 0); return; }
    std::vector<float> flat(nq * dim_);
    std::vector<coltt_handle_t> fh(nq);
    for (size_t i = 0; i < nq; i++) {
      std::memcpy(flat.data() + i * dim_, batch[i]->q.data(), dim_ * sizeof(float));
      fh[i] = batch[i]->filter;
    }
    std::vector<uint64_t> ids(nq * (size_t)k);
    std::vector<float> sc(nq * (size_t)k);
    std::vector<uint32_t> cnt(nq, 0);
    const int rc = backend_(fh.data(), flat.data(), nq, k, ids.data(), sc.data(), cnt.data());
    if (rc == 0 || nq == 1) {
      for (size_t i = 0; i < nq; i++) answer(batch[i], rc, k, ids.data() + i * k, sc.data() + i * k, cnt[i]);
      return;
    }
    { std::lock_guard<std::mutex> g(mu_); n_retried_++; }   // counted before any caller of the batch is answered
    for (size_t i = 0; i < nq; i++) {   // the whole batch was refused: one query at a time, each caller gets its own call's result
      uint32_t c = 0;
      const int r = backend_(fh.data() + i, flat.data() + i * dim_, 1, k, ids.data(), sc.data(), &c);
      answer(batch[i], r, k, ids.data(), sc.data(), c);
    }
  }

  const uint32_t dim_; const size_t max_batch_; const std::chrono::microseconds max_wait_; Backend backend_;
  mutable std::mutex mu_; std::condition_variable cv_; std::deque<std::shared_ptr<Pending>> queue_;
  bool stop_ = false; uint64_t n_batches_ = 0, n_queries_ = 0, n_retried_ = 0; size_t largest_ = 0;
  std::thread worker_;  // last member: started after everything else is initialised
};

// A ready-made FilteredBatcher backend over the product-quantised walk: coltt_hnsw_pq_search_filtered_batch on `index` (which carries a quantiser:
// coltt_hnsw_pq_attach) with this `rerank`, ef and mode for every batch.  A filtered RPC served this way gets the answer of its own
// coltt_hnsw_pq_search_filtered call.
inline FilteredBatcher::Backend PqFilteredBackend(coltt_handle_t index, uint32_t rerank = 0, uint32_t ef = 0, int mode = COLTT_FILTER_AUTO) {
  return [index, rerank, ef, mode](const coltt_handle_t* filters, const float* queries, size_t nq, uint32_t k, uint64_t* ids, float* scores, uint32_t* counts) {
    return coltt_hnsw_pq_search_filtered_batch(index, filters, queries, nq, k, ef, rerank, mode, ids, scores, counts, nullptr, nullptr);
  };
}

// The micro-batcher for FLAT filtered searches (coltt_flat_search_ids_batch): the reference's FilterableVertexSearch RPC carries its own
// filter, which the inverted index turns into its own id list (edge/none_vectorstore.go:182-253); callers bring that list, batches are
// grouped by k only.  Backend = int(const float* queries, size_t nq, uint32_t k, const uint64_t* cand_ids, const uint64_t* list_offsets
// /*[nq + 1]: query i owns cand_ids[list_offsets[i] .. list_offsets[i+1])*/, uint64_t* ids, float* scores, uint32_t* counts).  A batch
// the backend refuses as a whole is re-issued one query at a time, and only the callers whose own call fails get its error.
class IdsBatcher {
 public:
  using Backend = std::function<int(const float*, size_t, uint32_t, const uint64_t*, const uint64_t*, uint64_t*, float*, uint32_t*)>;

  IdsBatcher(uint32_t dim, size_t max_batch, std::chrono::microseconds max_wait, Backend backend)
      : dim_(dim), max_batch_(max_batch ? max_batch : 1), max_wait_(max_wait), backend_(std::move(backend)),
        worker_([this] { loop(); }) {}
  ~IdsBatcher() {
    { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
    cv_.notify_all();
    worker_.join();
  }
  IdsBatcher(const IdsBatcher&) = delete;
  IdsBatcher& operator=(const IdsBatcher&) = delete;

  // blocks until answered; the query and the candidate ids are copied before returning to the collector
  BatchAnswer SearchIds(const float* query, uint32_t k, const uint64_t* cand_ids, size_t n_cand) {
    auto p = std::make_shared<Pending>();
    p->q.assign(query, query + dim_);
    if (n_cand) p->cand.assign(cand_ids, cand_ids + n_cand);
    p->k = k;
    std::future<BatchAnswer> f = p->done.get_future();
    {
      std::lock_guard<std::mutex> g(mu_);
      queue_.push_back(p);
    }
    cv_.notify_all();
    return f.get();
  }
  BatchAnswer SearchIds(const float* query, uint32_t k, const std::vector<uint64_t>& cand_ids) { return SearchIds(query, k, cand_ids.data(), cand_ids.size()); }

  // statistics (for tests / tuning); retried_batches: batches the backend refused as a whole and that were re-issued per query
  uint64_t batches() const { std::lock_guard<std::mutex> g(mu_); return n_batches_; }
  uint64_t queries() const { std::lock_guard<std::mutex> g(mu_); return n_queries_; }
  size_t largest_batch() const { std::lock_guard<std::mutex> g(mu_); return largest_; }
  uint64_t retried_batches() const { std::lock_guard<std::mutex> g(mu_); return n_retried_; }

 private:
  struct Pending { std::vector<float> q; std::vector<uint64_t> cand; uint32_t k = 0; std::promise<BatchAnswer> done; };

  void loop() {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      cv_.wait(lk, [this] { return stop_ || !queue_.empty(); });
      if (queue_.empty()) { if (stop_) return; continue; }
      const uint32_t k = queue_.front()->k;
      const auto deadline = std::chrono::steady_clock::now() + max_wait_;
      while (!stop_ && count_k(k) < max_batch_) {
        if (cv_.wait_until(lk, deadline) == std::cv_status::timeout) break;
      }
      std::vector<std::shared_ptr<Pending>> batch;
      for (auto it = queue_.begin(); it != queue_.end() && batch.size() < max_batch_;) {
        if ((*it)->k == k) { batch.push_back(*it); it = queue_.erase(it); } else ++it;
      }
      n_batches_++; n_queries_ += batch.size(); if (batch.size() > largest_) largest_ = batch.size();
      lk.unlock();
      flush(batch, k);
      lk.lock();
    }
  }
  size_t count_k(uint32_t k) const { size_t c = 0; for (auto& p : queue_) c += p->k == k; return c; }

  // hands one caller its answer: rc, and on success the first min(cnt, k) of ids / sc
  static void answer(std::shared_ptr<Pending>& p, int rc, uint32_t k, const uint64_t* ids, const float* sc, uint32_t cnt) {
    BatchAnswer a; a.rc = rc;
    if (rc == 0) {
      const uint32_t n = cnt < k ? cnt : k;
      a.items.resize(n);
      for (uint32_t j = 0; j < n; j++) a.items[j] = {ids[j], sc[j]};
    }
    p->done.set_value(std::move(a));
  }

  void flush(std::vector<std::shared_ptr<Pending>>& batch, uint32_t k) {
    const size_t nq = batch.size();
    if (k == 0) { for (auto& p : batch) answer(p, 0, 0, nullptr, nullptr, 0); return; }
    std::vector<float> flat(nq * dim_);
    std::vector<uint64_t> off(nq + 1, 0), cand;
    for (size_t i = 0; i < nq; i++) {
      std::memcpy(flat.data() + i * dim_, batch[i]->q.data(), dim_ * sizeof(float));
      cand.insert(cand.end(), batch[i]->cand.begin(), batch[i]->cand.end());
      off[i + 1] = cand.size();
    }
    std::vector<uint64_t> ids(nq * (size_t)k);
    std::vector<float> sc(nq * (size_t)k);
    std::vector<uint32_t> cnt(nq, 0);
    const int rc = backend_(flat.data(), nq, k, cand.data(), off.data(), ids.data(), sc.data(), cnt.data());
    if (rc == 0 || nq == 1) {
      for (size_t i = 0; i < nq; i++) answer(batch[i], rc, k, ids.data() + i * k, sc.data() + i * k, cnt[i]);
      return;
    }
    { std::lock_guard<std::mutex> g(mu_); n_retried_++; }   // counted before any caller of the batch is answered
    for (size_t i = 0; i < nq; i++) {   // the whole batch was refused: one query at a time, each caller gets its own call's result
      uint32_t c = 0;
      const uint64_t one[2] = {0, off[i + 1] - off[i]};
      const int r = backend_(flat.data() + i * dim_, 1, k, cand.data() + off[i], one, ids.data(), sc.data(), &c);
      answer(batch[i], r, k, ids.data(), sc.data(), c);
    }
  }

  const uint32_t dim_; const size_t max_batch_; const std::chrono::microseconds max_wait_; Backend backend_;
  mutable std::mutex mu_; std::condition_variable cv_; std::deque<std::shared_ptr<Pending>> queue_;
  bool stop_ = false; uint64_t n_batches_ = 0, n_queries_ = 0, n_retried_ = 0; size_t largest_ = 0;
  std::thread worker_;  // last member: started after everything else is initialised
};

// A ready-made IdsBatcher backend over a FLAT store: coltt_flat_search_ids_batch on `flat`, one list per query, this `select` for every
// batch.  A filtered RPC served this way gets the answer of its own coltt_flat_search_ids call.
inline IdsBatcher::Backend FlatIdsBackend(coltt_handle_t flat, int select = COLTT_SELECT_REFERENCE) {
  return [flat, select](const float* queries, size_t nq, uint32_t k, const uint64_t* cand_ids, const uint64_t* list_offsets, uint64_t* ids, float* scores, uint32_t* counts) {
    return coltt_flat_search_ids_batch(flat, queries, nq, k, select, cand_ids, list_offsets, nq, nullptr, ids, scores, counts);
  };
}

}  // namespace coltt
