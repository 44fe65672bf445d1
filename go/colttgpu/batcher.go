package colttgpu

import (
	"fmt"
	"sync"
	"time"
)

// Batcher coalesces the reference's one-query-per-RPC calls (core/core.go:633-695, edge/edge.go:610-690) into GPU batches:
// goroutines enqueue a query and block on a channel; the collector flushes when MaxBatch queries are waiting or MaxWait
// elapsed since the first of them and issues ONE batched search per distinct k.  Same semantics as the compiled C++ twin
// include/coltt_batcher.hpp (which is the one exercised on the GPU here — no Go toolchain in the build container):
//   - queries are GROUPED BY k: HNSW searches with ef = max(cfg.ef, k), so answers for different k are not prefixes of one
//     another; a k = 10 query batched with a k = 500 query must get exactly what a single-query call returns;
//   - k == 0 answers immediately with an empty result (hnsw.go:243-278 returns no rows), it never reaches the backend;
//   - len(query) != dim is an error for THAT caller only (C never reads past a short Go slice).
//
// Backend is any batched search: HnswBackend / FlatBackend below, or a test double.
type Backend func(queries []float32, nq int, k uint32) (ids []uint64, scores []float32, counts []uint32, err error)

type BatchItem struct {
	Id    uint64
	Score float32
}

type Batcher struct {
	dim      int
	backend  Backend
	fbackend FilteredBackend // set by NewFilteredBatcher: the filtered mode
	ibackend IdsBackend      // set by NewIdsBatcher: the ids mode
	MaxBatch int
	MaxWait  time.Duration
	in       chan *pending
	quit     chan struct{}
	closeOne sync.Once
}

type pending struct {
	q      []float32
	k      uint32
	filter Handle   // filtered mode: the caller's filter
	cand   []uint64 // ids mode: the caller's candidate ids
	done   chan batchResult
}
type batchResult struct {
	items []BatchItem
	err   error
}

func NewBatcher(dim int, backend Backend, maxBatch int, maxWait time.Duration) *Batcher {
	if maxBatch < 1 {
		maxBatch = 1
	}
	b := &Batcher{dim: dim, backend: backend, MaxBatch: maxBatch, MaxWait: maxWait, in: make(chan *pending, 4*maxBatch),
		quit: make(chan struct{})}
	go b.loop()
	return b
}

// Close stops the collector.  Queries still queued (or racing with Close) are answered with "batcher closed": no caller is left
// blocked on its done channel.  Safe to call more than once.
func (b *Batcher) Close() { b.closeOne.Do(func() { close(b.quit) }) }

var errClosed = fmt.Errorf("batcher closed")

// HnswBackend / FlatBackend: the two searches that need batching (BASELINE.json configs 2-5)
func HnswBackend(h Handle, dim uint32, ef uint32) Backend {
	return func(q []float32, nq int, k uint32) ([]uint64, []float32, []uint32, error) {
		return HnswSearch(h, dim, q, nq, k, ef)
	}
}
func FlatBackend(h Handle, dim uint32, sel, mode int) Backend {
	return func(q []float32, nq int, k uint32) ([]uint64, []float32, []uint32, error) {
		return FlatSearch(h, dim, q, nq, k, sel, mode, nil, false)
	}
}

// Filtered mode (same semantics as coltt::FilteredBatcher in include/coltt_batcher.hpp): every caller brings its own filter handle
// (HnswFilterCreate), batches are grouped by k only and mix any number of filters.  The batch call checks every handle before it runs
// anything, so one caller's bad filter (destroyed, stale, of another index) fails the whole call: the batch is then re-issued one query
// at a time and only the callers whose own call fails get its error.
type FilteredBackend func(filters []Handle, queries []float32, nq int, k uint32) (ids []uint64, scores []float32, counts []uint32, err error)

func HnswFilteredBackend(h Handle, dim uint32, ef uint32) FilteredBackend {
	return func(f []Handle, q []float32, nq int, k uint32) ([]uint64, []float32, []uint32, error) {
		ids, sc, cnt, _, err := HnswSearchFilteredBatch(h, f, dim, q, nq, k, ef, FilterAuto)
		return ids, sc, cnt, err
	}
}

// HnswPqFilteredBackend: the filtered mode over the walk on product-quantiser codes (coltt_hnsw_pq_search_filtered_batch) for an index that
// carries a quantiser; every caller gets the answer of its own HnswPqSearchFiltered call at this rerank.
func HnswPqFilteredBackend(h Handle, dim uint32, ef, rerank uint32) FilteredBackend {
	return func(f []Handle, q []float32, nq int, k uint32) ([]uint64, []float32, []uint32, error) {
		ids, sc, cnt, _, err := HnswPqSearchFilteredBatch(h, f, dim, q, nq, k, ef, rerank, FilterAuto)
		return ids, sc, cnt, err
	}
}

func NewFilteredBatcher(dim int, backend FilteredBackend, maxBatch int, maxWait time.Duration) *Batcher {
	if maxBatch < 1 {
		maxBatch = 1
	}
	b := &Batcher{dim: dim, fbackend: backend, MaxBatch: maxBatch, MaxWait: maxWait, in: make(chan *pending, 4*maxBatch),
		quit: make(chan struct{})}
	go b.loop()
	return b
}

// Ids mode (same semantics as coltt::IdsBatcher in include/coltt_batcher.hpp): every caller brings its own candidate id list — the
// reference's FilterableVertexSearch RPC, whose filter expression the inverted index has turned into ids (edge/none_vectorstore.go:182-253).
// Batches are grouped by k only; lists[i] belongs to query i.  A batch the backend refuses as a whole is re-issued one query at a time.
type IdsBackend func(lists [][]uint64, queries []float32, nq int, k uint32) (ids []uint64, scores []float32, counts []uint32, err error)

// FlatIdsBackend: FlatSearchIdsBatch on a FLAT store; every caller gets the answer of its own filtered FlatSearch call.
func FlatIdsBackend(h Handle, dim uint32, sel int) IdsBackend {
	return func(lists [][]uint64, q []float32, nq int, k uint32) ([]uint64, []float32, []uint32, error) {
		return FlatSearchIdsBatch(h, dim, q, nq, k, sel, lists, nil)
	}
}

func NewIdsBatcher(dim int, backend IdsBackend, maxBatch int, maxWait time.Duration) *Batcher {
	if maxBatch < 1 {
		maxBatch = 1
	}
	b := &Batcher{dim: dim, ibackend: backend, MaxBatch: maxBatch, MaxWait: maxWait, in: make(chan *pending, 4*maxBatch),
		quit: make(chan struct{})}
	go b.loop()
	return b
}

// SearchIds (ids mode) blocks until the batch this query rode in has been answered.  The ids are copied before they are queued.
func (b *Batcher) SearchIds(q []float32, k uint, cand []uint64) ([]BatchItem, error) {
	if b.ibackend == nil {
		return nil, fmt.Errorf("SearchIds: not an ids batcher (NewIdsBatcher)")
	}
	return b.search(q, k, 0, append([]uint64(nil), cand...))
}

// SearchFiltered (filtered mode) blocks until the batch this query rode in has been answered.
func (b *Batcher) SearchFiltered(q []float32, k uint, filter Handle) ([]BatchItem, error) {
	if b.fbackend == nil {
		return nil, fmt.Errorf("SearchFiltered: not a filtered batcher (NewFilteredBatcher)")
	}
	return b.search(q, k, filter, nil)
}

// Search blocks until the batch this query rode in has been answered.  The query is copied before it is queued.
func (b *Batcher) Search(q []float32, k uint) ([]BatchItem, error) {
	if b.fbackend != nil {
		return nil, fmt.Errorf("Search: a filtered batcher takes SearchFiltered")
	}
	if b.ibackend != nil {
		return nil, fmt.Errorf("Search: an ids batcher takes SearchIds")
	}
	return b.search(q, k, 0, nil)
}

func (b *Batcher) search(q []float32, k uint, filter Handle, cand []uint64) ([]BatchItem, error) {
	if len(q) != b.dim {
		return nil, fmt.Errorf("Dim Length UnmatchdError: expect dimension: [%d], but got [%d]", b.dim, len(q))
	}
	if k == 0 {
		return []BatchItem{}, nil
	}
	p := &pending{q: append([]float32(nil), q...), k: uint32(k), filter: filter, cand: cand, done: make(chan batchResult, 1)}
	select {
	case b.in <- p:
	case <-b.quit:
		return nil, errClosed
	}
	select {
	case r := <-p.done:
		return r.items, r.err
	case <-b.quit:
		// the collector may still answer (it drains on quit) — prefer its answer, never block
		select {
		case r := <-p.done:
			return r.items, r.err
		default:
			return nil, errClosed
		}
	}
}

func (b *Batcher) loop() {
	for {
		var first *pending
		select {
		case first = <-b.in:
		case <-b.quit:
			b.drain(nil)
			return
		}
		batch := []*pending{first}
		timer := time.NewTimer(b.MaxWait)
		closed := false
	collect:
		for len(batch) < b.MaxBatch {
			select {
			case p := <-b.in:
				batch = append(batch, p)
			case <-timer.C:
				break collect
			case <-b.quit:
				closed = true
				break collect
			}
		}
		timer.Stop()
		if closed {
			b.drain(batch)
			return
		}
		b.flush(batch)
	}
}

// drain answers the batch in hand and everything still queued with errClosed (done has capacity 1: never blocks)
func (b *Batcher) drain(batch []*pending) {
	for _, p := range batch {
		p.done <- batchResult{nil, errClosed}
	}
	for {
		select {
		case p := <-b.in:
			p.done <- batchResult{nil, errClosed}
		default:
			return
		}
	}
}

func (b *Batcher) flush(batch []*pending) {
	byK := map[uint32][]*pending{}
	var order []uint32
	for _, p := range batch {
		if _, ok := byK[p.k]; !ok {
			order = append(order, p.k)
		}
		byK[p.k] = append(byK[p.k], p)
	}
	for _, k := range order {
		grp := byK[k]
		nq := len(grp)
		flat := make([]float32, nq*b.dim) // the library copies inputs before returning: no Go pointer is retained
		for i, p := range grp {
			copy(flat[i*b.dim:], p.q)
		}
		if b.fbackend != nil {
			b.flushFiltered(grp, flat, k)
			continue
		}
		if b.ibackend != nil {
			b.flushIds(grp, flat, k)
			continue
		}
		ids, sc, cnt, err := b.backend(flat, nq, k)
		for i, p := range grp {
			if err != nil {
				p.done <- batchResult{nil, err}
				continue
			}
			n := int(cnt[i])
			items := make([]BatchItem, n)
			for j := 0; j < n; j++ {
				items[j] = BatchItem{Id: ids[i*int(k)+j], Score: sc[i*int(k)+j]}
			}
			p.done <- batchResult{items, nil}
		}
	}
}

func rows(ids []uint64, sc []float32, cnt uint32, k uint32, i int) []BatchItem {
	items := make([]BatchItem, int(cnt))
	for j := range items {
		items[j] = BatchItem{Id: ids[i*int(k)+j], Score: sc[i*int(k)+j]}
	}
	return items
}

// flushFiltered: one backend call for the group; if it fails as a whole, one call per query (each caller gets its own call's result)
func (b *Batcher) flushFiltered(grp []*pending, flat []float32, k uint32) {
	fh := make([]Handle, len(grp))
	for i, p := range grp {
		fh[i] = p.filter
	}
	ids, sc, cnt, err := b.fbackend(fh, flat, len(grp), k)
	if err == nil || len(grp) == 1 {
		for i, p := range grp {
			if err != nil {
				p.done <- batchResult{nil, err}
				continue
			}
			p.done <- batchResult{rows(ids, sc, cnt[i], k, i), nil}
		}
		return
	}
	for i, p := range grp {
		ids1, sc1, cnt1, err1 := b.fbackend(fh[i:i+1], flat[i*b.dim:(i+1)*b.dim], 1, k)
		if err1 != nil {
			p.done <- batchResult{nil, err1}
			continue
		}
		p.done <- batchResult{rows(ids1, sc1, cnt1[0], k, 0), nil}
	}
}

// flushIds: one backend call for the group, a list per query; if it fails as a whole, one call per query (each caller gets its own call's result)
func (b *Batcher) flushIds(grp []*pending, flat []float32, k uint32) {
	lists := make([][]uint64, len(grp))
	for i, p := range grp {
		lists[i] = p.cand
	}
	ids, sc, cnt, err := b.ibackend(lists, flat, len(grp), k)
	if err == nil || len(grp) == 1 {
		for i, p := range grp {
			if err != nil {
				p.done <- batchResult{nil, err}
				continue
			}
			p.done <- batchResult{rows(ids, sc, cnt[i], k, i), nil}
		}
		return
	}
	for i, p := range grp {
		ids1, sc1, cnt1, err1 := b.ibackend(lists[i:i+1], flat[i*b.dim:(i+1)*b.dim], 1, k)
		if err1 != nil {
			p.done <- batchResult{nil, err1}
			continue
		}
		p.done <- batchResult{rows(ids1, sc1, cnt1[0], k, 0), nil}
	}
}
