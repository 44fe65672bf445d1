// Package vectorindex — GPU-backed REPLACEMENT BODY for github.com/sjy-dv/coltt/core/vectorindex.
//
// `core` stores the concrete type *vectorindex.Hnsw (core/core.go:34,51), so there is no interface to plug into: the
// drop-in is source level — this directory replaces core/vectorindex and exports every identifier core, e2e and playground
// use (usage census SURVEY.md §8b): Hnsw, NewHnsw, HnswOption + the nine option constructors, HnswSearchSimple /
// HnswSearchHeuristic, ProtoConfig, Metadata, SearchResult{,Item}, Normalize, ItemNotFoundError, ItemAlreadyExistsError,
// and GetVertex whose result offers Id / Vector / Metadata / Level.
//
// Division of labour: vectors, the graph and every distance evaluation live in HBM behind libcoltt_gpu.so
// (go/colttgpu); Metadata maps never cross the boundary — this package keeps id -> Metadata and re-attaches it.
// NOT COMPILED in the build container (no Go toolchain); see INTEGRATION.md for the build line.
package vectorindex

import (
	"bytes"
	"context"
	"encoding/binary"
	"errors"
	"fmt"
	"io"
	"math"
	"math/rand"
	"strings"
	"sync"
	"sync/atomic"

	"github.com/sjy-dv/coltt/edge"
	"github.com/sjy-dv/coltt/go/colttgpu"
	"github.com/sjy-dv/coltt/pkg/distance"
	"github.com/vmihailenco/msgpack/v5"
)

var (
	ItemNotFoundError      error = errors.New("Item not found")      // hnsw.go:39
	ItemAlreadyExistsError error = errors.New("Item already exists") // hnsw.go:40
)

// ---------------------------------------------------------------------------------------------- config (hnsw_config.go)
var hnswSearchAlgorithmNames = [...]string{"Simple", "Heuristic", "Diverse"}

type hnswSearchAlgorithm int

const (
	HnswSearchSimple hnswSearchAlgorithm = iota
	HnswSearchHeuristic
	// HnswSearchDiverse is NOT in the reference (COLTT_HNSW_DIVERSE, include/coltt_gpu.h): neighbour selection with the diversity test of
	// the HNSW paper, which the reference's "heuristic" (hnsw.go:399-447) does not apply.  It builds a DIFFERENT graph than the reference
	// would: NewHnsw refuses it unless HnswAllowNonReferenceSelection(true) is passed as well.
	HnswSearchDiverse
)

func (a hnswSearchAlgorithm) String() string { return hnswSearchAlgorithmNames[a] }

type hnswConfig struct {
	searchAlgorithm           hnswSearchAlgorithm
	levelMultiplier           float32
	ef, efConstruction        int
	m, mMax, mMax0            int
	heuristicExtendCandidates bool
	heuristicKeepPruned       bool
	quantization              int // extension (BASELINE.json configs[4]): 0 none, 1 f16, 2 f8, 3 "bf16" — edgepb.Quantization order
	allowNonReference         bool // opt-in for HnswSearchDiverse
}

// HnswOption — functional options, hnsw_config.go:43-109
type HnswOption interface{ apply(*hnswConfig) }
type hnswOption struct{ f func(*hnswConfig) }

func (o *hnswOption) apply(c *hnswConfig) { o.f(c) }

func HnswLevelMultiplier(v float32) HnswOption {
	return &hnswOption{func(c *hnswConfig) { c.levelMultiplier = v }}
}
func HnswEf(v int) HnswOption             { return &hnswOption{func(c *hnswConfig) { c.ef = v }} }
func HnswEfConstruction(v int) HnswOption { return &hnswOption{func(c *hnswConfig) { c.efConstruction = v }} }
func HnswM(v int) HnswOption              { return &hnswOption{func(c *hnswConfig) { c.m = v }} }
func HnswMmax(v int) HnswOption           { return &hnswOption{func(c *hnswConfig) { c.mMax = v }} }
func HnswMmax0(v int) HnswOption          { return &hnswOption{func(c *hnswConfig) { c.mMax0 = v }} }
func HnswSearchAlgorithm(v hnswSearchAlgorithm) HnswOption {
	return &hnswOption{func(c *hnswConfig) { c.searchAlgorithm = v }}
}
func HnswHeuristicExtendCandidates(v bool) HnswOption {
	return &hnswOption{func(c *hnswConfig) { c.heuristicExtendCandidates = v }}
}
func HnswHeuristicKeepPruned(v bool) HnswOption {
	return &hnswOption{func(c *hnswConfig) { c.heuristicKeepPruned = v }}
}

// HnswAllowNonReferenceSelection opts in to HnswSearchDiverse: without it a drop-in user can never get a graph the reference would not build.
func HnswAllowNonReferenceSelection(v bool) HnswOption {
	return &hnswOption{func(c *hnswConfig) { c.allowNonReference = v }}
}

// HnswQuantization is NOT in the reference: stored rows become 2-/1-byte codes scored as the edge quantised stores do.
func HnswQuantization(q int) HnswOption { return &hnswOption{func(c *hnswConfig) { c.quantization = q }} }

// ProtoConfig — hnsw_config.go:123-133
type ProtoConfig struct {
	SearchAlgorithm           string
	LevelMultiplier           float32
	Ef                        int
	EfConstruction            int
	M                         int
	MMax                      int
	MMax0                     int
	HeuristicExtendCandidates bool
	HeuristicKeepPruned       bool
}

func b2i(b bool) int32 {
	if b {
		return 1
	}
	return 0
}

// ---------------------------------------------------------------------------------------------- Metadata (metadata.go)
type Metadata map[string]any

// encode = Metadata.save (metadata.go:31-74): u16 pairs, each {u8 keylen, key, u16 vallen, msgpack(value)}
func (m Metadata) encode() ([]byte, error) {
	var b bytes.Buffer
	if err := binary.Write(&b, binary.BigEndian, uint16(len(m))); err != nil {
		return nil, err
	}
	for k, v := range m {
		if len(k) > 255 {
			return nil, fmt.Errorf("metadata key too long: %s", k)
		}
		b.WriteByte(uint8(len(k)))
		b.WriteString(k)
		vb, err := msgpack.Marshal(v)
		if err != nil {
			return nil, err
		}
		if err := binary.Write(&b, binary.BigEndian, uint16(len(vb))); err != nil {
			return nil, err
		}
		b.Write(vb)
	}
	return b.Bytes(), nil
}

// decodeMetadata = Metadata.load (metadata.go:43-105) over the blob the library located inside the stream
func decodeMetadata(blob []byte) (Metadata, error) {
	r := bytes.NewReader(blob)
	var n uint16
	if err := binary.Read(r, binary.BigEndian, &n); err != nil {
		return nil, err
	}
	m := make(Metadata, n)
	for i := 0; i < int(n); i++ {
		var kl uint8
		if err := binary.Read(r, binary.BigEndian, &kl); err != nil {
			return nil, err
		}
		kb := make([]byte, kl)
		if _, err := io.ReadFull(r, kb); err != nil {
			return nil, err
		}
		var vl uint16
		if err := binary.Read(r, binary.BigEndian, &vl); err != nil {
			return nil, err
		}
		vb := make([]byte, vl)
		if _, err := io.ReadFull(r, vb); err != nil {
			return nil, err
		}
		var v any
		if err := msgpack.Unmarshal(vb, &v); err != nil {
			return nil, err
		}
		m[string(kb)] = v
	}
	return m, nil
}

// Normalize — metadata.go:107-123.  Kept as an identifier for callers (core/core_helper.go).  The arithmetic has ONE copy, in the
// library, and this calls its host-side entry (coltt_normalize_host): no device work, no allocation beyond the result, infallible — as
// the reference's.
func Normalize(v []float32) []float32 { return colttgpu.Normalize(v) }

// ---------------------------------------------------------------------------------------------- results (search.go)
type SearchResult []SearchResultItem
type SearchResultItem struct {
	Id       uint64
	Metadata map[string]any
	Score    float32
}

func (xx SearchResult) Len() int           { return len(xx) }
func (xx SearchResult) Swap(i, j int)      { xx[i], xx[j] = xx[j], xx[i] }
func (xx SearchResult) Less(i, j int) bool { return xx[i].Score < xx[j].Score }

// hnswVertex — what GetVertex hands out (core/core.go:512-517,607 read .Metadata()); a value snapshot, not a live node
type hnswVertex struct {
	id       uint64
	vector   edge.Vector
	metadata Metadata
	level    int
}

func (v *hnswVertex) Id() uint64          { return v.id }
func (v *hnswVertex) Vector() edge.Vector { return v.vector }
func (v *hnswVertex) Metadata() Metadata  { return v.metadata }
func (v *hnswVertex) Level() int          { return v.level }

// ---------------------------------------------------------------------------------------------- Hnsw (hnsw.go:43-54)
const metaShards = 16

type Hnsw struct {
	dim       uint
	distancer distance.Space
	config    *hnswConfig
	h         colttgpu.Handle
	bytesSize uint64 // sum of vector + metadata bytes of live vertices (hnsw_vertex.go:123-127), Go side
	meta      [metaShards]map[uint64]Metadata
	metaMu    [metaShards]sync.RWMutex
	commitMu  sync.RWMutex // Insert / Remove hold it shared, Commit exclusive: a snapshot never interleaves with a mutation
	err       error // creation error, surfaced by the first call (NewHnsw has no error result in the reference)
	// the open filters and attribute columns made through this object: Compact carries them (coltt_hnsw_compact_carry)
	carryMu sync.Mutex
	filters map[*HnswFilter]struct{}
	columns map[*AttrColumn]struct{}
}

// trackFilter / trackColumn register an open object with its index; Close takes it out again.
func (xx *Hnsw) trackFilter(f *HnswFilter) *HnswFilter {
	xx.carryMu.Lock()
	if xx.filters == nil {
		xx.filters = make(map[*HnswFilter]struct{})
	}
	xx.filters[f] = struct{}{}
	xx.carryMu.Unlock()
	return f
}
func (xx *Hnsw) trackColumn(c *AttrColumn) *AttrColumn {
	xx.carryMu.Lock()
	if xx.columns == nil {
		xx.columns = make(map[*AttrColumn]struct{})
	}
	xx.columns[c] = struct{}{}
	xx.carryMu.Unlock()
	return c
}

func metric(d distance.Space) int {
	if d.Type() == "cosine-dot" { // pkg/distance/space.go:101
		return 0
	}
	return 1
}

// NewHnsw(dim, distancer, options...) — hnsw.go:56-73; defaults hnsw_config.go:135-162 are filled in by the library (-1).
func NewHnsw(dim uint, distancer distance.Space, option ...HnswOption) *Hnsw {
	c := &hnswConfig{searchAlgorithm: HnswSearchSimple, levelMultiplier: -1, ef: 20, efConstruction: 200, m: 16, mMax: -1, mMax0: -1,
		heuristicKeepPruned: true}
	for _, o := range option {
		o.apply(c)
	}
	x := &Hnsw{dim: dim, distancer: distancer, config: c}
	for i := range x.meta {
		x.meta[i] = make(map[uint64]Metadata)
	}
	if c.searchAlgorithm == HnswSearchDiverse && !c.allowNonReference {
		x.err = fmt.Errorf("HnswSearchDiverse is not reference behaviour: pass HnswAllowNonReferenceSelection(true) to opt in")
		return x
	}
	cfg := colttgpu.HnswCfg{M: int32(c.m), MMax: int32(c.mMax), MMax0: int32(c.mMax0), Ef: int32(c.ef), EfConstruction: int32(c.efConstruction),
		Algo: int32(c.searchAlgorithm), LevelMultiplier: c.levelMultiplier, ExtendCandidates: b2i(c.heuristicExtendCandidates),
		KeepPruned: b2i(c.heuristicKeepPruned)}
	x.h, x.err = colttgpu.HnswCreate(uint32(dim), metric(distancer), c.quantization, &cfg)
	if x.err == nil {
		x.refreshConfig()
	}
	return x
}

func (xx *Hnsw) refreshConfig() {
	if c, err := colttgpu.HnswGetCfg(xx.h); err == nil {
		xx.config.searchAlgorithm = hnswSearchAlgorithm(c.Algo)
		xx.config.levelMultiplier = c.LevelMultiplier
		xx.config.ef, xx.config.efConstruction = int(c.Ef), int(c.EfConstruction)
		xx.config.m, xx.config.mMax, xx.config.mMax0 = int(c.M), int(c.MMax), int(c.MMax0)
		xx.config.heuristicExtendCandidates, xx.config.heuristicKeepPruned = c.ExtendCandidates != 0, c.KeepPruned != 0
	}
}

func (xx *Hnsw) Close() { colttgpu.HnswDestroy(xx.h) }

func (xx *Hnsw) Info() string {
	c := xx.config
	return fmt.Sprintf("HNSW(dim: %d, distancer: %s, config={searchAlgorithm: %s, ef: %d, efConstruction: %d, m: %d, mMax: %d, mMax0: %d, levelMultiplier: %.4f, extendCandidates: %t, keepPruned: %t})",
		xx.dim, xx.distancer.Type(), c.searchAlgorithm, c.ef, c.efConstruction, c.m, c.mMax, c.mMax0, c.levelMultiplier,
		c.heuristicExtendCandidates, c.heuristicKeepPruned)
}
func (xx *Hnsw) Dim() uint32 { return uint32(xx.dim) }
func (xx *Hnsw) Len() int    { return colttgpu.HnswLen(xx.h) }
func (xx *Hnsw) Config() ProtoConfig { // hnsw.go:86-98
	c := xx.config
	return ProtoConfig{SearchAlgorithm: strings.ToLower(c.searchAlgorithm.String()), LevelMultiplier: c.levelMultiplier, Ef: c.ef,
		EfConstruction: c.efConstruction, M: c.m, MMax: c.mMax, MMax0: c.mMax0,
		HeuristicExtendCandidates: c.heuristicExtendCandidates, HeuristicKeepPruned: c.heuristicKeepPruned}
}
func (xx *Hnsw) Distance() string { return xx.distancer.Type() } // hnsw.go:100-102

func (xx *Hnsw) shard(id uint64) int { return int(id % metaShards) }

func mapErr(err error) error {
	switch err {
	case colttgpu.ErrNotFound:
		return ItemNotFoundError
	case colttgpu.ErrExists:
		return ItemAlreadyExistsError
	}
	return err
}

func metaBytes(m Metadata) uint64 { // coarse stand-in for Metadata.byteSize (metadata.go:125-132)
	var n uint64
	for k, v := range m {
		n += uint64(len(k)) + 16
		if s, ok := v.(string); ok {
			n += uint64(len(s))
		}
	}
	return n
}

// Insert(id, value, metadata, vertexLevel) — hnsw.go:104-167
func (xx *Hnsw) Insert(id uint64, value edge.Vector, metadata Metadata, vertexLevel int) error {
	if xx.err != nil {
		return xx.err
	}
	xx.commitMu.RLock()
	defer xx.commitMu.RUnlock()
	s := xx.shard(id)
	// the metadata is in place BEFORE the id becomes searchable (a concurrent Search must never see the id without it);
	// on failure it is taken out again unless the id already existed
	xx.metaMu[s].Lock()
	_, had := xx.meta[s][id]
	if !had {
		xx.meta[s][id] = metadata
	}
	xx.metaMu[s].Unlock()
	if err := colttgpu.HnswInsert(xx.h, uint32(xx.dim), id, value, vertexLevel); err != nil {
		if !had {
			xx.metaMu[s].Lock()
			delete(xx.meta[s], id)
			xx.metaMu[s].Unlock()
		}
		return mapErr(err)
	}
	atomic.AddUint64(&xx.bytesSize, uint64(len(value))*4+metaBytes(metadata))
	return nil
}

// Get(id) — hnsw.go:169-178
func (xx *Hnsw) Get(id uint64) (edge.Vector, error) {
	v, _, err := colttgpu.HnswGet(xx.h, uint32(xx.dim), id)
	if err != nil {
		return nil, mapErr(err)
	}
	return edge.Vector(v), nil
}

// GetVertex(id) — hnsw.go:180-189
func (xx *Hnsw) GetVertex(id uint64) (*hnswVertex, error) {
	v, lv, err := colttgpu.HnswGet(xx.h, uint32(xx.dim), id)
	if err != nil {
		return nil, mapErr(err)
	}
	s := xx.shard(id)
	xx.metaMu[s].RLock()
	m := xx.meta[s][id]
	xx.metaMu[s].RUnlock()
	return &hnswVertex{id: id, vector: edge.Vector(v), metadata: m, level: lv}, nil
}

// Remove(id) — hnsw.go:191-241
func (xx *Hnsw) Remove(id uint64) error {
	xx.commitMu.RLock()
	defer xx.commitMu.RUnlock()
	if err := colttgpu.HnswRemove(xx.h, id); err != nil {
		return mapErr(err)
	}
	s := xx.shard(id)
	xx.metaMu[s].Lock()
	m := xx.meta[s][id]
	delete(xx.meta[s], id)
	xx.metaMu[s].Unlock()
	atomic.AddUint64(&xx.bytesSize, ^(uint64(xx.dim)*4 + metaBytes(m) - 1))
	return nil
}

// Search(ctx, query, k) — hnsw.go:243-278.  One query per call as in the reference; Batcher (batcher.go) coalesces callers.
func (xx *Hnsw) Search(_ context.Context, query edge.Vector, k uint) (SearchResult, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	ids, sc, cnt, err := colttgpu.HnswSearch(xx.h, uint32(xx.dim), query, 1, uint32(k), 0)
	if err != nil {
		return nil, err
	}
	return xx.attach(ids, sc, int(cnt[0])), nil
}

// HnswFilter — an allow-list of ids for SearchFiltered.  NOT reference behaviour: the reference has no filtered HNSW search (its
// Core.HybridSearch post-filters an unfiltered one, core/core.go:760-836).  Built against one index; ids inserted later are not allowed,
// removed ones are never returned; a Load makes it stale (SearchFiltered then fails).  Close releases its device memory.
type HnswFilter struct {
	h       colttgpu.Handle
	index   *Hnsw
	Allowed uint64 // live vertices the filter allows
	stale   bool   // a Load renumbered the index since: Compact does not list it
}

// NewFilter builds a filter from ids (unknown / removed ids are ignored, duplicates count once).
func (xx *Hnsw) NewFilter(ids []uint64) (*HnswFilter, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	f, n, err := colttgpu.HnswFilterCreate(xx.h, ids)
	if err != nil {
		return nil, err
	}
	return xx.trackFilter(&HnswFilter{h: f, index: xx, Allowed: n}), nil
}

// Handle: the library's handle of the filter (colttgpu.Batcher.SearchFiltered takes it)
func (f *HnswFilter) Handle() colttgpu.Handle { return f.h }

// Handle: the library's handle of the index (colttgpu.HnswFilteredBackend takes it)
func (xx *Hnsw) Handle() colttgpu.Handle { return xx.h }

func (f *HnswFilter) Close() error {
	if f.h == 0 {
		return nil
	}
	if f.index != nil {
		f.index.carryMu.Lock()
		delete(f.index.filters, f)
		f.index.carryMu.Unlock()
	}
	err := colttgpu.HnswFilterDestroy(f.h)
	f.h = 0
	return err
}

// FilterExpr — a filter expression over resident filters, the shape of the reference's composite filters (pkg/inverted/search.go:50-77,
// evaluateCompositeFilter): a leaf is Leaf(i) = the i-th filter of the table given to EvalFilter, inner nodes are And / Or / AndNot / Not,
// All() is every live vertex.  Postfix() is the programme the library evaluates on the device.
type FilterExpr struct {
	op   int32 // >= 0: leaf index (pred: predicate index); otherwise a colttgpu.Fop*
	pred bool  // op counts in the predicate table of EvalFilterAttr, which follows the leaf table in the programme's numbering
	args []FilterExpr
}

func Leaf(i int) FilterExpr { return FilterExpr{op: int32(i)} }

// Pred(i) = the i-th predicate of the table given to EvalFilterAttr: a comparison over an attribute column, standing wherever a Leaf can.
func Pred(i int) FilterExpr { return FilterExpr{op: int32(i), pred: true} }
func All() FilterExpr       { return FilterExpr{op: colttgpu.FopAll} }
func Not(a FilterExpr) FilterExpr {
	return FilterExpr{op: colttgpu.FopNot, args: []FilterExpr{a}}
}
func AndNot(a, b FilterExpr) FilterExpr {
	return FilterExpr{op: colttgpu.FopAndNot, args: []FilterExpr{a, b}}
}

// And / Or of two or more operands fold from the left, so the stack stays at two values however many terms a request has.
func And(a, b FilterExpr, more ...FilterExpr) FilterExpr {
	return FilterExpr{op: colttgpu.FopAnd, args: append([]FilterExpr{a, b}, more...)}
}
func Or(a, b FilterExpr, more ...FilterExpr) FilterExpr {
	return FilterExpr{op: colttgpu.FopOr, args: append([]FilterExpr{a, b}, more...)}
}

func (e FilterExpr) Postfix() []int32 { return e.postfix(nil, 0) }

// PostfixAttr: the programme of EvalFilterAttr over nLeaves leaves: Pred(i) is the value nLeaves + i.
func (e FilterExpr) PostfixAttr(nLeaves int) []int32 { return e.postfix(nil, int32(nLeaves)) }
func (e FilterExpr) postfix(out []int32, nLeaves int32) []int32 {
	if e.op >= 0 && e.pred {
		return append(out, nLeaves+e.op)
	}
	if e.op >= 0 || e.op == colttgpu.FopAll {
		return append(out, e.op)
	}
	out = e.args[0].postfix(out, nLeaves)
	if e.op == colttgpu.FopNot {
		return append(out, e.op)
	}
	for _, a := range e.args[1:] {
		out = a.postfix(out, nLeaves)
		out = append(out, e.op)
	}
	return out
}

// EvalFilter evaluates expr over the resident filters `leaves` on the device (coltt_hnsw_filter_eval).  The result is an ordinary,
// immutable HnswFilter: exactly NewFilter over the ids of the live vertices the expression allows.  Not and All see vertices inserted
// after their operands were built; And / Or / AndNot of plain leaves do not.  Refreshing a term ("add these ids, drop those") is
// EvalFilter(AndNot(Or(Leaf(0), Leaf(1)), Leaf(2)), old, NewFilter(added), NewFilter(dropped)).
func (xx *Hnsw) EvalFilter(expr FilterExpr, leaves ...*HnswFilter) (*HnswFilter, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	lh := make([]colttgpu.Handle, len(leaves))
	for i, l := range leaves {
		if l == nil {
			return nil, fmt.Errorf("EvalFilter: no filter at leaf %d", i)
		}
		lh[i] = l.h
	}
	f, n, err := colttgpu.HnswFilterEval(xx.h, expr.Postfix(), lh)
	if err != nil {
		return nil, err
	}
	return xx.trackFilter(&HnswFilter{h: f, index: xx, Allowed: n}), nil
}

// EvalFilters: one filter per expression over a shared leaf table in one call (coltt_hnsw_filter_eval_batch): two kernel launches and
// two device allocations whatever len(exprs) is.  One bad expression or leaf fails the whole call and nothing is created.
func (xx *Hnsw) EvalFilters(exprs []FilterExpr, leaves ...*HnswFilter) ([]*HnswFilter, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	lh := make([]colttgpu.Handle, len(leaves))
	for i, l := range leaves {
		if l == nil {
			return nil, fmt.Errorf("EvalFilters: no filter at leaf %d", i)
		}
		lh[i] = l.h
	}
	progs := make([][]int32, len(exprs))
	for i, e := range exprs {
		progs[i] = e.Postfix()
	}
	hs, ns, err := colttgpu.HnswFilterEvalBatch(xx.h, progs, lh)
	if err != nil {
		return nil, err
	}
	out := make([]*HnswFilter, len(hs))
	for i := range hs {
		out[i] = xx.trackFilter(&HnswFilter{h: hs[i], index: xx, Allowed: ns[i]})
	}
	return out, nil
}

// AttrColumn — a numeric field beside the index: one int64 (colttgpu.AttrI64) or float64 (colttgpu.AttrF64) per vertex on the device
// (coltt_gpu.h, "Attribute columns and predicates").  NOT reference behaviour: the reference keeps a bitmap per distinct value of a field
// and, for every operator but OpEqual, walks all of them per request (pkg/inverted/search.go:36-45).  A vertex never set — or inserted after
// the last Set, or re-inserted by Update, which is Remove + Insert — holds no value and satisfies no comparison.  Load makes the column
// stale: build a new one by ids.  (*Hnsw).Compact carries the open columns along.  Close releases its device memory.
type AttrColumn struct {
	h     colttgpu.Handle
	index *Hnsw
	Type  int
	stale bool // a Load renumbered the index since: Compact does not list it
}

func (xx *Hnsw) NewAttrColumn(typ int) (*AttrColumn, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	c, err := colttgpu.HnswAttrCreate(xx.h, typ)
	if err != nil {
		return nil, err
	}
	return xx.trackColumn(&AttrColumn{h: c, index: xx, Type: typ}), nil
}

func (c *AttrColumn) Handle() colttgpu.Handle { return c.h }

// SetI64 / SetF64: ids -> values; unknown and removed ids are ignored, an id repeated takes its last value; returns the vertices set.
func (c *AttrColumn) SetI64(ids []uint64, values []int64) (uint64, error) {
	if c.Type != colttgpu.AttrI64 {
		return 0, errors.New("AttrColumn.SetI64: the column holds float64 values")
	}
	return colttgpu.HnswAttrSetI64(c.h, ids, values)
}
func (c *AttrColumn) SetF64(ids []uint64, values []float64) (uint64, error) {
	if c.Type != colttgpu.AttrF64 {
		return 0, errors.New("AttrColumn.SetF64: the column holds int64 values")
	}
	return colttgpu.HnswAttrSetF64(c.h, ids, values)
}

// Get: the raw 8-byte values of ids (math.Float64frombits for a float64 column) and whether each vertex holds one.
func (c *AttrColumn) Get(ids []uint64) ([]uint64, []bool, error) { return colttgpu.HnswAttrGet(c.h, ids) }

func (c *AttrColumn) Close() error {
	if c.h == 0 {
		return nil
	}
	if c.index != nil {
		c.index.carryMu.Lock()
		delete(c.index.columns, c)
		c.index.carryMu.Unlock()
	}
	err := colttgpu.HnswAttrDestroy(c.h)
	c.h = 0
	return err
}

// PredFromFilter translates one comparison of the reference's filter language — inverted.Filter{IndexName, Op, Value}
// (pkg/inverted/filter.go:40-44); op is the FilterOp, whose order colttgpu.Cmp* keeps — into a predicate over the column registered under
// IndexName.  An int / int64 value goes to an int64 column, a float32 / float64 value to a float64 column; anything else, and a value whose
// kind is not the column's, is an error (mixed comparison is the caller's conversion).
func PredFromFilter(columns map[string]*AttrColumn, indexName string, op int, value interface{}) (colttgpu.AttrPred, error) {
	c, ok := columns[indexName]
	if !ok || c == nil {
		return colttgpu.AttrPred{}, fmt.Errorf("PredFromFilter: no attribute column for index %q", indexName)
	}
	if op < int(colttgpu.CmpEq) || op > int(colttgpu.CmpLe) {
		return colttgpu.AttrPred{}, fmt.Errorf("PredFromFilter: unknown FilterOp %d", op)
	}
	switch v := value.(type) {
	case int:
		if c.Type == colttgpu.AttrI64 {
			return colttgpu.AttrPredI64(c.h, int32(op), int64(v)), nil
		}
	case int64:
		if c.Type == colttgpu.AttrI64 {
			return colttgpu.AttrPredI64(c.h, int32(op), v), nil
		}
	case float32:
		if c.Type == colttgpu.AttrF64 {
			return colttgpu.AttrPredF64(c.h, int32(op), float64(v)), nil
		}
	case float64:
		if c.Type == colttgpu.AttrF64 {
			return colttgpu.AttrPredF64(c.h, int32(op), v), nil
		}
	default:
		return colttgpu.AttrPred{}, fmt.Errorf("PredFromFilter: a %T value is neither an integer nor a float", value)
	}
	return colttgpu.AttrPred{}, fmt.Errorf("PredFromFilter: a %T value against column %q of the other type", value, indexName)
}

// EvalFilterAttr evaluates expr over resident filters and predicates on the device (coltt_hnsw_filter_eval_attr): Leaf(i) is leaves[i],
// Pred(i) is preds[i].  The result is an ordinary HnswFilter, exactly NewFilter over the ids the expression allows; Not and All see
// vertices without a value and newer vertices, a bare predicate does not.
func (xx *Hnsw) EvalFilterAttr(expr FilterExpr, leaves []*HnswFilter, preds []colttgpu.AttrPred) (*HnswFilter, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	lh := make([]colttgpu.Handle, len(leaves))
	for i, l := range leaves {
		if l == nil {
			return nil, fmt.Errorf("EvalFilterAttr: no filter at leaf %d", i)
		}
		lh[i] = l.h
	}
	f, n, err := colttgpu.HnswFilterEvalAttr(xx.h, expr.PostfixAttr(len(leaves)), lh, preds)
	if err != nil {
		return nil, err
	}
	return xx.trackFilter(&HnswFilter{h: f, index: xx, Allowed: n}), nil
}

// Ids: the ids the filter allows, in ascending slot order (gathered on the device)
func (f *HnswFilter) Ids() ([]uint64, error) {
	ids, _, err := colttgpu.HnswFilterIds(f.h, f.Allowed)
	return ids, err
}

// SearchFiltered(ctx, query, k, f) — the k nearest among the vertices f allows (the library's AUTO path: a filtered walk, or an exact
// scan of the allowed rows when the filter is selective).
func (xx *Hnsw) SearchFiltered(_ context.Context, query edge.Vector, k uint, f *HnswFilter) (SearchResult, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	ids, sc, cnt, err := colttgpu.HnswSearchFiltered(xx.h, f.h, uint32(xx.dim), query, 1, uint32(k), 0, colttgpu.FilterAuto)
	if err != nil {
		return nil, err
	}
	return xx.attach(ids, sc, int(cnt[0])), nil
}

// SearchFilteredPq(ctx, query, k, f, rerank) — SearchFiltered over the walk on product-quantiser codes, for an index that carries a quantiser
// (colttgpu.HnswPqAttach(xx.Handle(), pq)); rerank as colttgpu.HnswPqSearch (0: every member of the allowed set is re-scored exactly).
// The library's AUTO path, by the rule of SearchFiltered.
func (xx *Hnsw) SearchFilteredPq(_ context.Context, query edge.Vector, k uint, f *HnswFilter, rerank uint) (SearchResult, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	ids, sc, cnt, err := colttgpu.HnswPqSearchFiltered(xx.h, f.h, uint32(xx.dim), query, 1, uint32(k), 0, uint32(rerank), colttgpu.FilterAuto)
	if err != nil {
		return nil, err
	}
	return xx.attach(ids, sc, int(cnt[0])), nil
}

// PqNbrStats — the neighbourhood blocks the product-quantised walk reads (colttgpu.HnswPqNbrStats): built whole by the first walk that needs them, kept
// current by Insert and Remove afterwards (State 1); Load, a new quantiser or a grown capacity leave them stale (State 2) for the next walk to rebuild.
func (xx *Hnsw) PqNbrStats() (colttgpu.PqNbrStats, error) {
	if xx.err != nil {
		return colttgpu.PqNbrStats{}, xx.err
	}
	return colttgpu.HnswPqNbrStats(xx.h)
}

// PqFetchNbr — the blocks of slots [first, first + n) as the walk reads them, [n][mMax0][rowBytes] (colttgpu.HnswPqFetchNbr; rowBytes = the quantiser's
// sub-vector count rounded up to 16).  Test / diagnostics.
func (xx *Hnsw) PqFetchNbr(first, n uint64, rowBytes uint32) ([]byte, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	cfg, err := colttgpu.HnswGetCfg(xx.h)
	if err != nil {
		return nil, err
	}
	return colttgpu.HnswPqFetchNbr(xx.h, first, n, uint32(cfg.MMax0), rowBytes)
}

// SearchFilteredBatch(ctx, queries, k, filters) — a filter per query in one call: result i == SearchFiltered(ctx, queries[i], k, filters[i]).
// One bad filter (closed, stale, of another index) fails the whole call; the micro-batcher's filtered mode (colttgpu.FilteredBatcher)
// re-issues such a batch one query at a time.
func (xx *Hnsw) SearchFilteredBatch(_ context.Context, queries []edge.Vector, k uint, filters []*HnswFilter) ([]SearchResult, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	if len(filters) != len(queries) {
		return nil, fmt.Errorf("SearchFilteredBatch: %d filters for %d queries", len(filters), len(queries))
	}
	nq := len(queries)
	flat := make([]float32, 0, nq*int(xx.dim))
	fh := make([]colttgpu.Handle, nq)
	for i, q := range queries {
		if filters[i] == nil {
			return nil, fmt.Errorf("SearchFilteredBatch: no filter at position %d", i)
		}
		flat = append(flat, q...)
		fh[i] = filters[i].h
	}
	ids, sc, cnt, _, err := colttgpu.HnswSearchFilteredBatch(xx.h, fh, uint32(xx.dim), flat, nq, uint32(k), 0, colttgpu.FilterAuto)
	if err != nil {
		return nil, err
	}
	out := make([]SearchResult, nq)
	for i := range out {
		out[i] = xx.attach(ids[i*int(k):], sc[i*int(k):], int(cnt[i]))
	}
	return out, nil
}

// SearchFilteredPqBatch(ctx, queries, k, filters, rerank) — a filter per query over the walk on product-quantiser codes in one call: result i ==
// SearchFilteredPq(ctx, queries[i], k, filters[i], rerank).  One bad filter fails the whole call, as in SearchFilteredBatch.
func (xx *Hnsw) SearchFilteredPqBatch(_ context.Context, queries []edge.Vector, k uint, filters []*HnswFilter, rerank uint) ([]SearchResult, error) {
	if xx.err != nil {
		return nil, xx.err
	}
	if len(filters) != len(queries) {
		return nil, fmt.Errorf("SearchFilteredPqBatch: %d filters for %d queries", len(filters), len(queries))
	}
	nq := len(queries)
	flat := make([]float32, 0, nq*int(xx.dim))
	fh := make([]colttgpu.Handle, nq)
	for i, q := range queries {
		if filters[i] == nil {
			return nil, fmt.Errorf("SearchFilteredPqBatch: no filter at position %d", i)
		}
		flat = append(flat, q...)
		fh[i] = filters[i].h
	}
	ids, sc, cnt, _, err := colttgpu.HnswPqSearchFilteredBatch(xx.h, fh, uint32(xx.dim), flat, nq, uint32(k), 0, uint32(rerank), colttgpu.FilterAuto)
	if err != nil {
		return nil, err
	}
	out := make([]SearchResult, nq)
	for i := range out {
		out[i] = xx.attach(ids[i*int(k):], sc[i*int(k):], int(cnt[i]))
	}
	return out, nil
}

func (xx *Hnsw) attach(ids []uint64, sc []float32, n int) SearchResult {
	res := make(SearchResult, n)
	for i := 0; i < n; i++ {
		s := xx.shard(ids[i])
		xx.metaMu[s].RLock()
		res[i] = SearchResultItem{Id: ids[i], Score: sc[i], Metadata: xx.meta[s][ids[i]]}
		xx.metaMu[s].RUnlock()
	}
	return res
}

// RandomLevel — hnsw.go:280-282: the uniform draw stays with Go's global math/rand (gomath/rand.go:42-44), the library applies
// gomath.Floor(-gomath.Log(u) * levelMultiplier).  u = 0 (the reference's Floor(+Inf)) is redrawn.
func (xx *Hnsw) RandomLevel() int {
	u := rand.Float32()
	for u <= 0 {
		u = rand.Float32()
	}
	lv, err := colttgpu.HnswRandomLevel(xx.h, u)
	if err != nil {
		return 0
	}
	return lv
}

// BytesSize — hnsw.go:476-490 (HNSW_VERTEX_EDGE_BYTES = 12, HNSW_VERTEX_MUTEX_BYTES = 24: the HOST-side estimate the
// reference reports; the HBM footprint is Len() * (row stride + 2 * 4 * mMax0) + upper rows)
func (xx *Hnsw) BytesSize() uint64 {
	maxLevel := 10
	if lv, err := colttgpu.HnswEntryLevel(xx.h); err == nil && lv >= 0 { // host-side field of the index: no adjacency is copied
		maxLevel = lv
	}
	const edgeB, mutB = 12.0, 24.0
	ptr := float64(xx.config.mMax0)*edgeB + mutB
	for i := 1; i < maxLevel; i++ {
		ptr += (float64(xx.config.mMax)*edgeB + mutB) * math.Exp(float64(i)/-float64(xx.config.levelMultiplier))
	}
	return uint64(math.Floor(float64(xx.Len())*ptr)) + atomic.LoadUint64(&xx.bytesSize)
}

// Commit(w, header) — hnsw_commit.go:69-162: the reference's big-endian stream, produced by the library from the HBM layout.
func (xx *Hnsw) Commit(w io.Writer, header bool) error {
	// Snapshot against mutations: the reference's Commit walks the live maps without a lock; here the slot list, the metadata
	// blobs and the stream are produced under commitMu so an Insert / Remove cannot interleave (they take it shared).
	xx.commitMu.Lock()
	defer xx.commitMu.Unlock()
	ids, deleted, err := colttgpu.HnswSlots(xx.h)
	if err != nil {
		return err
	}
	blobs := make([][]byte, len(ids))
	for slot, id := range ids {
		if deleted[slot] != 0 {
			continue
		}
		s := xx.shard(id)
		xx.metaMu[s].RLock()
		m := xx.meta[s][id]
		xx.metaMu[s].RUnlock()
		if blobs[slot], err = m.encode(); err != nil {
			return err
		}
	}
	out, err := colttgpu.HnswCommit(xx.h, header, blobs)
	if err != nil {
		return err
	}
	_, err = w.Write(out)
	return err
}

// Compact reclaims the device memory of removed vertices (coltt_hnsw_compact) — NOT in the reference, whose Remove frees its vertex to
// the garbage collector.  An index that is updated in place (Core.Update = Remove + Insert) should call it now and then: answers do not
// change, walks stop testing tombstones, later Inserts fill the freed slots.  It takes commitMu exclusive like Commit: Commit's blob table
// is indexed by slot from HnswSlots, and the call renumbers the slots (the metadata here is keyed by id and stays as it is).  The open
// filters and attribute columns made through this object (NewFilter, EvalFilter*, NewAttrColumn; not yet closed) are carried along
// (coltt_hnsw_compact_carry): they stay valid under their handles, a filter's Allowed is refreshed.  A filter or column this object knows
// to be stale (a Load, a failed call) is left out of the carry and stays stale.  If the library rejects a handle all the same — an object
// made stale behind this object's back (a direct colttgpu.HnswCompact or BulkLoad on the handle), or closed between the snapshot of the
// lists and the call — nothing has changed yet: the index is then compacted without a carry, as before this call existed, and every open
// object is stale and marked so.  A device failure leaves the empty index and likewise marks them.
func (xx *Hnsw) Compact() (colttgpu.HnswCompactStats, error) {
	if xx.err != nil {
		return colttgpu.HnswCompactStats{}, xx.err
	}
	xx.commitMu.Lock()
	defer xx.commitMu.Unlock()
	xx.carryMu.Lock()
	fs := make([]*HnswFilter, 0, len(xx.filters))
	fh := make([]colttgpu.Handle, 0, len(xx.filters))
	for f := range xx.filters {
		if f.h != 0 && !f.stale {
			fs = append(fs, f)
			fh = append(fh, f.h)
		}
	}
	ch := make([]colttgpu.Handle, 0, len(xx.columns))
	for c := range xx.columns {
		if c.h != 0 && !c.stale {
			ch = append(ch, c.h)
		}
	}
	xx.carryMu.Unlock()
	st, _, allowed, _, code, err := colttgpu.HnswCompactCarry(xx.h, 0, fh, ch)
	switch code {
	case colttgpu.CodeOK:
		for i, f := range fs {
			f.Allowed = allowed[i]
		}
	case colttgpu.CodeUnsupported, colttgpu.CodeNoMem: // refused, the index and the objects are as they were
	case colttgpu.CodeNotFound, colttgpu.CodeInvalid: // a handle was rejected before anything changed: compact without a carry
		st, err = colttgpu.HnswCompact(xx.h, 0)
		if err != nil || st.SlotsAfter != st.SlotsBefore {
			xx.markStale()
		}
	default: // a device failure: the empty index
		xx.markStale()
	}
	return st, mapErr(err)
}

// markStale: the slots were renumbered without the open objects (or the index was emptied): Compact lists none of them again.
func (xx *Hnsw) markStale() {
	xx.carryMu.Lock()
	for f := range xx.filters {
		f.stale = true
	}
	for c := range xx.columns {
		c.stale = true
	}
	xx.carryMu.Unlock()
}

// Load(r, header) — hnsw_commit.go:164-278: the stream goes straight into HBM; metadata blobs are decoded here.
func (xx *Hnsw) Load(r io.Reader, header bool) error {
	data, err := io.ReadAll(r)
	if err != nil {
		return err
	}
	ids, off, ln, err := colttgpu.HnswLoad(xx.h, header, data, uint32(xx.dim))
	xx.markStale() // the slots were renumbered (or the index emptied by a failed install): what was open is stale for good
	if err != nil {
		return err
	}
	fresh := [metaShards]map[uint64]Metadata{}
	for i := range fresh {
		fresh[i] = make(map[uint64]Metadata)
	}
	var size uint64
	for i, id := range ids {
		m, err := decodeMetadata(data[off[i] : off[i]+uint64(ln[i])])
		if err != nil {
			return err
		}
		fresh[xx.shard(id)][id] = m
		size += uint64(xx.dim)*4 + metaBytes(m)
	}
	for i := range fresh {
		xx.metaMu[i].Lock()
		xx.meta[i] = fresh[i]
		xx.metaMu[i].Unlock()
	}
	atomic.StoreUint64(&xx.bytesSize, size)
	xx.refreshConfig()
	return nil
}
