// Package colttgpu — the cgo layer under the two drop-in packages of this directory tree:
//
//	go/vectorindex  replacement body for github.com/sjy-dv/coltt/core/vectorindex   (*Hnsw and friends)
//	go/edge         one extra file for package github.com/sjy-dv/coltt/edge          (gpuVecSpace, an edge.vectorspace)
//
// NOT COMPILED in the build container (no Go toolchain there); shipped as source for the maintainer (INTEGRATION.md).
// Rules kept here once so the callers cannot get them wrong:
//   - no Go pointer is retained by C: every call copies in / out before it returns;
//   - coltt_last_error() is thread-local and a goroutine may migrate between OS threads across cgo calls, so every
//     call + error fetch runs under runtime.LockOSThread (Call);
//   - slices handed to C are validated against `dim` first — C never reads past a short Go slice.
package colttgpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../coltt_amd -lcoltt_gpu -Wl,-rpath,${SRCDIR}/../../coltt_amd
#include <stdlib.h>
#include "coltt_gpu.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"math"
	"runtime"
	"unsafe"
)

var (
	ErrNotFound = errors.New("Item not found")      // core/vectorindex/hnsw.go:39 ItemNotFoundError
	ErrExists   = errors.New("Item already exists") // core/vectorindex/hnsw.go:40 ItemAlreadyExistsError
)

type Handle = C.coltt_handle_t

// HnswCfg mirrors coltt_hnsw_cfg (hnswConfig, core/vectorindex/hnsw_config.go:135-162).
type HnswCfg struct {
	M, MMax, MMax0, Ef, EfConstruction, Algo int32
	LevelMultiplier                          float32
	ExtendCandidates, KeepPruned             int32
}

func (c *HnswCfg) c() C.coltt_hnsw_cfg {
	return C.coltt_hnsw_cfg{m: C.int32_t(c.M), m_max: C.int32_t(c.MMax), m_max0: C.int32_t(c.MMax0), ef: C.int32_t(c.Ef),
		ef_construction: C.int32_t(c.EfConstruction), algo: C.int32_t(c.Algo), level_multiplier: C.float(c.LevelMultiplier),
		extend_candidates: C.int32_t(c.ExtendCandidates), keep_pruned: C.int32_t(c.KeepPruned)}
}

// call runs one C entry point and turns its status into a Go error on the SAME OS thread that made the call.
func call(f func() C.int) error {
	runtime.LockOSThread()
	defer runtime.UnlockOSThread()
	rc := f()
	switch rc {
	case C.COLTT_OK:
		return nil
	case C.COLTT_E_NOT_FOUND:
		return ErrNotFound
	case C.COLTT_E_EXISTS:
		return ErrExists
	}
	return errors.New(C.GoString(C.coltt_last_error()))
}

func checkDim(v []float32, dim uint32, n int) error {
	if n == 0 || uint64(len(v)) != uint64(dim)*uint64(n) {
		// edge/none_vectorstore.go:86-88
		return fmt.Errorf("Dim Length UnmatchdError: expect dimension: [%d], but got [%d]", dim, len(v)/max1(n))
	}
	return nil
}
func max1(n int) int {
	if n < 1 {
		return 1
	}
	return n
}
func fptr(v []float32) *C.float {
	if len(v) == 0 {
		return nil
	}
	return (*C.float)(unsafe.Pointer(&v[0]))
}
func uptr(v []uint64) *C.uint64_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint64_t)(unsafe.Pointer(&v[0]))
}
func bptr(v []byte) *C.uint8_t {
	if len(v) == 0 {
		return nil
	}
	return (*C.uint8_t)(unsafe.Pointer(&v[0]))
}

func Init(device int) error { return call(func() C.int { return C.coltt_init(C.int(device)) }) }

// Normalize — edge.Normalize / vectorindex.Normalize (edge/vectorstore.go:173-189; core/vectorindex/metadata.go:107-123) through
// coltt_normalize_host: the library's HOST copy of the arithmetic (sequential f32 sum, float64 sqrt, per-element divide).  It touches no
// device, stream or allocator, so a call per RPC cannot stall concurrent searches, needs no initialised GPU and — like the reference's
// function — cannot fail; a zero vector comes back as zeros.  Batches (tests, bulk ingest) use NormalizeBatch.
func Normalize(v []float32) []float32 {
	out := make([]float32, len(v))
	if len(v) != 0 {
		C.coltt_normalize_host(fptr(v), C.uint32_t(len(v)), fptr(out))
	}
	return out
}

// NormalizeBatch — n row-major vectors on the device (coltt_normalize); for bulk paths only.
func NormalizeBatch(v []float32, dim uint32) ([]float32, error) {
	out := make([]float32, len(v))
	if len(v) == 0 || dim == 0 {
		return out, nil
	}
	err := call(func() C.int { return C.coltt_normalize(fptr(v), C.size_t(len(v)/int(dim)), C.uint32_t(dim), fptr(out)) })
	return out, err
}

// ------------------------------------------------------------------------------------------------ HNSW
func HnswCreate(dim uint32, metric, quant int, cfg *HnswCfg) (Handle, error) {
	var h Handle
	cc := cfg.c()
	err := call(func() C.int { return C.coltt_hnsw_create(C.uint32_t(dim), C.int(metric), C.int(quant), &cc, &h) })
	return h, err
}
func HnswDestroy(h Handle) { C.coltt_hnsw_destroy(h) }
func HnswGetCfg(h Handle) (HnswCfg, error) {
	var c C.coltt_hnsw_cfg
	err := call(func() C.int { return C.coltt_hnsw_get_cfg(h, &c) })
	return HnswCfg{int32(c.m), int32(c.m_max), int32(c.m_max0), int32(c.ef), int32(c.ef_construction), int32(c.algo),
		float32(c.level_multiplier), int32(c.extend_candidates), int32(c.keep_pruned)}, err
}
func HnswInsert(h Handle, dim uint32, id uint64, v []float32, level int) error {
	if err := checkDim(v, dim, 1); err != nil {
		return err
	}
	return call(func() C.int { return C.coltt_hnsw_insert(h, C.uint64_t(id), fptr(v), C.int32_t(level)) })
}
// HnswReserve sizes every device array of the index for nSlots vertices in one allocation (coltt_hnsw_reserve): optional, but a
// collection whose size is known (a Load, a bulk import) should call it before the inserts — growth re-copies the arrays.
func HnswReserve(h Handle, nSlots uint64) error {
	return call(func() C.int { return C.coltt_hnsw_reserve(h, C.uint64_t(nSlots), 0) })
}

func HnswRemove(h Handle, id uint64) error {
	return call(func() C.int { return C.coltt_hnsw_remove(h, C.uint64_t(id)) })
}

// HnswCompactStats mirrors coltt_hnsw_compact_stats.
type HnswCompactStats struct {
	SlotsBefore, SlotsAfter         uint64
	UpperRowsBefore, UpperRowsAfter uint64
	EdgesDropped                    uint64 // adjacency entries that named a tombstoned slot, all levels
	RowsMoved                       uint64 // live slots whose number changed
	BytesMoved                      uint64 // bytes the move kernels wrote, staging included
	Ms                              float32
}

// HnswCompact reclaims the slots of removed vertices on the device (coltt_hnsw_compact — an extension the reference does not have): the
// live vertices keep their order and move down, no search answer changes, filters built before the call are stale.  stageBytes: the
// staging block (0 = 64 MiB).  The slots are renumbered: slot-indexed tables of the caller come from a fresh export afterwards.
func HnswCompact(h Handle, stageBytes uint64) (HnswCompactStats, error) {
	var st C.coltt_hnsw_compact_stats
	err := call(func() C.int { return C.coltt_hnsw_compact(h, C.uint64_t(stageBytes), nil, 0, &st) })
	return HnswCompactStats{uint64(st.slots_before), uint64(st.slots_after), uint64(st.upper_rows_before), uint64(st.upper_rows_after),
		uint64(st.edges_dropped), uint64(st.rows_moved), uint64(st.bytes_moved), float32(st.ms)}, err
}

// HnswCarryStats mirrors coltt_hnsw_carry_stats.
type HnswCarryStats struct {
	Filters, Columns uint64 // distinct objects carried
	BitmapWords      uint64 // written for them
	ListEntries      uint64
	ColumnValues     uint64
	Ms               float32 // device time of the carry launches alone
}

// HnswCompactCarry is HnswCompact after which the listed filters and attribute columns are valid at the new generation under the same
// handles (coltt_hnsw_compact_carry): a filter allows what it allowed among the live vertices, a column holds at every live vertex what it
// held.  Objects that are not listed go stale.  allowed[i] / set[i]: the allowed count of filters[i] / the set count of columns[i] after
// the call.  A handle may repeat.  A bad handle fails the call before anything changes.  code is the library's status (Code* below), so
// that a caller can tell a rejected handle (CodeNotFound, CodeInvalid: nothing changed) from a refusal that left the index as it was
// (CodeUnsupported, CodeNoMem) and from a device failure (anything else: the index is empty and every object stale).
func HnswCompactCarry(h Handle, stageBytes uint64, filters, columns []Handle) (st HnswCompactStats, carry HnswCarryStats, allowed, set []uint64, code int, err error) {
	var cst C.coltt_hnsw_compact_stats
	var ccs C.coltt_hnsw_carry_stats
	allowed = make([]uint64, len(filters))
	set = make([]uint64, len(columns))
	var fp, cp *Handle
	var ap, sp *C.uint64_t
	if len(filters) > 0 {
		fp = &filters[0]
		ap = (*C.uint64_t)(unsafe.Pointer(&allowed[0]))
	}
	if len(columns) > 0 {
		cp = &columns[0]
		sp = (*C.uint64_t)(unsafe.Pointer(&set[0]))
	}
	err = call(func() C.int {
		rc := C.coltt_hnsw_compact_carry(h, C.uint64_t(stageBytes), fp, C.size_t(len(filters)), ap, cp, C.size_t(len(columns)), sp, nil, 0, &cst, &ccs)
		code = int(rc)
		return rc
	})
	st = HnswCompactStats{uint64(cst.slots_before), uint64(cst.slots_after), uint64(cst.upper_rows_before), uint64(cst.upper_rows_after),
		uint64(cst.edges_dropped), uint64(cst.rows_moved), uint64(cst.bytes_moved), float32(cst.ms)}
	carry = HnswCarryStats{uint64(ccs.filters), uint64(ccs.columns), uint64(ccs.bitmap_words), uint64(ccs.list_entries), uint64(ccs.column_values), float32(ccs.ms)}
	return st, carry, allowed, set, code, err
}

// The library's status codes a caller of HnswCompactCarry tells apart.
const (
	CodeOK          = int(C.COLTT_OK)
	CodeInvalid     = int(C.COLTT_E_INVALID)
	CodeNotFound    = int(C.COLTT_E_NOT_FOUND)
	CodeUnsupported = int(C.COLTT_E_UNSUPPORTED)
	CodeNoMem       = int(C.COLTT_E_NOMEM)
)
func HnswLen(h Handle) int {
	var n C.uint64_t
	C.coltt_hnsw_len(h, &n)
	return int(n)
}

// HnswSearch: nq queries (row-major), k results each; returns ids, scores [nq*k] and counts [nq].
func HnswSearch(h Handle, dim uint32, queries []float32, nq int, k uint32, ef uint32) ([]uint64, []float32, []uint32, error) {
	if nq == 0 || k == 0 {
		return nil, nil, make([]uint32, nq), nil
	}
	if err := checkDim(queries, dim, nq); err != nil {
		return nil, nil, nil, err
	}
	ids := make([]uint64, nq*int(k))
	sc := make([]float32, nq*int(k))
	cnt := make([]uint32, nq)
	err := call(func() C.int {
		return C.coltt_hnsw_search(h, fptr(queries), C.size_t(nq), C.uint32_t(k), C.uint32_t(ef), uptr(ids), fptr(sc),
			(*C.uint32_t)(unsafe.Pointer(&cnt[0])), nil)
	})
	return ids, sc, cnt, err
}
// HnswFilterCreate: an allow-list of ids against index h (coltt_hnsw_filter_create — an extension the reference does not have);
// returns the filter's handle and how many live vertices it allows.  Release it with HnswFilterDestroy.
func HnswFilterCreate(h Handle, ids []uint64) (Handle, uint64, error) {
	var f Handle
	var allowed C.uint64_t
	err := call(func() C.int {
		var p *C.uint64_t
		if len(ids) > 0 {
			p = (*C.uint64_t)(unsafe.Pointer(&ids[0]))
		}
		return C.coltt_hnsw_filter_create(h, p, C.size_t(len(ids)), &allowed, &f)
	})
	return f, uint64(allowed), err
}
func HnswFilterDestroy(f Handle) error {
	return call(func() C.int { return C.coltt_hnsw_filter_destroy(f) })
}

// Operators of a filter programme (coltt_gpu.h: COLTT_FOP_*).  A programme is postfix: a value >= 0 pushes leaves[value].
const (
	FopAnd    int32 = -1 // a b -> a & b
	FopOr     int32 = -2 // a b -> a | b
	FopAndNot int32 = -3 // a b -> a & ~b
	FopNot    int32 = -4 // a   -> live & ~a
	FopAll    int32 = -5 //     -> live
)

func hptr(h []Handle) *Handle {
	if len(h) == 0 {
		return nil
	}
	return &h[0]
}

// HnswFilterEval: the filter of a postfix programme over resident filters, evaluated on the device (coltt_hnsw_filter_eval).  The result
// is an ordinary filter: the same as HnswFilterCreate over the ids of { live slots : expr }.  Release it with HnswFilterDestroy.
func HnswFilterEval(h Handle, prog []int32, leaves []Handle) (Handle, uint64, error) {
	var f Handle
	var allowed C.uint64_t
	err := call(func() C.int {
		var p *C.int32_t
		if len(prog) > 0 {
			p = (*C.int32_t)(unsafe.Pointer(&prog[0]))
		}
		return C.coltt_hnsw_filter_eval(h, p, C.size_t(len(prog)), hptr(leaves), C.size_t(len(leaves)), &allowed, &f)
	})
	return f, uint64(allowed), err
}

// HnswFilterEvalBatch: one filter per programme over a shared leaf table, under one index state, in two kernel launches whatever
// len(progs) is (coltt_hnsw_filter_eval_batch).  Nothing is created if any programme or handle is bad; the error names the first.
func HnswFilterEvalBatch(h Handle, progs [][]int32, leaves []Handle) ([]Handle, []uint64, error) {
	n := len(progs)
	if n == 0 {
		return nil, nil, nil
	}
	off := make([]uint64, n+1)
	var flat []int32
	for i, p := range progs {
		flat = append(flat, p...)
		off[i+1] = uint64(len(flat))
	}
	out := make([]Handle, n)
	allowed := make([]uint64, n)
	err := call(func() C.int {
		var p *C.int32_t
		if len(flat) > 0 {
			p = (*C.int32_t)(unsafe.Pointer(&flat[0]))
		}
		return C.coltt_hnsw_filter_eval_batch(h, p, (*C.uint64_t)(unsafe.Pointer(&off[0])), C.size_t(n), hptr(leaves), C.size_t(len(leaves)),
			(*C.uint64_t)(unsafe.Pointer(&allowed[0])), &out[0])
	})
	if err != nil {
		return nil, nil, err
	}
	return out, allowed, nil
}

// Attribute columns and predicates (coltt_gpu.h, "Attribute columns and predicates"): a numeric field as one 8-byte value per slot beside
// the index, comparisons over it as leaves of a filter programme.
const (
	AttrI64 = 0 // COLTT_ATTR_I64: int64 values
	AttrF64 = 1 // COLTT_ATTR_F64: float64 values
)

// Comparison operators (COLTT_CMP_*), in the order of the reference's FilterOp (pkg/inverted/filter.go:24-31).
const (
	CmpEq  int32 = 0
	CmpNe  int32 = 1
	CmpGt  int32 = 2
	CmpGe  int32 = 3
	CmpLt  int32 = 4
	CmpLe  int32 = 5
	CmpSet int32 = 6 // the slot has a value; the operand is ignored
)

// AttrPred mirrors coltt_attr_pred; Bits holds the operand's 8 bytes in the column's type (AttrPredI64 / AttrPredF64 fill it).
type AttrPred struct {
	Column Handle
	Op     int32
	Bits   uint64
}

func AttrPredI64(column Handle, op int32, operand int64) AttrPred {
	return AttrPred{Column: column, Op: op, Bits: uint64(operand)}
}
func AttrPredF64(column Handle, op int32, operand float64) AttrPred {
	return AttrPred{Column: column, Op: op, Bits: math.Float64bits(operand)}
}

func cpreds(preds []AttrPred) []C.coltt_attr_pred {
	out := make([]C.coltt_attr_pred, len(preds))
	for i, p := range preds {
		out[i].column = p.Column
		out[i].op = C.int32_t(p.Op)
		out[i].reserved = 0
		*(*uint64)(unsafe.Pointer(&out[i].value)) = p.Bits // the union: 8 bytes either way
	}
	return out
}

// HnswAttrCreate: an empty column of type AttrI64 / AttrF64 beside index h (coltt_hnsw_attr_create).  Release it with HnswAttrDestroy.
func HnswAttrCreate(h Handle, typ int) (Handle, error) {
	var c Handle
	err := call(func() C.int { return C.coltt_hnsw_attr_create(h, C.int(typ), &c) })
	return c, err
}
func HnswAttrDestroy(c Handle) error {
	return call(func() C.int { return C.coltt_hnsw_attr_destroy(c) })
}

// HnswAttrSetI64 / HnswAttrSetF64: ids -> values (coltt_hnsw_attr_set).  Unknown and removed ids are ignored, an id repeated takes its last
// value, a NaN refuses the whole call.  Returns the vertices set.
func HnswAttrSetI64(c Handle, ids []uint64, values []int64) (uint64, error) {
	if len(ids) != len(values) {
		return 0, fmt.Errorf("HnswAttrSetI64: %d ids, %d values", len(ids), len(values))
	}
	if len(ids) == 0 {
		return 0, nil
	}
	return attrSet(c, ids, unsafe.Pointer(&values[0]))
}
func HnswAttrSetF64(c Handle, ids []uint64, values []float64) (uint64, error) {
	if len(ids) != len(values) {
		return 0, fmt.Errorf("HnswAttrSetF64: %d ids, %d values", len(ids), len(values))
	}
	if len(ids) == 0 {
		return 0, nil
	}
	return attrSet(c, ids, unsafe.Pointer(&values[0]))
}
func attrSet(c Handle, ids []uint64, values unsafe.Pointer) (uint64, error) {
	var applied C.uint64_t
	err := call(func() C.int { return C.coltt_hnsw_attr_set(c, uptr(ids), values, C.size_t(len(ids)), &applied) })
	return uint64(applied), err
}

// HnswAttrGet: the raw 8-byte values of ids and whether each vertex holds one (coltt_hnsw_attr_get); math.Float64frombits for an F64 column.
func HnswAttrGet(c Handle, ids []uint64) ([]uint64, []bool, error) {
	if len(ids) == 0 {
		return nil, nil, nil
	}
	vals := make([]uint64, len(ids))
	flags := make([]uint8, len(ids))
	err := call(func() C.int {
		return C.coltt_hnsw_attr_get(c, uptr(ids), C.size_t(len(ids)), unsafe.Pointer(&vals[0]), (*C.uint8_t)(unsafe.Pointer(&flags[0])))
	})
	if err != nil {
		return nil, nil, err
	}
	set := make([]bool, len(ids))
	for i, f := range flags {
		set[i] = f != 0
	}
	return vals, set, nil
}

// HnswAttrInfo: the column's index, type, the slots it covers and the slots that hold a value (coltt_hnsw_attr_info).
func HnswAttrInfo(c Handle) (index Handle, typ int, slots, set uint64, err error) {
	var t C.int32_t
	var s, n C.uint64_t
	err = call(func() C.int { return C.coltt_hnsw_attr_info(c, &index, &t, &s, &n) })
	return index, int(t), uint64(s), uint64(n), err
}

// HnswFilterEvalAttr: HnswFilterEval over leaves and predicates (coltt_hnsw_filter_eval_attr): a value v >= 0 of the programme pushes
// leaves[v] when v < len(leaves) and preds[v - len(leaves)] otherwise.
func HnswFilterEvalAttr(h Handle, prog []int32, leaves []Handle, preds []AttrPred) (Handle, uint64, error) {
	var f Handle
	var allowed C.uint64_t
	cp := cpreds(preds)
	err := call(func() C.int {
		var p *C.int32_t
		if len(prog) > 0 {
			p = (*C.int32_t)(unsafe.Pointer(&prog[0]))
		}
		var pp *C.coltt_attr_pred
		if len(cp) > 0 {
			pp = &cp[0]
		}
		return C.coltt_hnsw_filter_eval_attr(h, p, C.size_t(len(prog)), hptr(leaves), C.size_t(len(leaves)), pp, C.size_t(len(cp)), &allowed, &f)
	})
	return f, uint64(allowed), err
}

// HnswFilterEvalAttrBatch: one filter per programme over shared leaf and predicate tables (coltt_hnsw_filter_eval_attr_batch).
func HnswFilterEvalAttrBatch(h Handle, progs [][]int32, leaves []Handle, preds []AttrPred) ([]Handle, []uint64, error) {
	n := len(progs)
	if n == 0 {
		return nil, nil, nil
	}
	off := make([]uint64, n+1)
	var flat []int32
	for i, p := range progs {
		flat = append(flat, p...)
		off[i+1] = uint64(len(flat))
	}
	out := make([]Handle, n)
	allowed := make([]uint64, n)
	cp := cpreds(preds)
	err := call(func() C.int {
		var p *C.int32_t
		if len(flat) > 0 {
			p = (*C.int32_t)(unsafe.Pointer(&flat[0]))
		}
		var pp *C.coltt_attr_pred
		if len(cp) > 0 {
			pp = &cp[0]
		}
		return C.coltt_hnsw_filter_eval_attr_batch(h, p, (*C.uint64_t)(unsafe.Pointer(&off[0])), C.size_t(n), hptr(leaves), C.size_t(len(leaves)),
			pp, C.size_t(len(cp)), (*C.uint64_t)(unsafe.Pointer(&allowed[0])), &out[0])
	})
	if err != nil {
		return nil, nil, err
	}
	return out, allowed, nil
}

// AttrCmpHost: the comparison itself with no device (coltt_attr_cmp_host): isSet && value OP operand, both as the column type's 8 bytes.
func AttrCmpHost(typ int, op int32, operand, value uint64, isSet bool) (bool, error) {
	s := C.int(0)
	if isSet {
		s = 1
	}
	var rc C.int
	err := call(func() C.int {
		rc = C.coltt_attr_cmp_host(C.int(typ), C.int(op), unsafe.Pointer(&operand), unsafe.Pointer(&value), s)
		if rc > 0 {
			return C.COLTT_OK
		}
		return rc
	})
	return rc == 1, err
}

// HnswFilterIds: the ids filter f allows, in ascending slot order, at most limit of them (coltt_hnsw_filter_ids; gathered on the device).
// The second result is the filter's allowed count.
func HnswFilterIds(f Handle, limit uint64) ([]uint64, uint64, error) {
	var n C.uint64_t
	ids := make([]uint64, limit)
	err := call(func() C.int { return C.coltt_hnsw_filter_ids(f, uptr(ids), C.uint64_t(limit), &n) })
	if err != nil {
		return nil, 0, err
	}
	if uint64(n) < limit {
		ids = ids[:n]
	}
	return ids, uint64(n), nil
}

// HnswFilterInfo: the index a filter was built for, its allowed count and the slots it covers (coltt_hnsw_filter_info).
func HnswFilterInfo(f Handle) (index Handle, allowed, slots uint64, err error) {
	var a, s C.uint64_t
	err = call(func() C.int { return C.coltt_hnsw_filter_info(f, &index, &a, &s) })
	return index, uint64(a), uint64(s), err
}

// FilterProgCheck: the programme rules with no device (coltt_hnsw_filter_prog_check_host); returns the deepest stack.
func FilterProgCheck(prog []int32, nLeaves int) (uint32, error) {
	var d C.uint32_t
	err := call(func() C.int {
		var p *C.int32_t
		if len(prog) > 0 {
			p = (*C.int32_t)(unsafe.Pointer(&prog[0]))
		}
		return C.coltt_hnsw_filter_prog_check_host(p, C.size_t(len(prog)), C.size_t(nLeaves), &d)
	})
	return uint32(d), err
}

// Filter modes of HnswSearchFiltered (coltt_gpu.h: COLTT_FILTER_*)
const (
	FilterAuto  = 0
	FilterWalk  = 1
	FilterExact = 2
)

// HnswSearchFiltered: as HnswSearch, among the vertices filter f allows.
func HnswSearchFiltered(h, f Handle, dim uint32, queries []float32, nq int, k uint32, ef uint32, mode int) ([]uint64, []float32, []uint32, error) {
	if nq == 0 || k == 0 {
		return nil, nil, make([]uint32, nq), nil
	}
	if err := checkDim(queries, dim, nq); err != nil {
		return nil, nil, nil, err
	}
	ids := make([]uint64, nq*int(k))
	sc := make([]float32, nq*int(k))
	cnt := make([]uint32, nq)
	err := call(func() C.int {
		return C.coltt_hnsw_search_filtered(h, f, fptr(queries), C.size_t(nq), C.uint32_t(k), C.uint32_t(ef), C.int(mode), uptr(ids), fptr(sc),
			(*C.uint32_t)(unsafe.Pointer(&cnt[0])), nil)
	})
	return ids, sc, cnt, err
}

// HnswSearchFilteredBatch: a filter per query (coltt_hnsw_search_filtered_batch).  Row i equals HnswSearchFiltered(h, filters[i], query i,
// 1, k, ef, mode); paths[i] is the path that call takes (FilterWalk / FilterExact).  Every handle is checked before anything runs: one bad
// filter fails the whole call, and the error names its position.
func HnswSearchFilteredBatch(h Handle, filters []Handle, dim uint32, queries []float32, nq int, k uint32, ef uint32, mode int) ([]uint64, []float32, []uint32, []int32, error) {
	if nq == 0 || k == 0 {
		return nil, nil, make([]uint32, nq), make([]int32, nq), nil
	}
	if len(filters) != nq {
		return nil, nil, nil, nil, fmt.Errorf("HnswSearchFilteredBatch: %d filters for %d queries", len(filters), nq)
	}
	if err := checkDim(queries, dim, nq); err != nil {
		return nil, nil, nil, nil, err
	}
	ids := make([]uint64, nq*int(k))
	sc := make([]float32, nq*int(k))
	cnt := make([]uint32, nq)
	paths := make([]int32, nq)
	err := call(func() C.int {
		return C.coltt_hnsw_search_filtered_batch(h, &filters[0], fptr(queries), C.size_t(nq), C.uint32_t(k),
			C.uint32_t(ef), C.int(mode), uptr(ids), fptr(sc), (*C.uint32_t)(unsafe.Pointer(&cnt[0])), (*C.int32_t)(unsafe.Pointer(&paths[0])), nil)
	})
	return ids, sc, cnt, paths, err
}

func HnswRandomLevel(h Handle, u float32) (int, error) {
	var lv C.int32_t
	err := call(func() C.int { return C.coltt_hnsw_random_level(h, C.float(u), &lv) })
	return int(lv), err
}

// HnswGet: stored (normalised) f32 vector and level of a live vertex (hnsw.go:169-189).
func HnswGet(h Handle, dim uint32, id uint64) ([]float32, int, error) {
	v := make([]float32, dim)
	var lv C.int32_t
	err := call(func() C.int { return C.coltt_hnsw_get(h, C.uint64_t(id), unsafe.Pointer(&v[0]), &lv) })
	return v, int(lv), err
}

// HnswEntryLevel: level of the entrypoint (-1 = empty index); host-side only, no device traffic (what BytesSize needs).
func HnswEntryLevel(h Handle) (int, error) {
	var lv C.int32_t
	err := call(func() C.int { return C.coltt_hnsw_entry_level(h, &lv) })
	return int(lv), err
}

// HnswSlots: ids of every slot in slot order and the deleted flags (what Commit walks).
// The size query and the fill are two cgo calls; an Insert may land between them.  The library treats the counts passed to
// the second call as the CAPACITIES of the slices and refuses (COLTT_E_INVALID, needed sizes returned) instead of writing past
// them, so the loop simply re-sizes and retries.
func HnswSlots(h Handle) (ids []uint64, deleted []byte, err error) {
	for attempt := 0; attempt < 8; attempt++ {
		var ns, nr, ne C.uint64_t
		var ent C.int32_t
		if err = call(func() C.int { return C.coltt_hnsw_export(h, &ns, &nr, &ne, nil, nil, nil, nil, nil, nil, &ent) }); err != nil {
			return
		}
		if ns == 0 {
			return nil, nil, nil
		}
		capSlots := ns
		ids = make([]uint64, int(capSlots))
		deleted = make([]byte, int(capSlots))
		rc := C.int(0)
		err = call(func() C.int {
			rc = C.coltt_hnsw_export(h, &ns, &nr, &ne, uptr(ids), nil, bptr(deleted), nil, nil, nil, &ent)
			return rc
		})
		if err == nil {
			return ids[:int(ns)], deleted[:int(ns)], nil // ns <= capSlots: Remove never shrinks the slot count
		}
		if rc != C.COLTT_E_INVALID || ns <= capSlots {
			return nil, nil, err
		}
	}
	return nil, nil, errors.New("hnsw export: the index kept growing during 8 attempts")
}

// HnswCommit: Hnsw.Commit stream (hnsw_commit.go:69-162); metaBlobs[slot] = that vertex's Metadata in stream encoding
// (metadata.go:31-74), nil = empty map.
func HnswCommit(h Handle, header bool, metaBlobs [][]byte) ([]byte, error) {
	n := len(metaBlobs)
	// C arrays of blob pointers live in C memory for the duration of the call (no Go pointer to Go pointer crosses cgo)
	var cptr **C.uint8_t
	var clen *C.uint32_t
	var pins []unsafe.Pointer
	if n > 0 {
		cptr = (**C.uint8_t)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))
		clen = (*C.uint32_t)(C.malloc(C.size_t(n) * 4))
		defer C.free(unsafe.Pointer(cptr))
		defer C.free(unsafe.Pointer(clen))
		ps := unsafe.Slice(cptr, n)
		ls := unsafe.Slice(clen, n)
		for i, b := range metaBlobs {
			if len(b) == 0 {
				ps[i], ls[i] = nil, 0
				continue
			}
			p := C.CBytes(b)
			pins = append(pins, p)
			ps[i], ls[i] = (*C.uint8_t)(p), C.uint32_t(len(b))
		}
		defer func() {
			for _, p := range pins {
				C.free(p)
			}
		}()
	}
	hd := C.int(0)
	if header {
		hd = 1
	}
	var need C.uint64_t
	if err := call(func() C.int { return C.coltt_hnsw_commit(h, hd, cptr, clen, C.uint64_t(n), nil, 0, &need) }); err != nil {
		return nil, err
	}
	// slots past n (vertices inserted since the caller built metaBlobs) are written with empty metadata by the library; a
	// stream that outgrew the buffer between the two calls comes back as "buffer too small" and is retried with the new size
	for attempt := 0; attempt < 8; attempt++ {
		capB := need
		out := make([]byte, int(capB))
		err := call(func() C.int { return C.coltt_hnsw_commit(h, hd, cptr, clen, C.uint64_t(n), bptr(out), capB, &need) })
		if err == nil {
			return out[:int(need)], nil
		}
		if need <= capB {
			return nil, err
		}
	}
	return nil, errors.New("hnsw commit: the index kept growing during 8 attempts")
}

// HnswLoad: Hnsw.Load (hnsw_commit.go:164-278) straight into HBM; returns each vertex's id and the position of its
// metadata blob inside data (the caller decodes the msgpack values).
func HnswLoad(h Handle, header bool, data []byte, dim uint32) (ids []uint64, metaOff []uint64, metaLen []uint32, err error) {
	capN := uint64(len(data))/uint64(14+4*dim) + 1 // a vertex record is at least 8 + 4 + 4*dim + 2 bytes
	ids = make([]uint64, capN)
	metaOff = make([]uint64, capN)
	metaLen = make([]uint32, capN)
	hd := C.int(0)
	if header {
		hd = 1
	}
	var n C.uint64_t
	err = call(func() C.int {
		return C.coltt_hnsw_load(h, hd, bptr(data), C.uint64_t(len(data)), &n, uptr(ids), uptr(metaOff),
			(*C.uint32_t)(unsafe.Pointer(&metaLen[0])), C.uint64_t(capN))
	})
	if err != nil {
		return nil, nil, nil, err
	}
	return ids[:n], metaOff[:n], metaLen[:n], nil
}

// ------------------------------------------------------------------------------------------------ FLAT
const (
	SelectReference = int(C.COLTT_SELECT_REFERENCE) // what edge.PriorityQueue does: keeps the K LARGEST distances (priority_queue.go:39-55)
	SelectNearest   = int(C.COLTT_SELECT_NEAREST)
	ModeExact       = int(C.COLTT_MODE_EXACT)
	ModeMFMA        = int(C.COLTT_MODE_MFMA)
)

func FlatCreate(dim uint32, metric, quant int) (Handle, error) {
	var h Handle
	err := call(func() C.int { return C.coltt_flat_create(C.uint32_t(dim), C.int(metric), C.int(quant), &h) })
	return h, err
}
func FlatDestroy(h Handle) { C.coltt_flat_destroy(h) }
func FlatLen(h Handle) int64 {
	var n C.uint64_t
	C.coltt_flat_len(h, &n)
	return int64(n)
}
func FlatUpsert(h Handle, dim uint32, ids []uint64, vecs []float32) error {
	if len(ids) == 0 {
		return nil
	}
	if err := checkDim(vecs, dim, len(ids)); err != nil {
		return err
	}
	return call(func() C.int { return C.coltt_flat_upsert(h, uptr(ids), fptr(vecs), C.size_t(len(ids))) })
}
func FlatRemove(h Handle, ids []uint64) error {
	if len(ids) == 0 {
		return nil
	}
	return call(func() C.int { return C.coltt_flat_remove(h, uptr(ids), C.size_t(len(ids))) })
}

// FlatSearch: cand == nil -> VertexSearch over the whole store; otherwise FilterableVertexSearch over the candidate ids.
func FlatSearch(h Handle, dim uint32, queries []float32, nq int, k uint32, sel, mode int, cand []uint64, filtered bool) ([]uint64, []float32, []uint32, error) {
	if nq == 0 || k == 0 {
		return nil, nil, make([]uint32, nq), nil
	}
	if err := checkDim(queries, dim, nq); err != nil {
		return nil, nil, nil, err
	}
	ids := make([]uint64, nq*int(k))
	sc := make([]float32, nq*int(k))
	cnt := make([]uint32, nq)
	cp := (*C.uint32_t)(unsafe.Pointer(&cnt[0]))
	var err error
	if !filtered {
		err = call(func() C.int {
			return C.coltt_flat_search(h, fptr(queries), C.size_t(nq), C.uint32_t(k), C.int(sel), C.int(mode), uptr(ids), fptr(sc), cp)
		})
	} else {
		err = call(func() C.int {
			// mode: ModeExact = the exact-order gather scan (one query per RPC); ModeMfma = candidates from the gathered rows on the matrix cores
			return C.coltt_flat_search_ids_mode(h, fptr(queries), C.size_t(nq), C.uint32_t(k), C.int(sel), C.int(mode), uptr(cand), C.size_t(len(cand)), uptr(ids), fptr(sc), cp)
		})
	}
	return ids, sc, cnt, err
}

// FlatSearchIdsBatch: a batch of FilterableVertexSearch RPCs in one call (coltt_flat_search_ids_batch), every query with its own candidate
// list: query i is searched over lists[listOf[i]] (listOf == nil: over lists[i], len(lists) == nq).  Row i equals FlatSearch(h, dim,
// query i, 1, k, sel, ModeExact, that list, true).  Exact-order arithmetic; the lists are translated to rows once per list.
func FlatSearchIdsBatch(h Handle, dim uint32, queries []float32, nq int, k uint32, sel int, lists [][]uint64, listOf []uint32) ([]uint64, []float32, []uint32, error) {
	if nq == 0 || k == 0 {
		return nil, nil, make([]uint32, nq), nil
	}
	if err := checkDim(queries, dim, nq); err != nil {
		return nil, nil, nil, err
	}
	if listOf != nil && len(listOf) != nq {
		return nil, nil, nil, fmt.Errorf("FlatSearchIdsBatch: %d list indices for %d queries", len(listOf), nq)
	}
	off := make([]uint64, len(lists)+1)
	total := 0
	for l, c := range lists {
		total += len(c)
		off[l+1] = uint64(total)
	}
	cand := make([]uint64, 0, total) // the library copies inputs before returning: no Go pointer is retained
	for _, c := range lists {
		cand = append(cand, c...)
	}
	ids := make([]uint64, nq*int(k))
	sc := make([]float32, nq*int(k))
	cnt := make([]uint32, nq)
	cp := (*C.uint32_t)(unsafe.Pointer(&cnt[0]))
	var lp *C.uint32_t
	if listOf != nil {
		lp = (*C.uint32_t)(unsafe.Pointer(&listOf[0]))
	}
	err := call(func() C.int {
		return C.coltt_flat_search_ids_batch(h, fptr(queries), C.size_t(nq), C.uint32_t(k), C.int(sel), uptr(cand), uptr(off), C.size_t(len(lists)), lp,
			uptr(ids), fptr(sc), cp)
	})
	return ids, sc, cnt, err
}

// FlatIdsBatchStats: FlatSearchIdsBatch calls served by the one-pass path and by the k > 64 path, and the (query, row) pairs the one-pass
// path scored (coltt_flat_ids_batch_stats).
func FlatIdsBatchStats(h Handle) (onePass, fallback, pairs uint64, err error) {
	var a, b, p C.uint64_t
	err = call(func() C.int { return C.coltt_flat_ids_batch_stats(h, &a, &b, &p) })
	return uint64(a), uint64(b), uint64(p), err
}

// FlatSaveVertex / FlatLoadVertex: the edge `.vertex` stream (none_vectorstore.go:308-516 and the f16/f8/bf16 twins).
// FlatOneLaunchSearches: how many searches of <= 4 queries the one-launch kernel served (coltt_flat_one_launch_searches) —
// a diagnostic for dashboards: the RPC path of the reference issues exactly this shape (edge/edge.go:610-690).
func FlatOneLaunchSearches(h Handle) (uint64, error) {
	var n C.uint64_t
	err := call(func() C.int { return C.coltt_flat_one_launch_searches(h, &n) })
	return uint64(n), err
}

func FlatSaveVertex(h Handle, metaIds []uint64, metaBlobs [][]byte) ([]byte, error) {
	n := len(metaIds)
	var cptr **C.uint8_t
	var clen *C.uint32_t
	var pins []unsafe.Pointer
	if n > 0 {
		cptr = (**C.uint8_t)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))
		clen = (*C.uint32_t)(C.malloc(C.size_t(n) * 4))
		defer C.free(unsafe.Pointer(cptr))
		defer C.free(unsafe.Pointer(clen))
		ps := unsafe.Slice(cptr, n)
		ls := unsafe.Slice(clen, n)
		for i, b := range metaBlobs {
			p := C.CBytes(b)
			pins = append(pins, p)
			ps[i], ls[i] = (*C.uint8_t)(p), C.uint32_t(len(b))
		}
		defer func() {
			for _, p := range pins {
				C.free(p)
			}
		}()
	}
	var need C.uint64_t
	if err := call(func() C.int { return C.coltt_flat_save_vertex(h, uptr(metaIds), cptr, clen, C.uint64_t(n), nil, 0, &need) }); err != nil {
		return nil, err
	}
	out := make([]byte, int(need))
	err := call(func() C.int { return C.coltt_flat_save_vertex(h, uptr(metaIds), cptr, clen, C.uint64_t(n), bptr(out), need, &need) })
	return out[:int(need)], err
}
func FlatLoadVertex(h Handle, data []byte, elemBytes int, dim uint32) (ids []uint64, metaOff []uint64, metaLen []uint32, err error) {
	capN := uint64(len(data))/uint64(16+uint32(elemBytes)*dim) + 1 // key u64 + vecLen u32 + codes + metaCount u32
	ids = make([]uint64, capN)
	metaOff = make([]uint64, capN)
	metaLen = make([]uint32, capN)
	var n C.uint64_t
	err = call(func() C.int {
		return C.coltt_flat_load_vertex(h, bptr(data), C.uint64_t(len(data)), &n, uptr(ids), uptr(metaOff),
			(*C.uint32_t)(unsafe.Pointer(&metaLen[0])), C.uint64_t(capN))
	})
	if err != nil {
		return nil, nil, nil, err
	}
	return ids[:n], metaOff[:n], metaLen[:n], nil
}
