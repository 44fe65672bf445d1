"""The case table of the latency kernel's instance tests (hnsw_search_lat_kernel<METRIC, QUANT, TP, SEQ>, coltt_amd/csrc/hnsw_lat.hpp): which index shapes
and knobs reach which of the 28 compiled instances.  Pure data and arithmetic: test_latency_cases_host.py holds the table against the plan function
without a device, test_gpu_latency_instances.py runs every case on one.

The library compiles, per metric (cosine, L2):
  f32 and 2-byte rows ("bf16" shares the binary16 device code): TP staged / any-lines / 24 / 12 on the pipelined walk, TP staged / any-lines on the
  sequential one — 6 instances each; f8 rows: staged only, both walks — 2 instances.   2 x (6 + 6 + 2) = 28."""
from collections import namedtuple

COSINE, L2 = 0, 1
Q_NONE, Q_F16, Q_F8, Q_BF16 = 0, 1, 2, 3
QUANT_BYTES = {Q_NONE: 4, Q_F16: 2, Q_F8: 1, Q_BF16: 2}
QUANT_NAME = {Q_NONE: "f32", Q_F16: "f16", Q_F8: "f8", Q_BF16: "bf16"}
TP_STAGED, TP_ANY = 0, -1
LAT_MAX_STRIDE, LAT_MIN_STRIDE, LAT_MASTERS = 3200, 1024, 8
PLAN_LATENCY = 0

# every knob the plan or the index's creation reads: cleared before a case sets its own
KNOBS = ("COLTT_ROW_FILTER", "COLTT_ROW_FILTER_BITS", "COLTT_ROW_FILTER_UPPER", "COLTT_VIS16", "COLTT_VIS16_BUCKET_BITS", "COLTT_ROWS_NT", "COLTT_ROWS_NT_MIN_MB",
         "COLTT_EV8", "COLTT_WALK2", "COLTT_WALK2_LDS", "COLTT_VISG", "COLTT_BLOOM_KB", "COLTT_WAVES_PER_CU", "COLTT_DESCENT_NT", "COLTT_LAT_MAX_NQ", "COLTT_MW_MAX_NQ",
         "COLTT_LAT_SEQ", "COLTT_LAT_HELPERS", "COLTT_ROW_SHADOW", "COLTT_ROW_SHADOW_BITS", "COLTT_ROWS8")

# name; group A / B / C / D; row format; dim; metric; m (mMax0 = 2 m); seq: the COLTT_LAT_SEQ a search runs under ("0" = unset);
# rows8: the COLTT_ROWS8 the index is created under (None = unset); ef200: (k 10, ef 200) still plans the latency kernel
Case = namedtuple("Case", "name group quant dim metric m seq rows8 ef200")


def _c(name, group, quant, dim, metric, m=16, seq="0", rows8=None, ef200=True):
    return Case(name, group, quant, dim, metric, m, seq, rows8, ef200)


def _both_walks(name, *a, **kw):
    return [_c(name + "-pipelined", *a, seq="0", **kw), _c(name + "-sequential", *a, seq="1", **kw)]


CASES = [
    # ---- A: line-transposed rows, pipelined walk
    # A1: TP 12
    _c("a1-f32-384-cos", "A", Q_NONE, 384, COSINE), _c("a1-f32-384-l2", "A", Q_NONE, 384, L2),
    _c("a1-f16-768-cos", "A", Q_F16, 768, COSINE), _c("a1-f16-768-l2", "A", Q_F16, 768, L2), _c("a1-bf16-768-cos", "A", Q_BF16, 768, COSINE),
    # A2: TP 24 (f32 768-d L2: the only case that names <L2, f32, 24, pipelined>)
    _c("a2-f16-1536-cos", "A", Q_F16, 1536, COSINE), _c("a2-f16-1536-l2", "A", Q_F16, 1536, L2),
    _c("a2-f32-768-cos", "A", Q_NONE, 768, COSINE), _c("a2-f32-768-l2", "A", Q_NONE, 768, L2),
    # A3: any-lines; 800-d f32 and 1600-d f16 are 25 lines = LAT_MAX_PIECES
    _c("a3-f16-512-cos", "A", Q_F16, 512, COSINE), _c("a3-f16-1024-l2", "A", Q_F16, 1024, L2), _c("a3-f32-512-l2", "A", Q_NONE, 512, L2),
    _c("a3-f32-800-cos", "A", Q_NONE, 800, COSINE), _c("a3-f16-1600-cos", "A", Q_F16, 1600, COSINE),
    # ---- B: line-transposed rows, sequential walk: mMax0 48 (two chunks per expansion), or COLTT_LAT_SEQ=1 over the index of an A case
    # (f32 512-d L2: the only case that names <L2, f32, any-lines, sequential>)
    _c("b-f32-256-cos-m24", "B", Q_NONE, 256, COSINE, m=24), _c("b-f16-768-l2-m24", "B", Q_F16, 768, L2, m=24),
    _c("b-f32-768-cos-seq", "B", Q_NONE, 768, COSINE, seq="1"), _c("b-f16-512-cos-seq", "B", Q_F16, 512, COSINE, seq="1"),
    _c("b-f32-512-l2-seq", "B", Q_NONE, 512, L2, seq="1"),
    # ---- C: natural-order rows, staged through LDS, both walks.  300-d: nblk 2, one odd group, scalar tail 4; 799-d: stride 3 200 = LAT_MAX_STRIDE;
    # f16 1000-d: nblk 7; f8 1024-d: nblk 8; f8 1100-d: tail; 768-d under COLTT_ROWS8=0: the layout A/B partner of a2-f32-768-cos
    # ("bf16" 1000-d L2: the only cases that name the two <L2, 2-byte, staged> instances)
    *_both_walks("c-f32-300-l2", "C", Q_NONE, 300, L2),
    *_both_walks("c-f32-799-cos", "C", Q_NONE, 799, COSINE, ef200=False),
    *_both_walks("c-f16-1000-cos", "C", Q_F16, 1000, COSINE),
    *_both_walks("c-bf16-1000-l2", "C", Q_BF16, 1000, L2),
    *_both_walks("c-f8-1024-cos", "C", Q_F8, 1024, COSINE),
    *_both_walks("c-f8-1100-l2", "C", Q_F8, 1100, L2),
    *_both_walks("c-f32-768-cos-rows8off", "C", Q_NONE, 768, COSINE, rows8="0", ef200=False),
    _c("c-f32-300-l2-m24", "C", Q_NONE, 300, L2, m=24),
    # ---- D: NaN distances and exact ties (two all-zero rows, rows 1000-1999 copies of rows 0-999), m 8
    *_both_walks("d-f32-256-cos-ties", "D", Q_NONE, 256, COSINE, m=8),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# beside c-f32-799-cos: one element more and the row (stride 3 216) no longer fits the staging area — the plan must leave the latency kernel
CASE_801 = _c("c-f32-801-cos-not-latency", "C", Q_NONE, 801, COSINE, ef200=False)

# (k, ef) of every case, at nq 1, 7 and 40: the smallest sets (the speculatively popped candidate is truncated away), k > ef (the walk runs with max(ef, k)),
# ef 200 where the plan still says latency
NQS = (1, 7, 40)
SEARCHES = ((1, 1), (1, 2), (1, 3), (10, 20), (10, 64), (10, 128), (50, 20), (10, 200))
TIES_K = 300                                # group D also answers k = ef = 300
# the call at the edge of the hash-capacity rule, the second-query call (COLTT_LAT_MAX_NQ=512, nq 300 on a grid of 256) and the helper calls
EDGE_CASES = ("a2-f32-768-cos", "b-f16-768-l2-m24", "c-f32-799-cos-pipelined")
SECOND_QUERY_CASES = ("a1-f16-768-cos", "b-f32-256-cos-m24", "c-f32-300-l2-pipelined", "c-f8-1024-cos-sequential")
SECOND_QUERY_NQ = 300
HELPER_CASES = ("a2-f32-768-cos", "c-f32-300-l2-pipelined")
HELPER_SEQ_CASE = "b-f32-768-cos-seq"
HELPER_NQS, HELPER_EFS = (1, 8, 9), (64, 200)


def stride(c):
    """bytes per stored row: the elements, rounded up to 16"""
    return (c.dim * QUANT_BYTES[c.quant] + 15) & ~15


def r8(c):
    """rows8_shape (hnsw.hip): 2- and 4-byte rows of whole 128-byte lines are line-transposed, from 256 elements on (COLTT_ROWS8=2 lifts that limit);
    f8 rows never; an index created under COLTT_ROWS8=0 never"""
    if c.quant == Q_F8 or c.rows8 == "0":
        return 0
    if c.rows8 != "2" and c.dim < 256:
        return 0
    return int((c.dim * QUANT_BYTES[c.quant]) % 128 == 0)


def lat_seq(c):
    return int(c.seq == "1" or 2 * c.m > 32)


def tp_of(r8_, stride_, seq_):
    """launch_search_lat's choice of instance: natural order -> staged; line-transposed -> 12 / 24 lines as a constant on the pipelined walk, else any-lines"""
    if not r8_:
        return TP_STAGED
    lines = stride_ >> 7
    return lines if (lines in (12, 24) and not seq_) else TP_ANY


def tp(c):
    return tp_of(r8(c), stride(c), lat_seq(c))


def instance(c):
    """(metric, row format, TP, SEQ) — "bf16" counted with f16"""
    fmt = {Q_NONE: "f32", Q_F16: "2-byte", Q_BF16: "2-byte", Q_F8: "f8"}[c.quant]
    return (c.metric, fmt, tp(c), lat_seq(c))


def all_instances():
    out = set()
    for metric in (COSINE, L2):
        for fmt in ("f32", "2-byte"):
            out |= {(metric, fmt, t, 0) for t in (TP_STAGED, TP_ANY, 24, 12)} | {(metric, fmt, t, 1) for t in (TP_STAGED, TP_ANY)}
        out |= {(metric, "f8", TP_STAGED, 0), (metric, "f8", TP_STAGED, 1)}
    return out


def index_key(c):
    """cases that differ in search-time knobs only share one index"""
    return (c.group == "D", c.quant, c.dim, c.metric, c.m, c.rows8)


def sizes(c):
    """(rows built in batches, rows added by single Inserts).  2 400: with 1 200 rows and 12 % of them removed only ~40 level-0 entries of live rows still
    named a tombstone (37 - 42 over the 3 200-byte cases); the cases ask for 50.  Group D needs its 1 000 copied rows."""
    return (3000 if c.group == "D" else 2400), 40


def search_knobs(c):
    return {"COLTT_LAT_SEQ": "1"} if c.seq == "1" else {}


def facts(c, vis_ready=0, slots=None):
    """coltt_hnsw_plan_facts of the case's index, by hand (no shadows: the latency plan reads none)"""
    n1, n2 = sizes(c)
    return dict(dim=c.dim, metric=c.metric, quant=c.quant, m_max0=2 * c.m, stride=stride(c), slots=n1 + n2 if slots is None else slots, r8=r8(c),
                shadow8=0, shadow16=0, vis_ready=vis_ready, vis_regions=1024 if vis_ready else 0)


def largest_latency_ef(plan, k=10, hi=4096):
    """the largest ef in [k, hi] at which plan(1, k, ef) is the latency family, by bisection (the plan function is the authority: a larger set never fits a
    table a smaller one does not); None if not even ef = k is"""
    if plan(1, k, k)["family"] != PLAN_LATENCY:
        return None
    lo = k                                    # invariant: plan(lo) is latency, plan(hi + 1) is not (ef > 4096 is refused)
    if plan(1, k, hi)["family"] == PLAN_LATENCY:
        return hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(1, k, mid)["family"] == PLAN_LATENCY:
            lo = mid
        else:
            hi = mid
    return lo
