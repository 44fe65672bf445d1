"""The sweep behind tests/golden/search_plan.npz: every (knob setting, index facts, nq, k, ef, force) the search-plan fixture holds, and the two ways to
answer it — the library's own coltt_hnsw_search_plan_host, or a recording shim built from another commit (profiles/search_plan_kernels.md says how the
fixture's was made).  No device.

  python tools/search_plan_sweep.py --record SHIM.so OUT.npz    record the answers of `coltt_parent_plan_shim` exported by SHIM.so
  python tools/search_plan_sweep.py --diff FIXTURE.npz          the library beside the sources against a fixture: prints the rows that differ

A fixture holds `knobs` (one JSON object of COLTT_* settings per knob set), `inputs` [rows][len(IN_COLS)] and `answers` [rows][len(OUT_COLS)]."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

COS, L2 = 0, 1
F32, F16, F8, BF16 = 0, 1, 2, 3
FACT_COLS = ("dim", "metric", "quant", "stride", "slots", "m_max0", "r8", "shadow8", "shadow16", "vis_ready", "vis_regions")
IN_COLS = ("knob_set",) + FACT_COLS + ("nq", "k", "ef", "force")
# rc: the call's return code; err: which message (1 ef > 4096, 2 LDS beyond 160 KiB, 3 walk variant not compiled); the rest: coltt_hnsw_search_plan
PLAN_COLS = ("family", "ef", "ef_pad", "hcap", "lds", "vis_kind", "w2", "bloom_words", "ev8", "nt", "filter", "upper", "v16_bits", "v16_limit", "per_cu", "grid",
             "rows8_launch", "lat_seq", "lat_helpers", "r8")
OUT_COLS = ("rc", "err") + PLAN_COLS
ERR_MARKS = ((1, b"> 4096"), (2, b"B of LDS"), (3, b"is not compiled into this build"), (4, b"no instance for line-transposed rows"))
VIS16_LIMIT = 1 << 24   # the most slots the 16-bit visited table represents (vis16.hpp: 14 tag bits + 10 bucket bits)

EFS = (10, 64, 128, 129, 256, 1024, 4096, 4097)
NQS = (1, 256, 257, 10000)
FORCES = (0, 1, 3)


def qbytes(q):
    return 4 if q == F32 else (1 if q == F8 else 2)


def r8_values(dim, quant):
    """the values COLTT_ROWS8 = 0 / 1 / 2 give an index of this shape (hnsw.hip: rows8_shape)"""
    ok = quant != F8 and (dim * qbytes(quant)) % 128 == 0
    return (0, 1) if ok else (0,)


def facts(dim, metric, quant, r8, shadows, slots, regions, m_max0):
    return (dim, metric, quant, dim * qbytes(quant), slots, m_max0, r8, 1 if shadows & 8 else 0, 1 if shadows & 16 else 0, 1 if regions else 0, regions)


def shapes(dims, quants, metrics):
    """(dim, metric, quant, r8, shadows): the shadows an index of that shape can keep (f32 cosine, line-transposed)"""
    for dim, quant, metric in itertools.product(dims, quants, metrics):
        for r8 in r8_values(dim, quant):
            for sh in ((0, 16, 8, 24) if (r8 and quant == F32 and metric == COS) else (0,)):
                yield dim, metric, quant, r8, sh


def default_rows():
    """the default policy: the full product of a reduced grid, then each factor's remaining values over a base set"""
    out = []
    for shp in shapes((64, 128, 256, 384, 768, 1536, 4096), (F32, F16, F8), (COS, L2)):
        for slots, regions, m in itertools.product((0, 1000, 10 ** 7, VIS16_LIMIT + 1), (0, 2048), (32, 2048)):
            f = facts(*shp, slots, regions, m)
            out += [f + (nq, 10, ef, force) for ef, nq, force in itertools.product(EFS, NQS, FORCES)]
    # the values the product leaves out: slots 1 and the 16-bit limit itself, 256 regions, binary16's sibling format, k above ef
    base = list(shapes((128, 768, 4096), (F32, F16, BF16, F8), (COS, L2)))
    for shp in base:
        for slots, regions in ((1, 2048), (VIS16_LIMIT, 0), (VIS16_LIMIT, 256), (10 ** 7, 256), (VIS16_LIMIT - 1, 2048)):
            f = facts(*shp, slots, regions, 32)
            out += [f + (nq, 10, ef, force) for ef, nq, force in itertools.product(EFS, NQS, FORCES)]
        f = facts(*shp, 10 ** 7, 2048, 32)
        out += [f + (nq, k, ef, 0) for ef, nq, k in itertools.product((10, 128), (1, 257), (1, 100, 129, 200, 5000))]
    # beyond the table: rows so long that no walk's LDS fits (the only way to the 160 KiB error)
    for shp in shapes((32768,), (F32, F16), (COS,)):
        f = facts(*shp, 1000, 2048, 32)
        out += [f + (nq, 10, ef, 0) for ef, nq in itertools.product((10, 129, 4096), (1, 257))]
    return out


KNOB_SETS = [{}] + [{k: v} for k, vs in (
    ("COLTT_VISG", ("0", "1")),
    ("COLTT_WALK2", ("off", "2", "3", "5", "6", "15")),
    ("COLTT_WALK2_LDS", ("off", "2", "6")),
    ("COLTT_BLOOM_KB", ("1", "2", "16", "64")),
    ("COLTT_WAVES_PER_CU", ("1", "2", "8", "12")),
    ("COLTT_EV8", ("0",)),
    ("COLTT_ROWS_NT", ("0", "1", "-1")),
    ("COLTT_ROWS_NT_MIN_MB", ("0", "100000000")),
    ("COLTT_ROW_FILTER", ("0", "1")),
    ("COLTT_ROW_FILTER_BITS", ("8", "16", "8i")),
    ("COLTT_ROW_FILTER_UPPER", ("0", "1")),
    ("COLTT_DESCENT_NT", ("0", "1")),
    ("COLTT_VIS16", ("0",)),
    ("COLTT_VIS16_BUCKET_BITS", ("1", "4", "10")),
    ("COLTT_LAT_MAX_NQ", ("0", "1", "300", "100000")),
    ("COLTT_MW_MAX_NQ", ("0", "300")),
    ("COLTT_LAT_SEQ", ("1",)),
    ("COLTT_LAT_HELPERS", ("1", "3", "5")),
) for v in vs] + [
    {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": b} for b in ("8", "16", "8i")
] + [
    {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_UPPER": "1"}, {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": "16", "COLTT_ROW_FILTER_UPPER": "1"},
    {"COLTT_ROWS_NT": "1", "COLTT_DESCENT_NT": "1"}, {"COLTT_ROWS_NT": "1", "COLTT_ROW_FILTER": "1"}, {"COLTT_ROW_FILTER": "1", "COLTT_VIS16": "0"},
    {"COLTT_LAT_MAX_NQ": "300", "COLTT_MW_MAX_NQ": "0"}, {"COLTT_ROW_FILTER": "1", "COLTT_VIS16_BUCKET_BITS": "1"}, {"COLTT_ROW_FILTER": "1", "COLTT_VIS16_BUCKET_BITS": "4"},
]


def knob_rows():
    """every knob alone at each of its values (and the pairs above) over facts that reach its rule"""
    shp = [(768, COS, F32, 1, sh) for sh in (0, 16, 8, 24)] + [(768, COS, F32, 0, 0), (768, L2, F32, 1, 0), (768, COS, F16, 1, 0), (768, COS, F8, 0, 0),
                                                               (128, COS, F32, 0, 0), (4096, COS, F32, 1, 8), (256, L2, F16, 0, 0)]
    fs = [facts(*s, slots, regions, 32) for s in shp for slots in (1000, 10 ** 7, VIS16_LIMIT + 1) for regions in (0, 2048)]
    fs += [facts(768, COS, F32, 1, 8, 10 ** 7, 2048, 2048), facts(768, COS, F32, 1, 8, 10 ** 7, 2048, 64)]
    return [f + (nq, 10, ef, force) for f in fs for ef, nq, force in itertools.product((10, 128, 129, 1024), (1, 8, 257), FORCES)]


def inputs():
    rows = [(0,) + r for r in default_rows()]
    kr = knob_rows()
    for i in range(1, len(KNOB_SETS)):
        rows += [(i,) + r for r in kr]
    return np.asarray(rows, np.int64)


def with_knobs(knobs, reload):
    """set exactly these COLTT_* knobs in the environment (all others of the sweep unset), then reload the library's snapshot"""
    for ks in KNOB_SETS:
        for k in ks:
            os.environ.pop(k, None)
    os.environ.update(knobs)
    reload()


def run_library(inp, knob_sets):
    """the answers of coltt_hnsw_search_plan_host, [rows][len(OUT_COLS)]"""
    import coltt_amd
    from coltt_amd import hnsw as H
    out = np.zeros((len(inp), len(OUT_COLS)), np.int64)
    for ki, knobs in enumerate(knob_sets):
        sel = np.nonzero(inp[:, 0] == ki)[0]
        if not len(sel):
            continue
        with_knobs(knobs, lambda: coltt_amd.lib())   # the binding reloads the policy when it sees the environment change
        L = coltt_amd.lib()
        fn = L.coltt_hnsw_search_plan_host
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        plans = (H.SearchPlanC * len(sel))()
        base, step = C.addressof(plans), C.sizeof(H.SearchPlanC)
        last_f, fc = None, H.PlanFactsC()
        for j, r in enumerate(sel):
            row = inp[r]
            f = tuple(row[1:1 + len(FACT_COLS)])
            if f != last_f:
                for name, v in zip(FACT_COLS, f):
                    setattr(fc, name, int(v))
                last_f = f
            rc = fn(C.addressof(fc), int(row[-4]), int(row[-3]), int(row[-2]), int(row[-1]), base + j * step)
            if rc:
                msg = L.coltt_last_error()
                out[r, 0] = rc
                out[r, 1] = next((e for e, mark in ERR_MARKS if mark in msg), -1)
        got = np.frombuffer(plans, dtype=H.SEARCH_PLAN_DTYPE)
        for c, name in enumerate(PLAN_COLS):
            out[sel, 2 + c] = got[name]
    with_knobs({}, lambda: coltt_amd.lib())
    return out


def run_shim(path, inp, knob_sets):
    """the answers of the recording shim: int coltt_parent_plan_shim(const int64 facts[11], u64 nq, u32 k, u32 ef, int force, int64 out[24]) — out[0 .. 21] in
    OUT_COLS' order, [21] the distance core of the instance taken (0 pair-owned over natural rows, 1 over line-transposed rows, 2 eight lanes: r8 = non-zero)"""
    S = C.CDLL(path)
    fn = S.coltt_parent_plan_shim
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
    out = np.zeros((len(inp), len(OUT_COLS)), np.int64)
    buf = np.zeros(24, np.int64)
    for ki, knobs in enumerate(knob_sets):
        sel = np.nonzero(inp[:, 0] == ki)[0]
        with_knobs(knobs, S.coltt_policy_reload)
        for r in sel:
            row = inp[r]
            f = np.ascontiguousarray(row[1:1 + len(FACT_COLS)])
            rc = fn(f.ctypes.data, int(row[-4]), int(row[-3]), int(row[-2]), int(row[-1]), buf.ctypes.data)
            assert rc == 0, (rc, row)
            out[r, :21] = buf[:21]
            out[r, 21] = 0 if buf[0] else int(buf[21] != 0)   # r8: the instance taken reads line-transposed rows
    with_knobs({}, S.coltt_policy_reload)
    return out


def save(path, inp, ans):
    small = lambda a: a.astype(np.int32) if np.abs(a).max() < 2 ** 31 else a
    np.savez_compressed(path, knobs=np.asarray([json.dumps(k, sort_keys=True) for k in KNOB_SETS]), inputs_t=small(inp.T.copy()), answers_t=small(ans.T.copy()),
                        in_cols=np.asarray(IN_COLS), out_cols=np.asarray(OUT_COLS))


def load(path):
    z = np.load(path)
    assert tuple(z["in_cols"]) == IN_COLS and tuple(z["out_cols"]) == OUT_COLS, "the fixture's columns are not this sweep's"
    return [json.loads(s) for s in z["knobs"]], z["inputs_t"].T.astype(np.int64), z["answers_t"].T.astype(np.int64)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--record":
        inp = inputs()
        ans = run_shim(sys.argv[2], inp, KNOB_SETS)
        save(sys.argv[3], inp, ans)
        print(f"{len(inp)} rows, {len(KNOB_SETS)} knob sets -> {sys.argv[3]} ({os.path.getsize(sys.argv[3])} bytes)")
    elif len(sys.argv) == 3 and sys.argv[1] == "--diff":
        knobs, inp, want = load(sys.argv[2])
        got = run_library(inp, knobs)
        bad = np.nonzero((got != want).any(axis=1))[0]
        print(f"{len(inp)} rows, {len(bad)} differ")
        for r in bad[:40]:
            cols = [OUT_COLS[c] for c in np.nonzero(got[r] != want[r])[0]]
            print(knobs[inp[r, 0]], dict(zip(IN_COLS[1:], inp[r, 1:].tolist())), {c: (int(want[r, OUT_COLS.index(c)]), int(got[r, OUT_COLS.index(c)])) for c in cols})
        sys.exit(1 if len(bad) else 0)
    else:
        sys.exit(__doc__)
