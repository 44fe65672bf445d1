#!/usr/bin/env python3
"""What a comparison predicate over a device-resident attribute column costs, on one MI355X, against today's route for the same filter.

    python tools/attr_filter_probe.py --resources-only --out profiles/attr_filter_probe_1m128_f32.jsonl     (no device: the first line)
    python tools/attr_filter_probe.py [--n 1000000] [--dim 128] --out profiles/attr_filter_probe_1m128_f32.jsonl

Index: --n x --dim f32, built on the GPU, with one I64 column a (a permutation of 0 .. n-1) and one F64 column b (another permutation, halved),
so `a < t` allows exactly t vertices.  Per fraction f in --fracs, t = f * n:
  (a) attr        coltt_hnsw_filter_eval_attr of the one-predicate programme  a < t;
  (b) host        today's route on the same data: numpy compare + nonzero over the host copy of the column, then coltt_hnsw_filter_create
                  on the ids (both inside the timed window: the compare is per request, it has no hot term to keep);
  (c) leaves      coltt_hnsw_filter_eval of  A B AND  over two resident leaves whose intersection is the same set: the same two launches
                  without the column reads — the floor;
and once: (a2 / b2 / c2) the two-predicate  a >= x AND b < y  the same three ways; (d) coltt_hnsw_filter_eval_attr_batch of --batch programmes
`a < t_i` with distinct operands against as many runs of (b); (e) coltt_hnsw_attr_set of all n values.
Every timing is the wall time of the call from Python, the median of --reps calls after --warmup calls, all in one process; the filters a timed
call creates are destroyed outside the timed window; every evaluation is checked equal to its filter_create twin.
--resources-only compiles attr_filter.hpp for gfx950 with -Rpass-analysis=kernel-resource-usage and writes the evaluate kernel's scratch, VGPRs
and occupancy as one line (the file's first)."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def med(fn, after, warmup, reps):
    """median wall ms of fn() over `reps` calls after `warmup`; after(result) runs outside the timed window"""
    ts = []
    for r in range(warmup + reps):
        t0 = time.perf_counter(); out = fn(); dt = (time.perf_counter() - t0) * 1e3
        after(out)
        if r >= warmup:
            ts.append(dt)
    return round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)


def resources():
    """the compile-time resources of the kernels of attr_filter.hpp, with the build's flags"""
    from coltt_amd import build as B
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "attr_filter_tu.hip")
        with open(src, "w") as f:
            f.write('#include "attr_filter.hpp"\n')
        cmd = [B._hipcc()] + B.FLAGS + ["-I", B.CSRC, "-I", os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c", src,
                                        "-o", os.path.join(td, "attr_filter_tu.o")]
        err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            name = re.search(r"(attr_filter_eval_kernel|attr_scatter_kernel|attr_gather_kernel|filter_compact_kernel)", t)
            cur = out.setdefault(name.group(1), {}) if name else None
        elif cur is not None and ":" in t:
            k, v = t.rsplit(":", 1)
            cur[k.strip()] = v.strip()
    k = out["attr_filter_eval_kernel"]
    emit({"part": "resources", "what": "hipcc " + " ".join(B.FLAGS) + " -Rpass-analysis=kernel-resource-usage on attr_filter.hpp, cross-compiled",
          "attr_filter_eval_kernel": {"scratch_bytes_per_lane": int(k["ScratchSize [bytes/lane]"]), "vgprs": int(k["VGPRs"]), "waves_per_simd": int(k["Occupancy [waves/SIMD]"]),
                                      "sgprs": int(k["TotalSGPRs"]), "vgpr_spills": int(k["VGPRs Spill"]), "sgpr_spills": int(k["SGPRs Spill"]),
                                      "lds_bytes_per_block": int(k["LDS Size [bytes/block]"])},
          "others": {n: {"scratch_bytes_per_lane": int(v["ScratchSize [bytes/lane]"]), "vgprs": int(v["VGPRs"]), "waves_per_simd": int(v["Occupancy [waves/SIMD]"])}
                     for n, v in out.items() if n != "attr_filter_eval_kernel"}})
    assert int(k["ScratchSize [bytes/lane]"]) == 0, "the evaluate kernel's stack left the registers"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--fracs", default="0.001,0.01,0.1,0.5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1000, help="programmes of the batch call / runs of the host route it is measured against")
    ap.add_argument("--batch-reps", type=int, default=5)
    ap.add_argument("--out", default="", help="append every JSON line to this file as it is measured")
    ap.add_argument("--resources-only", action="store_true", help="no device: write the compile-time resource line and stop")
    a = ap.parse_args()
    global OUT
    OUT = a.out or None
    if a.resources_only:
        resources()
        return

    import torch
    import coltt_amd as G
    import bench as B
    L = G.lib()
    assert L.coltt_init(0) == 0
    dev = torch.device("cuda", 0)

    class Args: m = 16; ef = 128; efc = 200; build_batch = 16384
    t0 = time.perf_counter()
    h, _ = B.build_index(G, torch, dev, B.Dataset(torch, dev, a.dim, "normal"), a.n, a.dim, Args, 0xC0177, 0)
    n = h.Len()
    emit({"part": "setup", "n": n, "dim": a.dim, "quant": 0, "build_s": round(time.perf_counter() - t0, 1), "reps": a.reps, "warmup": a.warmup,
          "timing": "wall ms of the call from Python, median (min, max)", "column_bytes": n * 8, "bitmap_bytes": (n + 31) // 32 * 4})

    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rng = np.random.default_rng(0xA77)
    ids = np.arange(n, dtype=np.uint64)
    va = rng.permutation(n).astype(np.int64)                 # a < t allows exactly t vertices
    vb = rng.permutation(n).astype(np.float64) / 2.0
    ca, cb = h.AttrColumn(G.ATTR_I64), h.AttrColumn(G.ATTR_F64)

    # (e) attr_set of all n values (the first call also allocates the column)
    t0 = time.perf_counter(); assert ca.set(ids, va) == n; first = (time.perf_counter() - t0) * 1e3
    assert cb.set(ids, vb) == n
    e = med(lambda: ca.set(ids, va), lambda r: None, 1, max(3, a.reps // 4))
    emit({"part": "attr_set", "values": n, "upload_bytes": n * 12, "set_ms": e[0], "set_ms_min_max": e[1:], "first_call_ms": round(first, 4)})

    destroy = lambda f: L.coltt_hnsw_filter_destroy(f)   # noqa: E731
    AND = np.array([0, 1, G.FOP_AND], np.int32)

    def three_ways(label, frac, prog, preds, host_ids, leaf_sets):
        """(a) the predicates on the device, (b) the host route, (c) resident leaves of the same sets"""
        pa = (G.AttrPred * len(preds))(*preds)
        p = np.asarray(prog, np.int32)
        S = host_ids()
        ns = len(S)

        def ev():
            f = C.c_uint64(0); al = C.c_uint64(0)
            rc = L.coltt_hnsw_filter_eval_attr(h.h, vp(p), C.c_size_t(p.size), None, C.c_size_t(0), pa, C.c_size_t(len(preds)), C.byref(al), C.byref(f))
            assert rc == 0 and al.value == ns, (rc, al.value, ns)
            return f

        def host():
            s = host_ids()
            f = C.c_uint64(0); al = C.c_uint64(0)
            rc = L.coltt_hnsw_filter_create(h.h, vp(s), C.c_size_t(s.size), C.byref(al), C.byref(f))
            assert rc == 0 and al.value == ns, (rc, al.value, ns)
            return f

        leaves = [h.Filter(s) for s in leaf_sets(S)]
        lh = np.array([f.h.value for f in leaves], np.uint64)

        def lv():
            f = C.c_uint64(0); al = C.c_uint64(0)
            rc = L.coltt_hnsw_filter_eval(h.h, vp(AND), C.c_size_t(3), vp(lh), C.c_size_t(2), C.byref(al), C.byref(f))
            assert rc == 0 and al.value == ns, (rc, al.value, ns)
            return f

        f = ev(); tw = G.HnswFilter._from_handle(f.value, ns)
        same = bool(np.array_equal(tw.ids(), S)); tw.close()
        ra = med(ev, destroy, a.warmup, a.reps); rb = med(host, destroy, a.warmup, a.reps); rc_ = med(lv, destroy, a.warmup, a.reps)
        emit({"part": label, "slots": n, "frac": frac, "allowed": ns, "predicates": len(preds), "equal_to_create": same,
              "attr_ms": ra[0], "attr_ms_min_max": ra[1:], "host_ms": rb[0], "host_ms_min_max": rb[1:], "leaves_ms": rc_[0], "leaves_ms_min_max": rc_[1:],
              "host_over_attr": round(rb[0] / ra[0], 2), "attr_over_leaves": round(ra[0] / rc_[0], 2)})
        for x in leaves:
            x.close()

    def pred(col, op, i64=None, f64=None):
        q = G.AttrPred(); q.column = col.h.value; q.op = op; q.reserved = 0
        if f64 is not None:
            q.value.f64 = f64
        else:
            q.value.i64 = i64
        return q

    extra = n // 10

    def two_leaves(S):
        """A = S + a tenth of the collection, B = S + another, disjoint tenth: A AND B = S"""
        rest = np.setdiff1d(ids, S, assume_unique=True)
        rest = rest[rng.permutation(len(rest))[:2 * min(extra, len(rest) // 2)]]
        half = len(rest) // 2
        return [np.concatenate([S, rest[:half]]), np.concatenate([S, rest[half:]])]

    for frac in (float(x) for x in a.fracs.split(",")):
        t = int(round(frac * n))
        three_ways("single", frac, [0], [pred(ca, G.CMP_LT, i64=t)], lambda: np.nonzero(va < t)[0].astype(np.uint64), two_leaves)

    # a >= x AND b < y: half of the collection each, about a quarter together; the leaves of (c) are the two predicates' own sets
    x, y = n // 2, n / 4.0
    three_ways("two_predicates", None, [0, 1, G.FOP_AND], [pred(ca, G.CMP_GE, i64=x), pred(cb, G.CMP_LT, f64=y)],
               lambda: np.nonzero((va >= x) & (vb < y))[0].astype(np.uint64),
               lambda S: [np.nonzero(va >= x)[0].astype(np.uint64), np.nonzero(vb < y)[0].astype(np.uint64)])

    # (d) a batch of programmes `a < t_i` with distinct operands around 10 % against as many runs of the host route
    nb = a.batch
    ts_ = (n // 10 + np.arange(nb) * 7).astype(np.int64)
    plist = [pred(ca, G.CMP_LT, i64=int(t)) for t in ts_]
    pa = (G.AttrPred * nb)(*plist)
    progs = np.arange(nb, dtype=np.int32); off = np.arange(nb + 1, dtype=np.uint64)
    out = np.zeros(nb, np.uint64); al = np.zeros(nb, np.uint64)

    def evb():
        rc = L.coltt_hnsw_filter_eval_attr_batch(h.h, vp(progs), vp(off), C.c_size_t(nb), None, C.c_size_t(0), pa, C.c_size_t(nb), vp(al), vp(out))
        assert rc == 0 and np.array_equal(al, ts_.astype(np.uint64)), rc
        return out.copy()

    def hostb():
        hs = []
        for t in ts_:
            s = np.nonzero(va < t)[0].astype(np.uint64)
            f = C.c_uint64(0)
            assert L.coltt_hnsw_filter_create(h.h, vp(s), C.c_size_t(s.size), None, C.byref(f)) == 0
            hs.append(f)
        return hs

    def destroy_all(hs):
        for q in hs:
            L.coltt_hnsw_filter_destroy(C.c_uint64(int(q)) if not isinstance(q, C.c_uint64) else q)

    eb = med(evb, destroy_all, 1, a.batch_reps); hb = med(hostb, destroy_all, 0, max(1, a.batch_reps // 2))
    emit({"part": "batch", "slots": n, "programmes": nb, "predicates": nb, "allowed_about": int(ts_[nb // 2]), "attr_batch_ms": eb[0], "attr_batch_ms_min_max": eb[1:],
          "hosts_ms": hb[0], "hosts_ms_min_max": hb[1:], "hosts_over_attr_batch": round(hb[0] / eb[0], 2)})
    ca.close(); cb.close()


if __name__ == "__main__":
    main()
