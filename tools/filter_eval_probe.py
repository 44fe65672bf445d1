#!/usr/bin/env python3
"""What building a filter costs, on one MI355X: coltt_hnsw_filter_eval (two resident leaves combined on the device) against
coltt_hnsw_filter_create on the ids of the same set (the host route: a loop over the ids, a host bitmap, a host scan into the slot list,
two uploads — the only route before filter expressions), and coltt_hnsw_filter_eval_batch of --batch programmes against as many
coltt_hnsw_filter_create calls.

    python tools/filter_eval_probe.py [--n 1000000] [--dim 128] [--out profiles/filter_eval_probe_1m128_f32.jsonl]

Index: --n x --dim f32, built on the GPU.  Per fraction f in --fracs: a random set S of f * n vertices and two resident leaves A = S + a tenth
of the collection, B = S + another, disjoint tenth, so that A AND B = S exactly.  The set algebra that produces the id list of S (numpy, the
stand-in for the caller's host evaluation of its inverted index) is NOT counted against filter_create: only the call is timed.  Every
timing is the wall time of the C call from Python, the median of --reps calls after --warmup calls, all in one process; the filters a timed
call creates are destroyed outside the timed window.  The result of every evaluation is checked equal to the filter_create twin."""
import argparse
import ctypes as C
import json
import os
import sys
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--fracs", default="0.001,0.01,0.1,0.5")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1000, help="programmes of the batch call / filter_create calls it is measured against")
    ap.add_argument("--out", default="", help="append every JSON line to this file as it is measured")
    a = ap.parse_args()
    global OUT
    OUT = a.out or None

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
          "timing": "wall ms of the C call from Python, median (min, max)", "bitmap_bytes": (n + 31) // 32 * 4})

    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    prog = np.array([0, 1, G.FOP_AND], np.int32)
    rng = np.random.default_rng(0xF11)
    for frac in (float(x) for x in a.fracs.split(",")):
        perm = rng.permutation(n)
        ns = int(round(frac * n)); extra = min(n // 10, (n - ns) // 2)
        S = np.sort(perm[:ns]).astype(np.uint64)
        fa = h.Filter(np.concatenate([perm[:ns], perm[ns:ns + extra]]))
        fb = h.Filter(np.concatenate([perm[:ns], perm[ns + extra:ns + 2 * extra]]))
        lh = np.array([fa.h.value, fb.h.value], np.uint64)

        def ev():
            f = C.c_uint64(0); al = C.c_uint64(0)
            rc = L.coltt_hnsw_filter_eval(h.h, vp(prog), C.c_size_t(3), vp(lh), C.c_size_t(2), C.byref(al), C.byref(f))
            assert rc == 0 and al.value == ns, (rc, al.value, ns)
            return f

        def cr():
            f = C.c_uint64(0); al = C.c_uint64(0)
            rc = L.coltt_hnsw_filter_create(h.h, vp(S), C.c_size_t(S.size), C.byref(al), C.byref(f))
            assert rc == 0 and al.value == ns, (rc, al.value, ns)
            return f

        destroy = lambda f: L.coltt_hnsw_filter_destroy(f)   # noqa: E731
        with h.FilterEval([0, 1, G.FOP_AND], [fa, fb]) as f:      # the evaluation gives the set
            same = bool(np.array_equal(f.ids(), S))
        e = med(ev, destroy, a.warmup, a.reps); c = med(cr, destroy, a.warmup, a.reps)
        emit({"part": "single", "frac": frac, "allowed": ns, "leaf_allowed": [fa.allowed, fb.allowed], "equal_to_create": same,
              "eval_ms": e[0], "eval_ms_min_max": e[1:], "create_ms": c[0], "create_ms_min_max": c[1:], "create_over_eval": round(c[0] / e[0], 2)})

        nb = a.batch
        progs = np.tile(prog, nb); off = (np.arange(nb + 1, dtype=np.uint64) * 3)
        out = np.zeros(nb, np.uint64); al = np.zeros(nb, np.uint64)

        def evb():
            rc = L.coltt_hnsw_filter_eval_batch(h.h, vp(progs), vp(off), C.c_size_t(nb), vp(lh), C.c_size_t(2), vp(al), vp(out))
            assert rc == 0 and (al == ns).all(), rc
            return out.copy()

        def crb():
            hs = []
            for _ in range(nb):
                hs.append(cr())
            return hs

        def destroy_all(hs):
            for x in hs:
                L.coltt_hnsw_filter_destroy(C.c_uint64(int(x)) if not isinstance(x, C.c_uint64) else x)

        eb = med(evb, destroy_all, a.warmup, a.reps); cb = med(crb, destroy_all, a.warmup, a.reps)
        emit({"part": "batch", "frac": frac, "allowed": ns, "programmes": nb, "eval_batch_ms": eb[0], "eval_batch_ms_min_max": eb[1:],
              "creates_ms": cb[0], "creates_ms_min_max": cb[1:], "creates_over_eval_batch": round(cb[0] / eb[0], 2)})
        fa.close(); fb.close()


if __name__ == "__main__":
    main()
