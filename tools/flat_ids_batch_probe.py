#!/usr/bin/env python3
"""A candidate list per query on the FLAT store (coltt_flat_search_ids_batch) on one MI355X: 64 queries with 64 distinct random lists of
0.1 %, 1 % and 10 % of a 1 M x 768 f16 cosine store, k = 10.

    python tools/flat_ids_batch_probe.py [--n 1000000] [--dim 768] [--quant 1] [--nq 64] [--k 10] [--reps 20] [--out FILE]

Per list size (part "point"; medians over --reps timed repetitions after one warm-up; ms = kernel time between the call's hipEvents
(coltt_last_kernel_ms_flat), wall = the whole call from Python):
  (i)   batch          the batch call, 64 lists (wall through the binding, which concatenates the 64 arrays; batch_abi_wall: the C call on
                       ids already in its one-array form)
  (ii)  singles        the loop of 64 coltt_flat_search_ids calls (the path before the batch call; kernel ms summed over the calls)
  (iii) shared_batch   64 queries sharing ONE list through the batch call
  (iv)  shared_exact   the same through coltt_flat_search_ids_mode(EXACT): the shared-list scan, the yardstick for the new scan's gather rate
  (v)   bytes read (pairs x row bytes) over the batch call's kernel time, as a fraction of the 8 TB/s HBM peak
and (part "batcher") 64 callers with their own 1 % (and 0.1 %) lists through coltt::IdsBatcher against 64 direct callers (tools/flat_ids_batcher_qps.cpp).
Rows of the batch are checked equal to the single calls at every point."""
import argparse
import ctypes as C
import json
import os
import platform
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACS = (0.001, 0.01, 0.1)
HBM_PEAK = 8.0e12
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def timed(f, fn, reps):
    ms, wall, out = [], [], None
    for _ in range(reps + 1):   # the first call warms up
        t0 = time.perf_counter(); out, kms = fn(); w = time.perf_counter() - t0
        ms.append(kms); wall.append(w * 1e3)
    return out, round(float(np.median(ms[1:])), 4), round(float(np.median(wall[1:])), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--quant", type=int, default=1)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--per-thread", type=int, default=300)
    ap.add_argument("--out", default="", help="append every JSON line to this file as it is measured")
    a = ap.parse_args()
    global OUT
    OUT = a.out or None
    import torch
    import coltt_amd as G
    L = G.lib()
    assert L.coltt_device_count() > 0 and L.coltt_init(0) == 0, "no HIP device: this probe measures, it has no fallback"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0xF1A7)
    f = G.FlatSpace(a.dim, G.COSINE, a.quant)
    f.Reserve(a.n)
    step = 100_000
    for b in range(0, a.n, step):   # rows generated on the device, appended through the dense fast path (id = slot)
        m = min(step, a.n - b)
        x = torch.randn((m, a.dim), generator=gen, device=dev, dtype=torch.float32)
        torch.cuda.synchronize()
        f.ChangedVertexDevice(x.data_ptr(), m, first_id=b)
    Q = torch.randn((a.nq, a.dim), generator=gen, device=dev, dtype=torch.float32).cpu().numpy()
    row_bytes = a.dim * {0: 4, 2: 1}.get(a.quant, 2)
    sel = G.SELECT_NEAREST

    def last_ms():
        ms = C.c_float(0); L.coltt_last_kernel_ms_flat(f.h, C.byref(ms)); return ms.value
    emit({"part": "setup", "box": platform.node(), "device": torch.cuda.get_device_name(0), "n": f.LoadSize(), "dim": a.dim, "quant": a.quant,
          "metric": "cosine", "nq": a.nq, "k": a.k, "reps": a.reps, "row_bytes": row_bytes})
    rng = np.random.default_rng(0x1D5)
    for frac in FRACS:
        m = int(a.n * frac)
        lists = [np.sort(rng.choice(a.n, m, replace=False).astype(np.uint64)) for _ in range(a.nq)]

        cand = np.concatenate(lists); off = np.arange(a.nq + 1, dtype=np.uint64) * np.uint64(m)

        def batch():
            r = f.FilterableVertexSearchBatch(lists, Q, a.k, sel); return r, last_ms()

        def batch_abi():   # the C call alone: the ids already in its one-array form
            r = f.FilterableVertexSearchBatch(cand, Q, a.k, sel, offsets=off); return r, last_ms()

        def singles():
            tot = 0.0; rows = []
            for i in range(a.nq):
                rows.append(f.FilterableVertexSearch(lists[i], Q[i:i + 1], a.k, sel)); tot += last_ms()
            return rows, tot

        def shared_batch():
            r = f.FilterableVertexSearchBatch(lists[:1], Q, a.k, sel, np.zeros(a.nq, np.uint32)); return r, last_ms()

        def shared_exact():
            r = f.FilterableVertexSearch(lists[0], Q, a.k, sel, G.MODE_EXACT); return r, last_ms()
        st0 = f.IdsBatchStats()
        (bi, bs, bc), b_ms, b_wall = timed(f, batch, a.reps)
        st1 = f.IdsBatchStats()
        pairs = (st1["pairs"] - st0["pairs"]) // (a.reps + 1)
        _, _, ba_wall = timed(f, batch_abi, a.reps)
        rows, s_ms, s_wall = timed(f, singles, a.reps)
        same = all(int(bc[i]) == int(rows[i][2][0]) and np.array_equal(bi[i], rows[i][0][0]) and
                   np.array_equal(bs[i].view(np.uint32), rows[i][1][0].view(np.uint32)) for i in range(a.nq))
        (si, ss, sc), sb_ms, sb_wall = timed(f, shared_batch, a.reps)
        (ei, es, ec), se_ms, se_wall = timed(f, shared_exact, a.reps)
        same_shared = np.array_equal(si, ei) and np.array_equal(ss.view(np.uint32), es.view(np.uint32)) and np.array_equal(sc, ec)
        emit({"part": "point", "frac": frac, "list_rows": m, "pairs": int(pairs),
              "batch_ms": b_ms, "batch_wall_ms": b_wall, "batch_abi_wall_ms": ba_wall, "singles_ms_sum": s_ms, "singles_wall_ms": s_wall,
              "singles_over_batch_kernel": round(s_ms / b_ms, 2), "singles_over_batch_wall": round(s_wall / b_wall, 2), "singles_over_batch_abi_wall": round(s_wall / ba_wall, 2), "rows_equal_singles": bool(same),
              "shared_batch_ms": sb_ms, "shared_batch_wall_ms": sb_wall, "shared_exact_ms": se_ms, "shared_exact_wall_ms": se_wall,
              "shared_batch_over_exact_kernel": round(sb_ms / se_ms, 3), "shared_rows_equal": bool(same_shared),
              "batch_bytes": int(pairs) * row_bytes, "batch_bytes_per_s": round(pairs * row_bytes / (b_ms * 1e-3), 1),
              "batch_fraction_of_hbm_peak": round(pairs * row_bytes / (b_ms * 1e-3) / HBM_PEAK, 4)})
    # 64 callers with their own 1 % lists through the C++ IdsBatcher against 64 direct callers
    T = a.nq
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "qps.so")
        libdir = os.path.dirname(G.lib_path())
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "flat_ids_batcher_qps.cpp"), "-o", so, "-L", libdir, "-lcoltt_gpu", f"-Wl,-rpath,{libdir}"])
        lib = C.CDLL(so)
        q = np.ascontiguousarray(np.tile(Q, (a.per_thread, 1))[:T * a.per_thread], np.float32)
        for frac in (0.01, 0.001):
            m = int(a.n * frac)
            lists = [np.sort(rng.choice(a.n, m, replace=False).astype(np.uint64)) for _ in range(T)]
            cand = np.concatenate(lists); off = np.arange(T + 1, dtype=np.uint64) * np.uint64(m)
            for batched in (0, 1, 0, 1, 0, 1):
                qps = C.c_double(0); nb = C.c_ulonglong(0)
                rc = lib.flat_ids_batcher_qps(f.h, C.c_uint32(a.dim), cand.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p),
                                              T, a.per_thread, C.c_uint32(a.k), sel, batched, C.byref(qps), C.byref(nb))
                emit({"part": "batcher", "mode": "batched" if batched else "direct", "threads": T, "frac": frac, "list_rows": m, "queries": T * a.per_thread, "rc": rc,
                      "qps": round(qps.value, 1), "batches": nb.value if batched else None})


if __name__ == "__main__":
    main()
