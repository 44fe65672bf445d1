#!/usr/bin/env python3
"""What reclaiming tombstoned slots costs, on one MI355X: coltt_hnsw_compact against the only routes there were before it — Commit -> Load into a
fresh index, and Export + FetchRows + BulkLoad into a fresh index (both move the whole collection through host memory, renumber the slots in
their own order and need a second index's worth of device memory while they run) — and what a search gains once no tombstone is left to test.

    python tools/compact_probe.py [--n 1000000] [--dim 128] [--out profiles/hnsw_compact_probe_1m128_f32.jsonl]

Index: --n x --dim f32 cosine, built on the GPU.  Per fraction f in --fracs (ascending): Remove is called until f * n vertices of a fixed random
order are gone, and the tombstoned index is snapshotted on the host (Export + FetchRows).  Compact changes the index it measures, so every
repetition first re-installs the snapshot with BulkLoad (not timed) and then times the call: `ms` is the call's own device time (hipEvents on
the mutation stream, coltt_hnsw_compact_stats.ms), `wall_ms` the wall time of the C call from Python.  hbm_frac = bytes_moved / ms against
8 TB/s; copy_gbps is a plain device-to-device copy of 512 MiB on the same device in the same process (bytes written per second, the unit of
bytes_moved), the yardstick for the move kernels.  The two host routes are timed as wall time on the same snapshot state into a fresh index.
Search: --nq queries at --ef on the tombstoned index and on the compacted one (wall time of the C call, queries per second; the answers are
checked equal).  Every figure is the median of --reps runs after --warmup (the slower host routes: --alt-reps), all in one process."""
import argparse
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


def med(vals):
    return round(float(np.median(vals)), 4), round(float(min(vals)), 4), round(float(max(vals)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--fracs", default="0.01,0.1,0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alt-reps", type=int, default=-1, help="repetitions of the two host routes (default: --reps)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--stage-bytes", type=int, default=0)
    ap.add_argument("--out", default="", help="append every JSON line to this file as it is measured")
    a = ap.parse_args()
    global OUT
    OUT = a.out or None
    alt_reps = a.reps if a.alt_reps < 0 else a.alt_reps

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
    # the yardstick of the move kernels: a plain device-to-device copy
    src = torch.empty(512 << 20, dtype=torch.uint8, device=dev); dst = torch.empty_like(src)
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    cp = []
    for r in range(a.warmup + a.reps):
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        if r >= a.warmup:
            cp.append(src.numel() / e0.elapsed_time(e1) / 1e6)
    del src, dst
    copy_gbps = med(cp)
    emit({"part": "setup", "n": n, "dim": a.dim, "quant": 0, "metric": "cosine", "build_s": round(time.perf_counter() - t0, 1), "reps": a.reps,
          "alt_reps": alt_reps, "warmup": a.warmup, "copy_gbps": copy_gbps[0], "copy_gbps_min_max": copy_gbps[1:],
          "timing": "median (min, max); ms = hipEvents inside the call, everything else wall time of the C calls from Python"})

    Q = torch.randn((a.nq, a.dim), generator=torch.Generator().manual_seed(7)).numpy()
    order = np.random.default_rng(0xC0).permutation(n)
    ids0 = h.Export()["ids"]
    removed = 0

    def qps(idx):
        ts = []
        for r in range(a.warmup + a.reps):
            t = time.perf_counter(); out = idx.Search(Q, 10, ef=a.ef); dt = time.perf_counter() - t
            if r >= a.warmup:
                ts.append(a.nq / dt)
        return med(ts), out

    for frac in (float(x) for x in a.fracs.split(",")):
        target = int(round(frac * n))
        t0 = time.perf_counter()
        for i, s in enumerate(order[removed:target]):
            h.Remove(int(ids0[s]))
            if i % 50_000 == 49_999:
                print(f"# removed {removed + i + 1}", flush=True)
        removed = max(removed, target)
        remove_s = time.perf_counter() - t0
        snap = h.Export(); rows = h.FetchRows()
        emit({"part": "tombstoned", "frac": frac, "removed": removed, "live": h.Len(), "remove_s": round(remove_s, 1)})

        h.BulkLoad(snap, rows)                               # every state below is this install of the snapshot (BulkLoad normalises the rows again)
        before_qps, before_ans = qps(h)
        ms, wall, stats = [], [], None
        for r in range(a.warmup + a.reps):
            if r:
                h.BulkLoad(snap, rows)                       # the call changed the index: put the tombstoned snapshot back (not timed)
            t = time.perf_counter(); stats = h.Compact(stage_bytes=a.stage_bytes); dt = (time.perf_counter() - t) * 1e3
            if r >= a.warmup:
                ms.append(stats["ms"]); wall.append(dt)
        after_qps, after_ans = qps(h)
        same = bool(all(np.array_equal(x, y) for x, y in zip(before_ans, after_ans)))
        m = med(ms); w = med(wall)
        emit({"part": "compact", "frac": frac, "slots_before": stats["slots_before"], "slots_after": stats["slots_after"],
              "rows_moved": stats["rows_moved"], "edges_dropped": stats["edges_dropped"], "bytes_moved": stats["bytes_moved"],
              "ms": m[0], "ms_min_max": m[1:], "wall_ms": w[0], "wall_ms_min_max": w[1:],
              "gbps": round(stats["bytes_moved"] / m[0] / 1e6, 1), "hbm_frac": round(stats["bytes_moved"] / m[0] / 8e9, 4),
              "frac_of_plain_copy": round(stats["bytes_moved"] / m[0] / 1e6 / copy_gbps[0], 3),
              "search_qps_tombstoned": before_qps[0], "search_qps_tombstoned_min_max": before_qps[1:],
              "search_qps_compacted": after_qps[0], "search_qps_compacted_min_max": after_qps[1:], "answers_equal": same})

        h.BulkLoad(snap, rows)                               # the tombstoned state again: the host routes start from it, and so do the next Removes
        cl, be = [], []
        for r in range(a.warmup + alt_reps if alt_reps else 0):   # --alt-reps 0: the call alone
            fresh = G.Hnsw(a.dim, G.COSINE, G.HnswCfg.default(m=Args.m, ef=Args.ef, ef_construction=Args.efc))
            t = time.perf_counter(); fresh.Load(h.Commit()); dt = (time.perf_counter() - t) * 1e3
            assert fresh.Len() == h.Len()
            fresh.close()
            if r >= a.warmup:
                cl.append(dt)
            fresh = G.Hnsw(a.dim, G.COSINE, G.HnswCfg.default(m=Args.m, ef=Args.ef, ef_construction=Args.efc))
            t = time.perf_counter(); fresh.BulkLoad(h.Export(), h.FetchRows()); dt = (time.perf_counter() - t) * 1e3
            fresh.close()
            if r >= a.warmup:
                be.append(dt)
        if cl:
            c = med(cl); b = med(be)
            emit({"part": "host-routes", "frac": frac, "commit_load_ms": c[0], "commit_load_ms_min_max": c[1:], "export_bulkload_ms": b[0],
                  "export_bulkload_ms_min_max": b[1:], "commit_load_over_compact": round(c[0] / w[0], 1), "export_bulkload_over_compact": round(b[0] / w[0], 1),
                  "note": "BulkLoad of the export keeps the tombstoned slots (it copies, it does not reclaim): dropping them on that route needs the caller's own remap on top"})


if __name__ == "__main__":
    main()
