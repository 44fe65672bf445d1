#!/usr/bin/env python3
"""What carrying resident filters and attribute columns through a compaction costs, on one MI355X: Hnsw.CompactCarry against the only route
there was before it — plain Compact, then every object made again from ids and values the caller kept on the host (filter_create per leaf, a
new column and attr_set per column).

    python tools/compact_carry_probe.py [--n 1000000] [--dim 128] [--out profiles/hnsw_compact_carry_probe_1m128_f32.jsonl]

Index: --n x --dim f32 cosine, built on the GPU, --frac of it removed in a fixed random order, the tombstoned state snapshotted on the host.
Objects: 1 / 100 / 1 000 (--filters) resident leaf filters whose allowed fractions are spread log-uniformly over 0.1 % .. 50 %, and --columns
attribute columns (I64 and F64 in turn) set on every id.  Both routes change the index they measure, so every repetition re-installs the
snapshot with BulkLoad and makes the objects again (neither is timed), then times ONE route:
  carry     CompactCarry(filters, columns): `ms` = the call's device time, `carry_ms` = the carry launches alone (coltt_hnsw_carry_stats.ms),
            `wall_ms` = the C call from Python;
  recreate  Compact(), then filter_create per leaf from its host ids and attr_create + attr_set per column from its host values: `ms` = the
            compaction's device time, `wall_ms` = everything, `filters_wall_ms` / `columns_wall_ms` its two parts.
carry_bytes = what the carry launches must move at least: per bitmap (filters and the columns' set bitmaps) the old words read and the new words
written, per filter the new words read again and the list entries written by the list kernel; the tombstones and the rank table, re-read per
bitmap, are left out (they are shared and stay in cache).  carry_hbm_frac = carry_bytes / carry_ms against 8 TB/s.  Every figure is the median
(min, max) of --reps runs after --warmup, all in one process.  No ratio is promised: the baseline is the recreate route here."""
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
    ap.add_argument("--frac", type=float, default=0.1)
    ap.add_argument("--filters", default="1,100,1000")
    ap.add_argument("--columns", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
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
    ids0 = h.Export()["ids"]
    order = np.random.default_rng(0xC0).permutation(n)
    target = int(round(a.frac * n))
    for s in order[:target]:
        h.Remove(int(ids0[s]))
    snap = h.Export(); rows = h.FetchRows()
    live = snap["deleted"] == 0
    emit({"part": "setup", "n": n, "dim": a.dim, "quant": 0, "metric": "cosine", "removed": target, "live": int(live.sum()), "columns": a.columns,
          "setup_s": round(time.perf_counter() - t0, 1), "reps": a.reps, "warmup": a.warmup,
          "timing": "median (min, max); ms / carry_ms = hipEvents inside the call, everything else wall time of the C calls from Python"})

    rng = np.random.default_rng(0xCA)
    col_vals = [rng.integers(-10**6, 10**6, n) if c % 2 == 0 else rng.normal(size=n) for c in range(a.columns)]
    col_type = [G.ATTR_I64 if c % 2 == 0 else G.ATTR_F64 for c in range(a.columns)]
    words_old, words_new = (n + 31) // 32, (int(live.sum()) + 31) // 32

    for nf in (int(x) for x in a.filters.split(",")):
        fracs = np.exp(rng.uniform(np.log(0.001), np.log(0.5), nf))
        leaf_ids = [ids0[rng.random(n) < f] for f in fracs]

        def install():
            """the tombstoned snapshot and the resident objects over it (not timed)"""
            h.BulkLoad(snap, rows)
            fl = [h.Filter(x) for x in leaf_ids]
            cl = []
            for c in range(a.columns):
                col = h.AttrColumn(col_type[c]); col.set(ids0, col_vals[c]); cl.append(col)
            return fl, cl

        def close(objs):
            for o in objs:
                o.close()

        ms, cms, wall, st, cs = [], [], [], None, None
        carried_ids = None
        for r in range(a.warmup + a.reps):
            fl, cl = install()
            t = time.perf_counter(); st, cs, al, ns = h.CompactCarry(fl, cl); dt = (time.perf_counter() - t) * 1e3
            if r >= a.warmup:
                ms.append(st["ms"]); cms.append(cs["ms"]); wall.append(dt)
            carried_ids = [fl[i].ids() for i in (0, nf - 1)]
            carried_col = cl[0].get(ids0[:1000])
            close(fl + cl)
        carry_bytes = (nf + a.columns) * (words_old + words_new) * 4 + nf * words_new * 4 + cs["list_entries"] * 4
        m, c, w = med(ms), med(cms), med(wall)
        emit({"part": "carry", "filters": nf, "columns": a.columns, "allowed_frac_min_max": [round(float(fracs.min()), 4), round(float(fracs.max()), 4)],
              "ms": m[0], "ms_min_max": m[1:], "carry_ms": c[0], "carry_ms_min_max": c[1:], "wall_ms": w[0], "wall_ms_min_max": w[1:],
              "bitmap_words": cs["bitmap_words"], "list_entries": cs["list_entries"], "column_values": cs["column_values"],
              "carry_bytes": carry_bytes, "carry_gbps": round(carry_bytes / c[0] / 1e6, 1), "carry_hbm_frac": round(carry_bytes / c[0] / 8e9, 4)})

        ms, wall, fw, cw = [], [], [], []
        same = True
        for r in range(a.warmup + a.reps):
            fl, cl = install()
            t = time.perf_counter(); st = h.Compact(); t1 = time.perf_counter()
            nfl = [h.Filter(x) for x in leaf_ids]; t2 = time.perf_counter()
            ncl = []
            for cix in range(a.columns):
                col = h.AttrColumn(col_type[cix]); col.set(ids0, col_vals[cix]); ncl.append(col)
            t3 = time.perf_counter()
            if r >= a.warmup:
                ms.append(st["ms"]); wall.append((t3 - t) * 1e3); fw.append((t2 - t1) * 1e3); cw.append((t3 - t2) * 1e3)
            same = same and all(np.array_equal(nfl[i].ids(), x) for i, x in zip((0, nf - 1), carried_ids))
            got = ncl[0].get(ids0[:1000])
            same = same and np.array_equal(got[0], carried_col[0]) and np.array_equal(got[1], carried_col[1])
            close(fl + cl + nfl + ncl)
        m2, w2, f2, c2 = med(ms), med(wall), med(fw), med(cw)
        emit({"part": "recreate", "filters": nf, "columns": a.columns, "ms": m2[0], "ms_min_max": m2[1:], "wall_ms": w2[0], "wall_ms_min_max": w2[1:],
              "filters_wall_ms": f2[0], "filters_wall_ms_min_max": f2[1:], "columns_wall_ms": c2[0], "columns_wall_ms_min_max": c2[1:],
              "recreate_wall_over_carry_wall": round(w2[0] / w[0], 2), "objects_equal": bool(same)})


if __name__ == "__main__":
    main()
