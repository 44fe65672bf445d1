#!/usr/bin/env python3
"""The multi-vector scan for a batch of requests on one MI355X: coltt_cflat_search_batch against the same requests through one
coltt_cflat_search call each, on one store, and the time to build that store through coltt_cflat_upsert.

    python tools/cflat_batch_probe.py [--n 1000000] [--fields 3] [--dim 128] [--metric cosine] [--k 10] [--nq 1,2,8,64,256] [--reps 7] [--out FILE]

The store holds fill_normal rows under permuted ids; request i takes one of five ratio / include sets (every field; ratio 0 on one; a
ratio of 250; the middle field only; all but the first field), so a group mixes masks.  Per nq (wall ms of the call from Python, median /
min / max over --reps after one warm-up):
  batch_ms        one coltt_cflat_search_batch of nq requests
  loop_ms         the same requests through nq calls of coltt_cflat_search
  rows_gbps       ceil(nq / --width) passes over every field row of the store, in bytes per second of batch_ms (--width: the requests
                  the library serves per pass at this shape; one request per pass when nq = 1), and hbm_fraction = that over the 8 TB/s
                  peak; request_rows_gbps counts the rows once per REQUEST instead: what nq single scans at that speed would need
and the two paths' answers must be the same bits.  A library without coltt_cflat_search_batch (COLTT_LIB pointing at an older build)
gets the loop and build times only.  One JSON line per part is appended to --out (default profiles/cflat_batch_probe.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8e12


def ratio_sets(nf):
    base = [50, 30, 20, 45, 5, 60, 10, 80][:nf]
    ones = [1] * nf
    zero = list(base); zero[nf - 1] = 0
    big = list(base); big[0] = 250
    one = [0] * nf; one[nf // 2] = 1
    rest = [1] * nf; rest[0] = 0 if nf > 1 else 1
    return [(base, ones), (zero, ones), (big, ones), (base, one), (base, rest)]


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--fields", type=int, default=3)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--metric", default="cosine", choices=["cosine", "l2"])
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", default="1,2,8,64,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=16, help="requests per pass over the rows of the library probed, at this shape")
    ap.add_argument("--label", default="", help="free text kept in every record (which library this is)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cflat_batch_probe.jsonl"))
    a = ap.parse_args()
    assert a.reps >= 5
    import coltt_amd as G
    from oracle import oracle as O
    L = G.lib()
    assert L.coltt_init(0) == 0
    has_batch = hasattr(L, "coltt_cflat_search_batch")
    nf, dim, n, k = a.fields, a.dim, a.n, a.k
    nqs = [int(x) for x in a.nq.split(",")]

    def emit(rec):
        rec = dict({"probe": "cflat_batch", "label": a.label, "lib": os.path.basename(os.path.dirname(G.lib_path())), "n": n, "fields": nf, "dim": dim,
                    "metric": a.metric, "k": k}, **rec)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    X = O.fill_normal(0xCF1A7, (n, nf, dim))
    ids = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(11)) % np.uint64(1 << 40)
    s = G.MultiVectorSpace(dim, nf, G.COSINE if a.metric == "cosine" else G.EUCLIDEAN)
    t0 = time.perf_counter(); s.ChangedVertex(ids, X); build_s = time.perf_counter() - t0
    assert s.Len() == n
    emit({"part": "build", "build_s": round(build_s, 3), "rows_per_s": round(n / build_s, 1)})
    del X

    sets = ratio_sets(nf)
    Q = O.fill_normal(0xCF1A8, (max(nqs), nf, dim))
    R = np.array([sets[i % 5][0] for i in range(max(nqs))], np.uint32); INC = np.array([sets[i % 5][1] for i in range(max(nqs))], np.uint8)
    row_bytes = n * nf * dim * 4

    def loop(nq):
        return [s.MultiVertexSearch(k, Q[i], R[i], INC[i]) for i in range(nq)]

    for nq in nqs:
        rec = {"part": "search", "nq": nq, "reps": a.reps}
        want = loop(nq)                                   # warm-up of the loop, and the answer the batch must reproduce
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); loop(nq); ts.append((time.perf_counter() - t0) * 1e3)
        rec["loop_ms"] = stats(ts)
        if has_batch:
            gi, gs, gc = s.MultiVertexSearchBatch(k, Q[:nq], R[:nq], INC[:nq])        # warm-up
            for i in range(nq):
                wi, ws, wc = want[i]
                assert gc[i] == wc[0] and np.array_equal(gi[i], wi[0]) and np.array_equal(gs[i].view(np.uint32), ws[0].view(np.uint32)), f"nq {nq} request {i}: the batch differs"
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter(); s.MultiVertexSearchBatch(k, Q[:nq], R[:nq], INC[:nq]); ts.append((time.perf_counter() - t0) * 1e3)
            rec["batch_ms"] = stats(ts)
            rec["identical_bits"] = True
            sec = rec["batch_ms"]["median"] * 1e-3
            passes = -(-nq // a.width)
            rec["width"] = a.width; rec["passes"] = passes
            rec["rows_gbps"] = round(passes * row_bytes / sec / 1e9, 1); rec["hbm_fraction"] = round(passes * row_bytes / sec / HBM_PEAK, 4)
            rec["request_rows_gbps"] = round(nq * row_bytes / sec / 1e9, 1)
            rec["speedup_median"] = round(rec["loop_ms"]["median"] / rec["batch_ms"]["median"], 2)
            rec["batch_beats_loop_beyond_spread"] = rec["batch_ms"]["max"] < rec["loop_ms"]["min"]
        emit(rec)
    s.close()


if __name__ == "__main__":
    main()
