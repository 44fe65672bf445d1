#!/usr/bin/env python3
"""Filtered search over the product-quantised walk (coltt_hnsw_pq_search_filtered) on one MI355X, on the collection of
tools/hnsw_filter_probe.py (same builder, same seeds, same queries): per allowed fraction, kernel ms per call and recall@10 against EXACT of
  row_walk   the row walk's filtered WALK (coltt_hnsw_search_filtered) at ef_walk — re-taken in this process
  pq_walk    the filtered WALK over the quantiser's codes at the same ef_walk, re-rank of --rerank
  exact      EXACT
  post       a post-filtered PqSearch: at the call's ef for 3 k candidates, and at ef_walk for its whole re-ranked result set
and the filter's overhead: an all-ones PqSearchFiltered(WALK) against PqSearch at ef 128 and ef 1 344, alternating in ONE process.

    python tools/hnsw_pq_filter_probe.py [--n 1000000] [--dim 768] [--quant 1] [--dataset lowrank:32:1.0] [--ef 128] [--pq 64,32] [--rerank 768] [--out FILE]

ms = kernel time of the call (coltt_last_kernel_ms), median of --reps after a warm-up call.  EXACT at a large allowed count runs over the
first exact_nq queries only (hnsw_filter_probe.py), which are the queries every recall is measured on."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hnsw_filter_probe as FP   # noqa: E402

FRACS = (1.0, 0.5, 0.1, 0.03, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--quant", type=int, default=1)
    ap.add_argument("--dataset", default="lowrank:32:1.0")
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=3, help="alternating pairs of the overhead measurement")
    ap.add_argument("--pq", default="64,32", help="sub-vectors,centroids of the quantiser")
    ap.add_argument("--rerank", type=int, default=768)
    ap.add_argument("--exact-budget", type=float, default=2e8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    FP.OUT = a.out or None
    emit, timed, recall = FP.emit, FP._timed, FP._recall
    G, h, Q, build_s = FP._setup(a)
    n = h.Len(); k = a.k
    m, c = (int(x) for x in a.pq.split(","))
    dt = np.float16 if a.quant != 0 else np.float32
    sample = h.FetchRows(0, min(n, 65536)).view(dt).astype(np.float32)     # the first stored rows as the index's distance sees them
    pq = G.PQSpace(a.dim, G.PQ_EUCLIDEAN, m, c)
    t0 = time.time(); pq.Fit(sample, iterations=6); fit_s = time.time() - t0
    t0 = time.time(); h.PqAttach(pq); attach_s = time.time() - t0
    emit({"part": "setup", "n": n, "dim": a.dim, "quant": a.quant, "dataset": a.dataset, "ef": a.ef, "pq": [m, c], "rerank": a.rerank,
          "build_s": round(build_s, 1), "fit_s": round(fit_s, 1), "attach_s": round(attach_s, 1)})
    rng = np.random.default_rng(1)
    for frac in FRACS:
        allow = np.ones(n, bool) if frac == 1.0 else rng.random(n) < frac
        with h.Filter(np.nonzero(allow)[0].astype(np.uint64)) as flt:
            A = flt.allowed
            ef = max(a.ef, k)
            ef_walk = min(4096, max(ef, -(-ef * n // A)))
            ne = int(max(1, min(a.nq, a.exact_budget // max(A, 1))))
            row = {"part": "sweep", "frac": frac, "allowed": A, "nq": a.nq, "exact_nq": ne, "ef_walk": ef_walk, "rows_per_ef": round(A / ef_walk, 1)}
            (ei, es, ec), row["exact_ms"], _ = timed(h, lambda: h.SearchFiltered(Q[:ne], k, flt, mode=G.FILTER_EXACT), a.reps if A * ne <= a.exact_budget // 4 else 1)
            row["exact_ms_per_10k"] = round(row["exact_ms"] * a.nq / ne, 1)
            (wi, _, wc, wst), row["row_walk_ms"], _ = timed(h, lambda: h.SearchFiltered(Q, k, flt, ef=ef_walk, mode=G.FILTER_WALK, with_stats=True), a.reps)
            row["row_walk_recall"] = recall(wi[:ne], wc[:ne], ei, ec)
            (pi, _, pc, pst), row["pq_walk_ms"], _ = timed(h, lambda: h.PqSearchFiltered(Q, k, flt, ef=ef_walk, rerank=a.rerank, mode=G.FILTER_WALK, with_stats=True), a.reps)
            row["pq_walk_recall"] = recall(pi[:ne], pc[:ne], ei, ec)
            row["pq_walk_exact_rows_per_query"] = round(pst["n_exact_rows"] / a.nq, 1)
            row["pq_walk_n_dist_per_query"] = round(pst["n_dist"] / a.nq, 1)
            (_, _, _, ast) = h.PqSearchFiltered(Q[:8], k, flt, ef=a.ef, rerank=a.rerank, with_stats=True)
            row["auto_path"] = {G.FILTER_WALK: "walk", G.FILTER_EXACT: "exact"}[ast["path"]]
            for tag, pef, pk in (("post_ef", ef, 3 * k), ("post_efwalk", ef_walk, min(ef_walk, max(a.rerank, k)))):
                (qi, _, qc), row[tag + "_ms"], _ = timed(h, lambda: h.PqSearch(Q, pk, ef=pef, rerank=a.rerank), a.reps)
                post = np.zeros((ne, k), np.uint64); postc = np.zeros(ne, np.uint32)
                for i in range(ne):
                    keep = [x for x in qi[i, :qc[i]] if allow[int(x)]][:k]
                    post[i, :len(keep)] = keep; postc[i] = len(keep)
                row[tag + "_recall"] = recall(post, postc, ei, ec)
            emit(row)
    # the filter's overhead, alternating in this process
    with h.Filter(np.arange(n, dtype=np.uint64)) as flt:
        for ef in (128, 1344):
            for pair in range(a.pairs):
                (_, _, _, st), ms_u, _ = timed(h, lambda: h.PqSearch(Q, k, ef=ef, rerank=a.rerank, with_stats=True), a.reps)
                (_, _, _, fst), ms_f, _ = timed(h, lambda: h.PqSearchFiltered(Q, k, flt, ef=ef, rerank=a.rerank, mode=G.FILTER_WALK, with_stats=True), a.reps)
                emit({"part": "overhead", "ef": ef, "pair": pair, "nq": a.nq, "pq_search_ms": ms_u, "pq_search_filtered_ms": ms_f, "ratio": round(ms_f / ms_u, 4),
                      "n_dist_equal": st["n_dist"] == fst["n_dist"]})


if __name__ == "__main__":
    main()
