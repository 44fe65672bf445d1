#!/usr/bin/env python3
"""What a write costs the product-quantised walk on one MI355X: single Inserts and Removes interleaved with one-query searches (the reference's call
shape: one vector per Insert RPC between Search RPCs), with the writers patching the neighbourhood blocks (default) and with COLTT_PQ_NBR_PATCH=0
(a write marks them stale, the next walk rebuilds all of them — the behaviour before the writers' patch), alternating per round in ONE process on ONE
index, on the collection of tools/hnsw_filter_probe.py (same builder, same seeds), Reserve'd for everything the probe adds.

    python tools/pq_mut_probe.py [--n 1000000] [--dim 768] [--quant 1] [--dataset lowrank:32:1.0] [--pq 64,32] [--ef 1152] [--rounds 200] [--out FILE]

Per side (wall ms of the call from Python, medians over --rounds):
  insert_ms                 one coltt_hnsw_insert
  search_after_insert_ms    the first one-query PqSearch after it
  remove_ms                 one coltt_hnsw_remove
  search_after_remove_ms    the first one-query PqSearch after it
and once: quiescent_search_ms, the same one-query PqSearch with no write in between; builds / patches / patched_rows per side from
coltt_hnsw_pq_nbr_stats.  Every sample is written too ("part": "samples")."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import hnsw_filter_probe as FP   # noqa: E402


def _ms(fn):
    t0 = time.perf_counter(); fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--quant", type=int, default=1)
    ap.add_argument("--dataset", default="lowrank:32:1.0")
    ap.add_argument("--ef", type=int, default=1152)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--pq", default="64,32", help="sub-vectors,centroids of the quantiser")
    ap.add_argument("--rerank", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--no-pq", action="store_true", help="no quantiser: only the latency of single Inserts / Removes on an index that keeps no blocks")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    FP.OUT = a.out or None
    emit = FP.emit
    import torch
    import coltt_amd as G
    import bench as B
    assert G.lib().coltt_init(0) == 0
    dev = torch.device("cuda", 0)
    extra = 2 * a.rounds + 64

    class Args: m = 16; ef = 128; efc = 200; build_batch = 16384; reserve = False
    ds = B.Dataset(torch, dev, a.dim, a.dataset)
    h = G.Hnsw(a.dim, G.COSINE, G.HnswCfg.default(m=Args.m, ef=Args.ef, ef_construction=Args.efc), quantization=a.quant)
    h.Reserve(a.n + extra)                                       # the writes below never grow the arrays: the blocks stay patchable
    t0 = time.perf_counter(); B.build_index(G, torch, dev, ds, a.n, a.dim, Args, 0xC0177, a.quant, h=h); build_s = time.perf_counter() - t0
    gen = torch.Generator(device=dev); gen.manual_seed(0x5EED5)
    Q = ds.rows(64, gen).cpu().numpy()
    new = ds.rows(extra, gen).cpu().numpy()                       # the vectors the probe inserts
    levels = B.draw_levels(extra, Args.m, 0xA11)
    rng = np.random.default_rng(3)
    victims = rng.choice(a.n, extra, replace=False)
    setup = {"part": "setup", "n": a.n, "dim": a.dim, "quant": a.quant, "dataset": a.dataset, "ef": a.ef, "rounds": a.rounds, "build_s": round(build_s, 1)}
    if a.no_pq:
        emit(setup)
        ins, rem = [], []
        for r in range(2 * a.rounds):
            ins.append(_ms(lambda: h.Insert(a.n + r, new[r], int(levels[r]))))
            rem.append(_ms(lambda: h.Remove(int(victims[r]))))
        emit({"part": "no_pq", "insert_ms": round(float(np.median(ins)), 4), "remove_ms": round(float(np.median(rem)), 4),
              "insert_ms_p10_p90": [round(float(np.percentile(ins, p)), 4) for p in (10, 90)], "samples": len(ins)})
        return
    m, c = (int(x) for x in a.pq.split(","))
    dt = np.float16 if a.quant != 0 else np.float32
    pq = G.PQSpace(a.dim, G.PQ_EUCLIDEAN, m, c)
    pq.Fit(h.FetchRows(0, min(a.n, 65536)).view(dt).astype(np.float32), iterations=6)
    h.PqAttach(pq)
    search = lambda i: h.PqSearch(Q[i % len(Q)], a.k, ef=a.ef, rerank=a.rerank)   # noqa: E731
    for i in range(8):
        search(i)                                                 # the whole build, workspaces, the visited map
    st = h.PqNbrStats()
    setup.update({"pq": [m, c], "rerank": a.rerank, "state_after_first_walks": st["state"], "block_bytes": a.n * h.cfg.m_max0 * ((m + 15) & ~15)})
    emit(setup)
    if st["state"] != 1:
        emit({"part": "error", "what": "the index keeps no neighbourhood blocks (not affordable?): nothing to compare"})
        return
    quiet = [_ms(lambda: search(i)) for i in range(a.rounds)]
    samples = {s: {k_: [] for k_ in ("insert_ms", "search_after_insert_ms", "remove_ms", "search_after_remove_ms")} for s in ("0", "1")}
    counts = {s: {"builds": 0, "patches": 0, "patched_rows": 0} for s in ("0", "1")}
    w = 0
    for r in range(a.rounds):
        for side in ("0", "1"):
            os.environ["COLTT_PQ_NBR_PATCH"] = side              # the binding sees the change and calls coltt_policy_reload before the next call
            before = h.PqNbrStats()
            s = samples[side]
            s["insert_ms"].append(_ms(lambda: h.Insert(a.n + w, new[w], int(levels[w]))))
            s["search_after_insert_ms"].append(_ms(lambda: search(w)))
            s["remove_ms"].append(_ms(lambda: h.Remove(int(victims[w]))))
            s["search_after_remove_ms"].append(_ms(lambda: search(w + 1)))
            after = h.PqNbrStats()
            for k_ in counts[side]:
                counts[side][k_] += after[k_] - before[k_]
            w += 1
    del os.environ["COLTT_PQ_NBR_PATCH"]
    quiet += [_ms(lambda: search(i)) for i in range(a.rounds)]
    q_ms = float(np.median(quiet))
    emit({"part": "quiescent", "search_ms": round(q_ms, 4), "p10_p90": [round(float(np.percentile(quiet, p)), 4) for p in (10, 90)], "samples": len(quiet)})
    for side in ("0", "1"):
        row = {"part": "side", "COLTT_PQ_NBR_PATCH": int(side), "rounds": a.rounds}
        for k_, v in samples[side].items():
            row[k_] = round(float(np.median(v)), 4)
        row["search_after_insert_over_quiescent"] = round(row["search_after_insert_ms"] / q_ms, 4)
        row["search_after_remove_over_quiescent"] = round(row["search_after_remove_ms"] / q_ms, 4)
        row.update(counts[side])
        emit(row)
    for side in ("0", "1"):
        emit({"part": "samples", "COLTT_PQ_NBR_PATCH": int(side), **{k_: [round(x, 4) for x in v] for k_, v in samples[side].items()}})
    emit({"part": "samples", "quiescent_search_ms": [round(x, 4) for x in quiet]})


if __name__ == "__main__":
    main()
