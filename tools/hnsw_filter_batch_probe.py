#!/usr/bin/env python3
"""A filter per query (coltt_hnsw_search_filtered_batch) on one MI355X: 10 000 queries spread over F distinct filters, F in {1, 16, 256,
10 000}, allowed fractions mixed over 10 % / 1 % / 0.1 % (filter j at FRACS[j % 3]) so that AUTO splits the batch between the walk and the
exact scan.

    python tools/hnsw_filter_batch_probe.py [--n 1000000] [--dim 768] [--quant 1] [--dataset lowrank:32:1.0] [--ef 128] [--out FILE]

Parts (each in a fresh child process; --part selects one):
  batch     per F: the batch call (ms = kernel time, hipEvents around its launches; wall = the whole call from Python; median of --reps)
            against the sum of the equivalent one-query single-filter calls, timed over --single-sample queries and scaled to the batch
            (marked "scaled"); for F = 1 also the single-filter call on the whole batch (the cost of the per-query descriptors and of
            residency at the largest query's LDS).  Rows of the batch are checked equal to the single calls over the sample.
  launches  one batch call at F = 256 under `rocprofv3 --kernel-trace --stats`: the kernels it launched, by name.
  batcher   the C++ FilteredBatcher (tools/filter_batcher_qps.cpp, in-process), 64 caller threads each with its own filter: queries/s
            batched against the same 64 threads calling coltt_hnsw_search_filtered directly.

--pq [--pq-shape 64,32] [--rerank 768] [--parent-lib PATH]: the same batches over the walk on product-quantiser codes
(coltt_hnsw_pq_search_filtered_batch), quantiser and rerank as tools/hnsw_pq_filter_probe.py.  Per filter mix ("mixed": the fractions above;
"10pct": every filter at 10 %) and number of distinct filters F:
  pq_batch    the batch call: kernel ms, wall ms, the path mix, recall@k against the exact answer over the first --exact-nq queries
  pq_shared   one shared filter: the batch call against the single-filter call, alternating, the single call three times per pair (its own spread)
and, in a second process that loads --parent-lib through COLTT_LIB (a library from before the entry point), on the same index and filters:
  pq_singles  (a) one coltt_hnsw_pq_search_filtered call per distinct filter over that filter's queries: the sum of their kernel ms, and the wall time
  row_batch   (b) coltt_hnsw_search_filtered_batch, the row walk, with its recall"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACS = (0.1, 0.01, 0.001)
FS = (1, 16, 256, 10_000)
OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def _setup(a):
    import torch
    import coltt_amd as G
    import bench as B
    assert G.lib().coltt_init(0) == 0
    dev = torch.device("cuda", 0)

    class Args: m = 16; ef = a.ef; efc = 200; build_batch = 16384
    ds = B.Dataset(torch, dev, a.dim, a.dataset)
    t0 = time.perf_counter()
    h, _ = B.build_index(G, torch, dev, ds, a.n, a.dim, Args, 0xC0177, a.quant)
    build_s = time.perf_counter() - t0
    gen = torch.Generator(device=dev); gen.manual_seed(0x5EED5)
    q = ds.rows(a.nq, gen).cpu().numpy()
    return G, h, q, build_s


def _filters(h, n, F, seed):
    """F filters, filter j allowing about FRACS[j % 3] of the ids (drawn with repeats; a filter counts each id once)"""
    rng = np.random.default_rng(seed)
    return [h.Filter(rng.integers(0, n, int(n * FRACS[j % 3]), dtype=np.uint64)) for j in range(F)]


def _timed(h, fn, reps):
    ms, wall, out = [], [], None
    for _ in range(reps + 1):   # the first call warms up
        t0 = time.perf_counter(); out = fn(); w = time.perf_counter() - t0
        ms.append(h.last_kernel_ms()); wall.append(w * 1e3)
    return out, round(float(np.median(ms[1:])), 3), round(float(np.median(wall[1:])), 3)


def part_batch(a):
    G, h, Q, build_s = _setup(a)
    n = h.Len(); k = a.k; nq = len(Q)
    emit({"part": "setup", "n": n, "dim": a.dim, "quant": a.quant, "dataset": a.dataset, "ef": a.ef, "nq": nq, "build_s": round(build_s, 1)})
    for F in FS:
        t0 = time.perf_counter()
        flts = _filters(h, n, F, 1000 + F)
        fbuild = time.perf_counter() - t0
        rows = [flts[i % F] for i in range(nq)]
        (bi, bs, bc, bp, st), row_ms, row_wall = _timed(h, lambda: h.SearchFilteredBatch(Q, k, rows, ef=a.ef, with_stats=True), a.reps)
        row = {"part": "batch", "F": F, "nq": nq, "filters_build_s": round(fbuild, 2), "batch_ms": row_ms, "batch_wall_ms": row_wall,
               "walk_queries": int((bp == G.FILTER_WALK).sum()), "exact_queries": int((bp == G.FILTER_EXACT).sum()), "ef_walk_max": st["ef_walk"]}
        # one-query single-filter calls over a sample, scaled to the batch
        idx = np.linspace(0, nq - 1, min(nq, a.single_sample)).astype(int)
        sms, swall, same = 0.0, 0.0, True
        for i in idx:
            t1 = time.perf_counter()
            si, ss, sc = h.SearchFiltered(Q[i:i + 1], k, rows[i], ef=a.ef)
            swall += (time.perf_counter() - t1) * 1e3
            sms += h.last_kernel_ms()
            c = int(sc[0])
            same &= c == int(bc[i]) and np.array_equal(si[0, :c], bi[i, :c]) and np.array_equal(ss[0, :c].view(np.uint32), bs[i, :c].view(np.uint32))
        scale = nq / len(idx)
        row.update({"singles_sampled": len(idx), "singles_ms_scaled": round(sms * scale, 1), "singles_wall_ms_scaled": round(swall * scale, 1),
                    "speedup_kernel": round(sms * scale / row_ms, 1) if row_ms else None,
                    "speedup_wall": round(swall * scale / row_wall, 1) if row_wall else None, "rows_equal_singles": bool(same)})
        if F == 1:
            _, row["single_filter_call_ms"], row["single_filter_call_wall_ms"] = _timed(h, lambda: h.SearchFiltered(Q, k, flts[0], ef=a.ef), a.reps)
            row["batch_over_single_filter_call"] = round(row_ms / row["single_filter_call_ms"], 4)
        emit(row)
        if F == 1:   # F = 1 at each of the three fractions: the descriptor cost on either path
            for j in (1, 2):
                with h.Filter(np.random.default_rng(7 + j).integers(0, n, int(n * FRACS[j]), dtype=np.uint64)) as f1:
                    (_, _, _, bp1), b_ms, _ = _timed(h, lambda: h.SearchFilteredBatch(Q, k, [f1] * nq, ef=a.ef), a.reps)
                    _, s_ms, _ = _timed(h, lambda: h.SearchFiltered(Q, k, f1, ef=a.ef), a.reps)
                    emit({"part": "batch_f1", "frac": FRACS[j], "allowed": f1.allowed, "path": int(bp1[0]), "batch_ms": b_ms,
                          "single_filter_call_ms": s_ms, "batch_over_single_filter_call": round(b_ms / s_ms, 4)})
        for f in flts:
            f.close()


def _pq_setup(a):
    """the index of _setup with a quantiser of --pq-shape trained on its first stored rows (tools/hnsw_pq_filter_probe.py) attached"""
    G, h, Q, build_s = _setup(a)
    m, c = (int(x) for x in a.pq_shape.split(","))
    dt = np.float16 if a.quant != 0 else np.float32
    sample = h.FetchRows(0, min(h.Len(), 65536)).view(dt).astype(np.float32)
    pq = G.PQSpace(a.dim, G.PQ_EUCLIDEAN, m, c)
    pq.Fit(sample, iterations=6)
    h.PqAttach(pq)
    emit({"part": "pq_setup", "lib": os.path.basename(os.path.dirname(G.lib_path())) + "/" + os.path.basename(G.lib_path()), "n": h.Len(), "dim": a.dim,
          "quant": a.quant, "dataset": a.dataset, "ef": a.ef, "pq": [m, c], "rerank": a.rerank, "nq": len(Q), "build_s": round(build_s, 1)})
    return G, h, Q


MIXES = (("mixed", FRACS), ("10pct", (0.1,)))


def _mix_filters(h, n, F, seed, fracs):
    rng = np.random.default_rng(seed)
    return [h.Filter(rng.integers(0, n, int(n * fracs[j % len(fracs)]), dtype=np.uint64)) for j in range(F)]


def _recall(ids, cnt, eids, ecnt):
    hit = tot = 0
    for i in range(len(ecnt)):
        e = set(int(x) for x in eids[i, :ecnt[i]])
        hit += len(e & set(int(x) for x in ids[i, :cnt[i]])); tot += len(e)
    return round(hit / max(tot, 1), 4)


def part_pq(a):
    """the batch call of the library under test"""
    G, h, Q = _pq_setup(a)
    n = h.Len(); k = a.k; nq = len(Q); ne = min(nq, a.exact_nq)
    for mix, fracs in MIXES:
        for F in FS:
            flts = _mix_filters(h, n, F, 1000 + F, fracs)
            rows = [flts[i % F] for i in range(nq)]
            ei, _, ec, _ = h.SearchFilteredBatch(Q[:ne], k, rows[:ne], ef=a.ef, mode=G.FILTER_EXACT)
            (bi, bs, bc, bp, st), ms, wall = _timed(h, lambda: h.PqSearchFilteredBatch(Q, k, rows, ef=a.ef, rerank=a.rerank, with_stats=True), a.reps)
            emit({"part": "pq_batch", "mix": mix, "F": F, "nq": nq, "batch_ms": ms, "batch_wall_ms": wall, "walk_queries": int((bp == G.FILTER_WALK).sum()),
                  "exact_queries": int((bp == G.FILTER_EXACT).sum()), "ef_walk_max": st["ef_walk"], "recall": _recall(bi[:ne], bc[:ne], ei, ec), "recall_nq": ne})
            for f in flts:
                f.close()
    # one shared filter: what the per-query descriptors and the compaction cost, read against the single call's own spread
    for frac in (0.1, 0.5):
        with h.Filter(np.random.default_rng(7).integers(0, n, int(n * frac), dtype=np.uint64)) as f1:
            for pair in range(a.pairs):
                (_, _, _, bp1), b_ms, _ = _timed(h, lambda: h.PqSearchFilteredBatch(Q, k, [f1] * nq, ef=a.ef, rerank=a.rerank), a.reps)
                s_ms = [_timed(h, lambda: h.PqSearchFiltered(Q, k, f1, ef=a.ef, rerank=a.rerank), a.reps)[1] for _ in range(3)]
                med = float(np.median(s_ms))
                emit({"part": "pq_shared", "frac": frac, "allowed": f1.allowed, "pair": pair, "path": int(bp1[0]), "batch_ms": b_ms, "single_filter_call_ms": s_ms,
                      "single_spread": round((max(s_ms) - min(s_ms)) / med, 4), "batch_over_single_filter_call": round(b_ms / med, 4)})


def part_pq_parent(a):
    """the comparators, meant for a library from before the entry point (COLTT_LIB): (a) one single-filter PQ call per distinct filter, (b) the row batch"""
    G, h, Q = _pq_setup(a)
    n = h.Len(); k = a.k; nq = len(Q); ne = min(nq, a.exact_nq)
    for mix, fracs in MIXES:
        for F in FS:
            flts = _mix_filters(h, n, F, 1000 + F, fracs)
            rows = [flts[i % F] for i in range(nq)]
            ei, _, ec, _ = h.SearchFilteredBatch(Q[:ne], k, rows[:ne], ef=a.ef, mode=G.FILTER_EXACT)
            groups = [np.arange(j, nq, F) for j in range(F)]
            passes = []
            for r in range((a.reps if F <= 256 else 1) + (1 if F <= 256 else 0)):   # F <= 256: a warm-up pass, then --reps; beyond: one pass after a few warm-up calls
                if F > 256 and r == 0:
                    for j in range(8):
                        h.PqSearchFiltered(Q[groups[j]], k, flts[j], ef=a.ef, rerank=a.rerank)
                ms = 0.0; t0 = time.perf_counter()
                for j in range(F):
                    h.PqSearchFiltered(Q[groups[j]], k, flts[j], ef=a.ef, rerank=a.rerank)
                    ms += h.last_kernel_ms()
                passes.append((ms, (time.perf_counter() - t0) * 1e3))
            passes = passes[1:] if F <= 256 else passes
            emit({"part": "pq_singles", "mix": mix, "F": F, "nq": nq, "calls": F, "passes": len(passes), "kernel_ms_sum": round(float(np.median([p[0] for p in passes])), 3),
                  "wall_ms": round(float(np.median([p[1] for p in passes])), 3)})
            (ri, _, rc, rp, rst), ms, wall = _timed(h, lambda: h.SearchFilteredBatch(Q, k, rows, ef=a.ef, with_stats=True), a.reps)
            emit({"part": "row_batch", "mix": mix, "F": F, "nq": nq, "batch_ms": ms, "batch_wall_ms": wall, "walk_queries": int((rp == G.FILTER_WALK).sum()),
                  "exact_queries": int((rp == G.FILTER_EXACT).sum()), "ef_walk_max": rst["ef_walk"], "recall": _recall(ri[:ne], rc[:ne], ei, ec), "recall_nq": ne})
            for f in flts:
                f.close()


def part_launch_call(a):
    G, h, Q, _ = _setup(a)
    flts = _filters(h, h.Len(), 256, 1256)
    rows = [flts[i % 256] for i in range(len(Q))]
    h.SearchFilteredBatch(Q, a.k, rows, ef=a.ef)


def part_batcher(a):
    G, h, Q, _ = _setup(a)
    n = h.Len(); T = a.threads
    with tempfile.TemporaryDirectory() as td:
        so = os.path.join(td, "qps.so")
        libdir = os.path.dirname(G.lib_path())
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-pthread", "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "filter_batcher_qps.cpp"), "-o", so, "-L", libdir, "-lcoltt_gpu", f"-Wl,-rpath,{libdir}"])
        lib = C.CDLL(so)
        flts = _filters(h, n, T, 4242)
        fh = np.array([f.h.value for f in flts], np.uint64)
        per = max(1, min(a.per_thread, len(Q) // T))
        q = np.ascontiguousarray(Q[:T * per], np.float32)
        for batched in (0, 1, 0, 1):
            qps = C.c_double(0); nb = C.c_ulonglong(0)
            rc = lib.filter_batcher_qps(h.h, C.c_uint32(a.dim), fh.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), T, per, C.c_uint32(a.k),
                                        batched, C.byref(qps), C.byref(nb))
            emit({"part": "batcher", "mode": "batched" if batched else "direct", "threads": T, "queries": T * per, "rc": rc,
                  "qps": round(qps.value, 1), "batches": nb.value if batched else None})
        for f in flts:
            f.close()


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
    ap.add_argument("--single-sample", type=int, default=500, help="one-query calls timed per F (scaled to the batch)")
    ap.add_argument("--threads", type=int, default=64)
    ap.add_argument("--per-thread", type=int, default=100)
    ap.add_argument("--part", default="all", help="all | batch | launches | launch_call | batcher | pq | pq_parent")
    ap.add_argument("--pq", action="store_true", help="the batches over the product-quantised walk (see above) instead of the row walk's parts")
    ap.add_argument("--pq-shape", default="64,32", help="sub-vectors,centroids of the quantiser")
    ap.add_argument("--rerank", type=int, default=768)
    ap.add_argument("--exact-nq", type=int, default=300, help="queries the recall is measured on")
    ap.add_argument("--pairs", type=int, default=3, help="alternating pairs of the shared-filter measurement")
    ap.add_argument("--parent-lib", default="", help="--pq: a library from before coltt_hnsw_pq_search_filtered_batch, for the two comparators")
    ap.add_argument("--out", default="", help="append every JSON line to this file as it is measured")
    a = ap.parse_args()
    global OUT
    OUT = a.out or None
    if a.part == "batch":
        return part_batch(a)
    if a.part == "launch_call":
        return part_launch_call(a)
    if a.part == "batcher":
        return part_batcher(a)
    if a.part == "pq":
        return part_pq(a)
    if a.part == "pq_parent":
        return part_pq_parent(a)
    base = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--dim", str(a.dim), "--quant", str(a.quant), "--dataset", a.dataset,
            "--ef", str(a.ef), "--k", str(a.k), "--nq", str(a.nq), "--reps", str(a.reps), "--single-sample", str(a.single_sample),
            "--threads", str(a.threads), "--per-thread", str(a.per_thread)]
    if a.out:
        base += ["--out", a.out]

    def run(cmd, timeout=900, env=None):
        r = subprocess.run(cmd, timeout=timeout, env=env)
        if r.returncode != 0:
            raise SystemExit(f"{cmd[-1]}: exit {r.returncode}")

    if a.pq:
        pq_args = ["--pq-shape", a.pq_shape, "--rerank", str(a.rerank), "--exact-nq", str(a.exact_nq), "--pairs", str(a.pairs)]
        run(base + pq_args + ["--part", "pq"], timeout=900)
        if a.parent_lib:
            run(base + pq_args + ["--part", "pq_parent"], timeout=900, env=dict(os.environ, COLTT_LIB=os.path.abspath(a.parent_lib)))
        return

    if a.part in ("all", "launches"):
        td = tempfile.mkdtemp()
        try:
            run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "run", "--"] + [c for c in base if c != a.out and c != "--out"] + ["--part", "launch_call"], timeout=400)
            counts = {}   # kernel name -> dispatches, from the kernel trace (one row per dispatch)
            for p in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
                with open(p) as f:
                    for r in csv.DictReader(f):
                        name = r.get("Kernel_Name", "?").split("(")[0][:120]
                        counts[name] = counts.get(name, 0) + 1
            mine = {k_: v for k_, v in counts.items() if "filtered_batch" in k_ or "scan_batch" in k_ or "select_batch" in k_}
            emit({"part": "launches", "F": 256, "nq": a.nq, "batch_kernels": mine, "batch_kernel_launches": sum(mine.values()),
                  "all_kernels_in_process": sum(counts.values())})
        finally:
            shutil.rmtree(td, ignore_errors=True)
    if a.part in ("all",):
        run(base + ["--part", "batch"], timeout=1800)
    if a.part in ("all",):
        run(base + ["--part", "batcher"])


if __name__ == "__main__":
    main()
