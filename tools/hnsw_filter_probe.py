#!/usr/bin/env python3
"""Filtered HNSW search (coltt_hnsw_search_filtered) on one MI355X: ms per call of WALK, EXACT and AUTO with recall@10 against EXACT, and the
post-filter baseline (an unfiltered Search for 3 k, the allowed ones kept), per allowed fraction, for a batch and for one query; plus the
filter's overhead (all-ones WALK against the unfiltered one-wave kernel at equal ef) in alternating processes.

    python tools/hnsw_filter_probe.py [--n 1000000] [--dim 768] [--quant 1] [--dataset lowrank:32:1.0] [--ef 128] [--out FILE]

WALK runs at the breadth AUTO would give it (ef_walk = min(4096, max(ef, ceil(ef * n / A)))), so WALK vs EXACT is the crossover AUTO decides.
ms = kernel time of the call (hipEvents around its launches: coltt_last_kernel_ms), median of --reps; wall = the whole call from Python.
EXACT at a large allowed count is a brute force: it runs over the first exact_nq queries only (A * exact_nq <= --exact-budget row
evaluations), which are also the queries every recall is measured on; exact_ms is per call of exact_nq queries."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRACS = (1.0, 0.5, 0.1, 0.03, 0.01, 0.001)
UNFILTERED_ONE_WAVE = {"COLTT_WALK2": "off", "COLTT_WALK2_LDS": "off", "COLTT_LAT_MAX_NQ": "0"}


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


OUT = None


def emit(row):
    line = json.dumps(row)
    print(line, flush=True)
    if OUT:
        with open(OUT, "a") as f:
            f.write(line + "\n")


def _timed(h, fn, reps):
    ms, wall, out = [], [], None
    for _ in range(reps + 1):   # the first call warms up (workspaces, the lazily allocated visited map)
        t0 = time.perf_counter(); out = fn(); w = time.perf_counter() - t0
        ms.append(h.last_kernel_ms()); wall.append(w * 1e3)
    return out, round(float(np.median(ms[1:])), 3), round(float(np.median(wall[1:])), 3)


def _recall(got, cnt, want, wcnt):
    r = []
    for i in range(len(want)):
        w = set(want[i, :wcnt[i]].tolist())
        if w:
            r.append(len(w & set(got[i, :cnt[i]].tolist())) / len(w))
    return round(float(np.mean(r)), 4) if r else None


def sweep(a):
    G, h, Q, build_s = _setup(a)
    n = h.Len(); k = a.k
    rng = np.random.default_rng(1)
    emit({"part": "setup", "n": n, "dim": a.dim, "quant": a.quant, "dataset": a.dataset, "ef": a.ef, "build_s": round(build_s, 1)})
    for frac in FRACS:
        allow = np.ones(n, bool) if frac == 1.0 else rng.random(n) < frac
        ids = np.nonzero(allow)[0].astype(np.uint64)
        with h.Filter(ids) as flt:
            A = flt.allowed
            ef = max(a.ef, k)
            ef_need = -(-ef * n // A)
            ef_walk = min(4096, max(ef, ef_need))
            for nq in (a.nq, 1):
                q = Q[:nq]
                ne = int(max(1, min(nq, a.exact_budget // max(A, 1))))
                row = {"part": "sweep", "frac": frac, "allowed": A, "nq": nq, "exact_nq": ne, "ef_walk_formula": ef_walk}
                (ei, es, ec), row["exact_ms"], row["exact_wall_ms"] = _timed(h, lambda: h.SearchFiltered(Q[:ne], k, flt, mode=G.FILTER_EXACT),
                                                                             a.reps if A * ne <= a.exact_budget // 4 else 1)
                (wi, ws, wc, wst), row["walk_ms"], row["walk_wall_ms"] = _timed(
                    h, lambda: h.SearchFiltered(q, k, flt, ef=ef_walk, mode=G.FILTER_WALK, with_stats=True), a.reps)
                row["walk_recall"] = _recall(wi[:ne], wc[:ne], ei, ec)
                row["walk_n_dist_per_query"] = round(wst["n_dist"] / nq, 1)
                (ai, as_, ac, ast), row["auto_ms"], row["auto_wall_ms"] = _timed(h, lambda: h.SearchFiltered(q, k, flt, ef=a.ef, with_stats=True), a.reps)
                row["auto_path"] = {G.FILTER_WALK: "walk", G.FILTER_EXACT: "exact"}[ast["path"]]
                row["auto_ef_walk"] = ast["ef_walk"]
                row["auto_recall"] = _recall(ai[:ne], ac[:ne], ei, ec)
                (pi, ps, pc), row["post_ms"], row["post_wall_ms"] = _timed(h, lambda: h.Search(q, 3 * k, ef=a.ef), a.reps)
                post = np.zeros((ne, k), np.uint64); postc = np.zeros(ne, np.uint32)
                for i in range(ne):
                    keep = [x for x in pi[i, :pc[i]] if allow[int(x)]][:k]
                    post[i, :len(keep)] = keep; postc[i] = len(keep)
                row["post_recall"] = _recall(post, postc, ei, ec)
                emit(row)


def overhead(a, which):
    G, h, Q, _ = _setup(a)
    n = h.Len(); ef = max(a.ef, a.k)
    res = {"part": "overhead", "which": which, "ef": ef, "nq": a.nq}
    if which == "unfiltered":
        (_, _, _, st), res["ms"], res["wall_ms"] = _timed(h, lambda: h.Search(Q, a.k, ef=ef, with_stats=True), a.reps)
    else:
        with h.Filter(np.arange(n, dtype=np.uint64)) as flt:
            (_, _, _, st), res["ms"], res["wall_ms"] = _timed(h, lambda: h.SearchFiltered(Q, a.k, flt, ef=ef, mode=G.FILTER_WALK, with_stats=True), a.reps)
    res["n_dist"] = st["n_dist"]
    emit(res)


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
    ap.add_argument("--pairs", type=int, default=3, help="alternating process pairs of the overhead measurement")
    ap.add_argument("--part", default="all", help="all | sweep | overhead:unfiltered | overhead:filtered")
    ap.add_argument("--exact-budget", type=float, default=2e8, help="row evaluations per EXACT call of the sweep (see above)")
    ap.add_argument("--out", default="", help="append every JSON line to this file as it is measured")
    a = ap.parse_args()
    global OUT
    OUT = a.out or None
    if a.part == "sweep":
        return sweep(a)
    if a.part.startswith("overhead:"):
        return overhead(a, a.part.split(":")[1])
    # parent: every measurement in a fresh child process; the overhead pairs alternate unfiltered / filtered
    base = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--dim", str(a.dim), "--quant", str(a.quant), "--dataset", a.dataset,
            "--ef", str(a.ef), "--k", str(a.k), "--nq", str(a.nq), "--reps", str(a.reps), "--exact-budget", str(a.exact_budget)]
    if a.out:
        base += ["--out", a.out]

    def run(part, env_extra):
        env = dict(os.environ); env.update(env_extra)
        r = subprocess.run(base + ["--part", part], env=env, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"{part}: exit {r.returncode}")

    run("sweep", {})
    for _ in range(a.pairs):
        run("overhead:unfiltered", UNFILTERED_ONE_WAVE)
        run("overhead:filtered", UNFILTERED_ONE_WAVE)


if __name__ == "__main__":
    main()
