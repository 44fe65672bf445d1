#!/usr/bin/env python3
"""A/B of the row-filter walk's DESCENT on ONE index in ONE process, four sides, calls alternating: the upper levels exact or through the certified
filter (COLTT_ROW_FILTER_UPPER=0 / 1) x the entrypoint's and the descent's rows with the launch's non-temporal hint or cacheable (COLTT_DESCENT_NT=1 / 0).
Everything else is the headline launch (8-bit shadow, quantised query, 16-bit visited set).  `python tools/descent_filter_ab.py [n] [ef,ef,...] [rounds]
[queries]` builds n x 768 f32 cosine with the batched builder as tools/row_filter_ab.py does, runs `queries` (10 000) queries `rounds` times per side
(kernel time from the hipEvent pair on the search stream; the first round of each side is a warm-up), checks np.array_equal on ids, score bits, counts
and the traversal counters across the sides and equality of the level-0 filter counters, and prints one JSON line: per side ms per launch (all values,
median), the descent's counters per query and the bytes the descent REQUESTS per query
    exact: (1 + evaluations above level 0) x dim x 4          filtered: dim x 4 + shadow rows x dim + f32 rows x dim x 4
(requested bytes from counters, not a FETCH_SIZE measurement).  A -DCOLTT_PHASE_TIMING build prints its phase clock per call on stderr."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIDES = (("exact-nt", "0", "1"), ("exact-cached", "0", "0"), ("filtered-nt", "1", "1"), ("filtered-cached", "1", "0"))
L0 = ("rejected", "f32_rows", "shadow_rows", "launches")
UP = ("upper_shadow_rows", "upper_rejected", "upper_f32_rows", "upper_launches")


def main():
    import torch
    import coltt_amd as G
    import bench as B
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    efs = [int(e) for e in (sys.argv[2] if len(sys.argv) > 2 else "128").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    nq = int(sys.argv[4]) if len(sys.argv) > 4 else 10_000
    dim = int(os.environ.get("ROW_FILTER_AB_DIM", "768")); k = 10
    assert G.lib().coltt_init(0) == 0
    dev = torch.device("cuda", 0)

    class A: m = 16; ef = 128; efc = 200; build_batch = 16384; reserve = True
    ds = B.Dataset(torch, dev, dim, "normal")
    h, build_s = B.build_index(G, torch, dev, ds, n, dim, A, 0xC0177, 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0x5EED5)
    q = ds.rows(nq, gen)
    out = B.Out(torch, dev, nq, k)
    res = {"n": n, "dim": dim, "queries": nq, "build_s": build_s, "shadow_bits": list(h.RowFilterStats()["shadow_bits"]), "ef": {}}
    for ef in efs:
        ms = {s[0]: [] for s in SIDES}; keep = {}; flt = {}; vis = {}
        for r in range(rounds):
            for name, up, dnt in SIDES:   # alternating: drift of the box hits every side alike
                os.environ["COLTT_ROW_FILTER_UPPER"] = up; os.environ["COLTT_DESCENT_NT"] = dnt
                s0 = h.RowFilterStats()
                st = h.SearchDevice(q.data_ptr(), nq, k, *out.ptrs(), ef=ef)
                s1 = h.RowFilterStats()
                vis[name] = h.VisitedStats()
                if r:
                    ms[name].append(h.last_kernel_ms())
                got = (out.ids.cpu().numpy().copy(), out.sc.cpu().numpy().copy(), out.cnt.cpu().numpy().copy() if hasattr(out, "cnt") else None,
                       {kk: st[kk] for kk in ("n_dist", "n_exp", "n_hops")})
                if name not in keep:
                    keep[name] = got
                else:   # every round of a side answers alike
                    assert np.array_equal(keep[name][0], got[0]) and np.array_equal(keep[name][1].view(np.uint32), got[1].view(np.uint32)) and keep[name][3] == got[3]
                flt[name] = {kk: s1[kk] - s0[kk] for kk in L0 + UP}
        for kk in ("COLTT_ROW_FILTER_UPPER", "COLTT_DESCENT_NT"):
            os.environ.pop(kk, None)
        a = keep[SIDES[0][0]]
        same = all(bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[3] == b[3]
                        and (a[2] is None or np.array_equal(a[2], b[2]))) for b in (keep[s_[0]] for s_ in SIDES[1:]))
        l0_same = all({kk: flt[s_[0]][kk] for kk in L0} == {kk: flt[SIDES[0][0]][kk] for kk in L0} for s_ in SIDES[1:])
        up_evals = flt["filtered-nt"]["upper_shadow_rows"] / nq   # every valid neighbour above level 0 reads its shadow row
        row = {"identical": same, "level0_filter_counters_equal": l0_same, "per_query": {"n_dist": a[3]["n_dist"] / nq, "n_exp": a[3]["n_exp"] / nq, "n_hops": a[3]["n_hops"] / nq,
                                                                                     "evaluations_above_level0": up_evals}}
        for name, up, dnt in SIDES:
            t = float(np.median(ms[name]))
            f = flt[name]
            sh, rej, f32 = f["upper_shadow_rows"] / nq, f["upper_rejected"] / nq, f["upper_f32_rows"] / nq
            req = dim * 4 + (sh * dim + f32 * dim * 4 if up == "1" else up_evals * dim * 4)
            row[name] = {"ms_per_launch": t, "min_ms": float(min(ms[name])), "max_ms": float(max(ms[name])), "all_ms": [float(x) for x in ms[name]], "queries_per_s": nq / t * 1e3,
                         "descent_shadow_rows": sh, "descent_rejected": rej, "descent_f32_rows": f32, "descent_bytes_requested_per_query": req,
                         "filter_counters_of_last_call": f, "visited_set_of_last_call": vis[name]}
        base = row["exact-nt"]["ms_per_launch"]
        for name, _, _ in SIDES[1:]:
            row[name]["speedup_over_exact_nt"] = base / row[name]["ms_per_launch"]
        res["ef"][str(ef)] = row
        print(json.dumps({str(ef): row}), file=sys.stderr, flush=True)
        assert same and l0_same, "the sides disagree"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
