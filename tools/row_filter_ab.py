#!/usr/bin/env python3
"""A/B of the certified level-0 row filter (coltt_amd/csrc/row_filter.hpp) on ONE index in ONE process: COLTT_ROW_FILTER=0 against 1, calls
alternating.  `python tools/row_filter_ab.py [n] [ef,ef,...] [rounds]` builds n x 768 f32 cosine with the batched builder (ROW_FILTER_AB_DIM for
another dim), then per ef runs 10 000 queries `rounds` times per variant (kernel time from the hipEvent pair on the search stream; the first
round of each variant is a warm-up), checks np.array_equal on ids, score bits, counts and the three traversal counters, and prints one JSON line:
ms per launch for both, the filter's counters, and the bytes each variant really moves per query
(shadow rows * dim * 2 + (n_dist - rejected) * dim * 4 + n_exp * 128 + n_dist * 4 against n_dist * dim * 4 + ...: a neighbour the shadow cannot
reject reads its shadow row AND its f32 row).  COLTT_ROW_FILTER=1 also forces the ef > 128 twins, which the default leaves off."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import coltt_amd as G
    import bench as B
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    efs = [int(e) for e in (sys.argv[2] if len(sys.argv) > 2 else "128").split(",")]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    dim = int(os.environ.get("ROW_FILTER_AB_DIM", "768")); k, nq = 10, 10_000
    assert G.lib().coltt_init(0) == 0
    dev = torch.device("cuda", 0)

    class A: m = 16; ef = 128; efc = 200; build_batch = 16384; reserve = True
    ds = B.Dataset(torch, dev, dim, "normal")
    h, build_s = B.build_index(G, torch, dev, ds, n, dim, A, 0xC0177, 0)
    gen = torch.Generator(device=dev); gen.manual_seed(0x5EED5)
    q = ds.rows(nq, gen)
    out = B.Out(torch, dev, nq, k)
    res = {"n": n, "dim": dim, "build_s": build_s, "shadow": h.RowFilterStats()["shadow"], "ef": {}}
    for ef in efs:
        ms = {"0": [], "1": []}; keep = {}; flt = {}
        for r in range(rounds):
            for v in ("0", "1"):   # alternating: drift of the box hits both variants alike
                os.environ["COLTT_ROW_FILTER"] = v
                s0 = h.RowFilterStats()
                st = h.SearchDevice(q.data_ptr(), nq, k, *out.ptrs(), ef=ef)
                s1 = h.RowFilterStats()
                if r:
                    ms[v].append(h.last_kernel_ms())
                got = (out.ids.cpu().numpy().copy(), out.sc.cpu().numpy().copy(), out.cnt.cpu().numpy().copy() if hasattr(out, "cnt") else None,
                       {kk: st[kk] for kk in ("n_dist", "n_exp", "n_hops")})
                if v not in keep:
                    keep[v] = got
                else:   # every round of a variant answers alike
                    assert np.array_equal(keep[v][0], got[0]) and np.array_equal(keep[v][1].view(np.uint32), got[1].view(np.uint32)) and keep[v][3] == got[3]
                flt[v] = {kk: s1[kk] - s0[kk] for kk in ("rejected", "f32_rows", "shadow_rows", "launches")}
        os.environ.pop("COLTT_ROW_FILTER", None)
        a, b = keep["0"], keep["1"]
        same = bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[3] == b[3]
                    and (a[2] is None or np.array_equal(a[2], b[2])))
        nd, ne = a[3]["n_dist"] / nq, a[3]["n_exp"] / nq
        rej, f32, h16 = flt["1"]["rejected"] / nq, flt["1"]["f32_rows"] / nq, flt["1"]["shadow_rows"] / nq
        row = {"identical": same, "per_query": {"n_dist": nd, "n_exp": ne, "rejected": rej, "f32_rows_level0": f32, "shadow_rows": h16, "survivors_reading_both": h16 - rej, "f32_rows_while_filling": f32 - (h16 - rej),
                                                "f32_fraction_of_level0": f32 / max(rej + f32, 1e-9)}}
        for v, name in (("0", "unfiltered"), ("1", "filtered")):
            t = float(np.median(ms[v])) / 1e3
            moved = (nd * dim * 4 if v == "0" else h16 * dim * 2 + (nd - rej) * dim * 4) + ne * 128 + nd * 4
            row[name] = {"ms_per_launch": t * 1e3, "min_ms": float(min(ms[v])), "max_ms": float(max(ms[v])), "all_ms": [float(x) for x in ms[v]], "queries_per_s": nq / t,
                         "bytes_moved_per_query": moved, "frac_of_hbm_peak_really_drawn": moved * nq / t / 8e12, "filter_counters_of_last_call": flt[v]}
        row["speedup"] = row["unfiltered"]["ms_per_launch"] / row["filtered"]["ms_per_launch"]
        row["bytes_ratio"] = row["filtered"]["bytes_moved_per_query"] / row["unfiltered"]["bytes_moved_per_query"]
        res["ef"][str(ef)] = row
        print(json.dumps({str(ef): row}), file=sys.stderr, flush=True)
        assert same, "the filtered and the unfiltered walk disagree"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
