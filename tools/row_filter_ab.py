#!/usr/bin/env python3
"""A/B of the certified level-0 row filter on ONE index in ONE process: filter off, over the binary16 shadow (row_filter.hpp), over the 8-bit
shadow with the f32 query (row_filter8.hpp) and with the quantised query (row_filter8i.hpp: integer phase A) — that last kind over the 32-bit LDS visited
table (side "8i": COLTT_VIS16=0, four traversals per CU) and over the 16-bit one (vis16.hpp; side "8i-v16": seven per CU, and "8i-v16-w4" .. "-w6": the same
binary held to 4 / 5 / 6 per CU by COLTT_WAVES_PER_CU; per side the visited set's report of the last launch: kind, traversals per CU, the fullest stash and
the most vertices one traversal visited).  The index is created with
COLTT_ROW_SHADOW_BITS=both; per call COLTT_ROW_FILTER=0 / 1 and COLTT_ROW_FILTER_BITS=16 / 8 / 8i pick the side, calls alternating.  `python tools/row_filter_ab.py [n] [ef,ef,...] [rounds]` builds n x 768 f32 cosine with the batched builder (ROW_FILTER_AB_DIM for
another dim), then per ef runs 10 000 queries `rounds` times per side (kernel time from the hipEvent pair on the search stream; the first round of each
side is a warm-up), checks np.array_equal on ids, score bits, counts and the three traversal counters across the sides, and prints one JSON line: per side
ms per launch (all values and the median), shadow rows / survivors / f32 rows per query, and the bytes the side REQUESTS per query
    shadow rows x shadow row bytes + f32 rows x dim x 4 + n_exp x (128 + 128 + 256) + n_dist x 4
(one adjacency row, its norms and its (scale, error norm) pairs per expansion — the same formula on every side, although only the 8-bit side reads the
last 256 bytes: 0.5 % of the total; a neighbour the shadow cannot reject reads its shadow row AND its f32 row; f32 rows = every evaluation on the
unfiltered side) as a fraction of the 8 TB/s peak.  Requested bytes
from counters, not a FETCH_SIZE measurement.  COLTT_ROW_FILTER=1 also forces the ef > 128 twins, which the default leaves off."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V16 = "8i-v16"
SIDES = (("off", "0", None, {}), ("16", "1", "16", {}), ("8", "1", "8", {}), ("8i", "1", "8i", {"COLTT_VIS16": "0"}), (V16, "1", "8i", {}),
         (V16 + "-w4", "1", "8i", {"COLTT_WAVES_PER_CU": "4"}), (V16 + "-w5", "1", "8i", {"COLTT_WAVES_PER_CU": "5"}), (V16 + "-w6", "1", "8i", {"COLTT_WAVES_PER_CU": "6"}))


def main():
    os.environ["COLTT_ROW_SHADOW_BITS"] = "both"
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
    st0 = h.RowFilterStats()
    res = {"n": n, "dim": dim, "build_s": build_s, "shadow": st0["shadow"], "shadow_bits": list(st0["shadow_bits"]), "ef": {}}
    assert tuple(st0["shadow_bits"]) == (8, 16), "the four-sided A/B needs an index that keeps both shadows"
    for ef in efs:
        ms = {s[0]: [] for s in SIDES}; keep = {}; flt = {}; vis = {}
        for r in range(rounds):
            for name, on, bits_, extra in SIDES:   # alternating: drift of the box hits every side alike
                os.environ["COLTT_ROW_FILTER"] = on
                for kk in ("COLTT_VIS16", "COLTT_WAVES_PER_CU"):
                    os.environ.pop(kk, None)
                os.environ.update(extra)
                if bits_:
                    os.environ["COLTT_ROW_FILTER_BITS"] = bits_
                else:
                    os.environ.pop("COLTT_ROW_FILTER_BITS", None)
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
                flt[name] = {kk: s1[kk] - s0[kk] for kk in ("rejected", "f32_rows", "shadow_rows", "launches")}
        for kk in ("COLTT_ROW_FILTER", "COLTT_ROW_FILTER_BITS", "COLTT_VIS16", "COLTT_WAVES_PER_CU"):
            os.environ.pop(kk, None)
        a = keep["off"]
        same = all(bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and a[3] == b[3]
                        and (a[2] is None or np.array_equal(a[2], b[2]))) for b in (keep[s_[0]] for s_ in SIDES[1:]))
        nd, ne = a[3]["n_dist"] / nq, a[3]["n_exp"] / nq
        row = {"identical": same, "per_query": {"n_dist": nd, "n_exp": ne}}
        for name, on, bits_, extra in SIDES:
            t = float(np.median(ms[name])) / 1e3
            rej, f32, sh = flt[name]["rejected"] / nq, flt[name]["f32_rows"] / nq, flt[name]["shadow_rows"] / nq
            # f32 rows: level 0 (the counter) + the upper levels' and the entrypoint's evaluations = every evaluation the filter did not reject
            f32_all, sh_bytes = nd - rej, 0 if name == "off" else dim * (2 if name == "16" else 1)
            moved = sh * sh_bytes + f32_all * dim * 4 + ne * (128 + 128 + 256) + nd * 4
            row[name] = {"ms_per_launch": t * 1e3, "min_ms": float(min(ms[name])), "max_ms": float(max(ms[name])), "all_ms": [float(x) for x in ms[name]], "queries_per_s": nq / t,
                         "shadow_rows": sh, "rejected": rej, "survivors_reading_both": sh - rej, "f32_rows_level0": f32, "f32_rows_while_filling": f32 - (sh - rej),
                         "f32_fraction_of_level0": f32 / max(rej + f32, 1e-9) if name != "off" else 1.0,
                         "bytes_requested_per_query": moved, "frac_of_hbm_peak_requested": moved * nq / t / 8e12, "filter_counters_of_last_call": flt[name], "visited_set_of_last_call": vis[name]}
        for name in [s_[0] for s_ in SIDES[1:]]:
            row[name]["speedup_over_off"] = row["off"]["ms_per_launch"] / row[name]["ms_per_launch"]
            row[name]["bytes_ratio_to_off"] = row[name]["bytes_requested_per_query"] / row["off"]["bytes_requested_per_query"]
        row["speedup_8_over_16"] = row["16"]["ms_per_launch"] / row["8"]["ms_per_launch"]
        row["speedup_8i_over_8"] = row["8"]["ms_per_launch"] / row["8i"]["ms_per_launch"]
        row["shadow_rows_equal_8_8i"] = flt["8"]["shadow_rows"] == flt["8i"]["shadow_rows"]
        row["speedup_v16_over_8i"] = row["8i"]["ms_per_launch"] / row[V16]["ms_per_launch"]
        row["filter_counters_equal_8i_v16"] = all(flt[s_[0]] == flt["8i"] for s_ in SIDES[4:])
        res["ef"][str(ef)] = row
        print(json.dumps({str(ef): row}), file=sys.stderr, flush=True)
        assert same, "the sides disagree"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
