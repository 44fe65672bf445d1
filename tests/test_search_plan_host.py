"""The search plan without a device: coltt_hnsw_search_plan_host — the function coltt_hnsw_search itself decides by — against the answers the commit
before it gave (tests/golden/search_plan.npz: recorded through a shim over that commit's search_geom / resident_waves / rows_nt / row_filter_on /
row_filter_bits, its latency-kernel block and its kernel-selection nest; profiles/search_plan_kernels.md; the sweep is tools/search_plan_sweep.py).

The fixture holds no row with the message "... has no instance for line-transposed rows": in the recorded code that check stood behind "walk variant %d
is not compiled into this build" and its condition implied the first one's, so no input reaches it (309 750 rows, COLTT_WALK2 / COLTT_WALK2_LDS at every
value, with and without line-transposed rows: 4 244 rows of the first message, none of the second).  The plan keeps the reachable one."""
import os
import sys

import numpy as np
import pytest

import coltt_amd
from coltt_amd import hnsw as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import search_plan_sweep as S  # noqa: E402

E_INVALID, E_UNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def sweep():
    knobs, inp, want = S.load(os.path.join(ROOT, "tests", "golden", "search_plan.npz"))
    got = S.run_library(inp, knobs)
    return knobs, inp, want, got


def col(a, name):
    return a[:, S.OUT_COLS.index(name)]


def test_every_recorded_row(sweep):
    """field for field, error codes and which message included"""
    knobs, inp, want, got = sweep
    bad = np.nonzero((got != want).any(axis=1))[0]
    show = [(knobs[inp[r, 0]], dict(zip(S.IN_COLS[1:], inp[r, 1:].tolist())),
             {S.OUT_COLS[c]: (int(want[r, c]), int(got[r, c])) for c in np.nonzero(got[r] != want[r])[0]}) for r in bad[:5]]
    assert len(bad) == 0, f"{len(bad)} of {len(inp)} rows differ, (knobs, inputs, {{field: (recorded, now)}}): {show}"


def test_fixture_reaches_every_branch(sweep):
    """the sweep cannot silently miss a branch: every kernel family, visited kind, filter kind, nt on and off, both prologue flags, every error"""
    knobs, inp, want, _ = sweep
    ok = want[col(want, "rc") == 0]
    assert set(col(ok, "family")) == {H.PLAN_LATENCY, H.PLAN_WALK2, H.PLAN_ONE_WAVE}
    assert set(col(ok, "vis_kind")) == {0, 16, 32}
    assert set(col(ok, "filter")) == {0, 16, 8, 80}
    w2 = ok[col(ok, "family") == H.PLAN_WALK2]
    assert set(col(w2, "w2")) == {4, 6, 7} and set(col(w2, "ev8")) == {0, 1} and set(col(w2, "r8")) == {0, 1}
    assert set(col(w2[col(w2, "ev8") == 1], "nt")) == {0, 1}
    assert set(col(w2, "upper")) == {0, H.ROWF_UPPER_FILTER, H.ROWF_UPPER_CACHED, H.ROWF_UPPER_FILTER | H.ROWF_UPPER_CACHED}
    assert (col(w2, "bloom_words") > 0).any() and (col(w2[col(w2, "vis_kind") == 0], "bloom_words") == 0).any()
    lat = ok[col(ok, "family") == H.PLAN_LATENCY]
    assert set(col(lat, "lat_seq")) == {0, 1} and set(col(lat, "lat_helpers")) == {0, 1, 3} and set(col(lat, "rows8_launch")) == {0, 1}
    assert set(col(ok, "v16_bits")) == {0, 1, 4, 10}
    err = want[col(want, "rc") != 0]
    assert set(col(err, "rc")) == {E_UNSUPPORTED}
    assert set(col(err, "err")) == {1, 2, 3}, "ef > 4096, LDS beyond 160 KiB, walk variant not compiled (the module docstring: why not the fourth message)"
    # every knob set of the sweep is in the fixture, the ROW_FILTER x ROW_FILTER_BITS pairs among them
    assert set(inp[:, 0]) == set(range(len(knobs)))
    assert all({"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": b} in knobs for b in ("8", "16", "8i"))
    for k in ("COLTT_VISG", "COLTT_WALK2", "COLTT_WALK2_LDS", "COLTT_BLOOM_KB", "COLTT_WAVES_PER_CU", "COLTT_EV8", "COLTT_ROWS_NT", "COLTT_ROWS_NT_MIN_MB",
              "COLTT_ROW_FILTER", "COLTT_ROW_FILTER_BITS", "COLTT_ROW_FILTER_UPPER", "COLTT_DESCENT_NT", "COLTT_VIS16", "COLTT_VIS16_BUCKET_BITS",
              "COLTT_LAT_MAX_NQ", "COLTT_MW_MAX_NQ", "COLTT_LAT_SEQ", "COLTT_LAT_HELPERS"):
        assert {k} in [set(ks) for ks in knobs], f"{k} is not swept alone"


def test_invariants_of_every_plan(sweep):
    """what the launcher's deleted cross-check stood for: the 16-bit visited set only under the 8i filter over LDS variant 4 with the eight-lane core; and no
    plan beyond the CU's LDS"""
    _, _, _, got = sweep
    ok = got[col(got, "rc") == 0]
    v16 = ok[col(ok, "vis_kind") == 16]
    assert len(v16) and (col(v16, "family") == H.PLAN_WALK2).all() and (col(v16, "filter") == 80).all() and (col(v16, "w2") == 4).all() and (col(v16, "ev8") == 1).all()
    assert (col(ok, "lds") <= 160 * 1024).all() and (col(ok, "lds") > 0).all()
    # a filter only over the eight-lane core; the eight-lane core only over line-transposed rows; nt only with it
    flt = ok[col(ok, "filter") != 0]
    assert (col(flt, "ev8") == 1).all() and (col(ok[col(ok, "ev8") == 1], "r8") == 1).all() and (col(ok[col(ok, "nt") == 1], "ev8") == 1).all()
    assert (col(ok[col(ok, "upper") != 0], "filter") != 0).all()
    assert (col(ok, "grid") >= 1).all() and (col(ok, "per_cu") >= 1).all()


def test_arguments_and_binding():
    L = coltt_amd.lib()
    f = dict(dim=768, metric=0, quant=0, m_max0=32, stride=3072, slots=10 ** 7, r8=1, shadow8=1, shadow16=0, vis_ready=0, vis_regions=0)
    p = H.search_plan_host(f, 10000, 10, 128)
    assert (p["family"], p["vis_kind"], p["filter"], p["w2"], p["ev8"], p["nt"], p["per_cu"], p["grid"]) == (H.PLAN_WALK2, 16, 80, 4, 1, 1, 7, 1792)
    assert H.search_plan_host(f, 1, 10, 128)["family"] == H.PLAN_LATENCY
    assert H.search_plan_host(f, 1, 10, 128, force=1)["family"] == H.PLAN_WALK2 and H.search_plan_host(f, 1, 10, 128, force=3)["family"] == H.PLAN_ONE_WAVE
    assert H.search_plan_host(f, 5, 200, 10)["ef"] == 200   # max(ef, k)
    for bad in (dict(nq=0, k=10, ef=64), dict(nq=1, k=0, ef=64), dict(nq=1, k=10, ef=0)):
        with pytest.raises(coltt_amd.ColttError) as e:
            H.search_plan_host(f, bad["nq"], bad["k"], bad["ef"])
        assert e.value.code == E_INVALID
    assert L.coltt_hnsw_search_plan_host(None, 1, 1, 1, 0, None) == E_INVALID
