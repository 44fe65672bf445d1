"""The 16-bit LDS visited set of the headline row-filter walk (coltt_amd/csrc/vis16.hpp; hnsw_walk2.hpp: VIS_LDS16) changes where a traversal remembers
what it has seen and how many traversals share a CU, never what a search answers.  One index answers the same call on the 16-bit table and — through
COLTT_VIS16=0 — on the 32-bit one: ids, score bits, counts, the traversal counters and the row filter's counters equal each other's and the oracle's.
COLTT_VIS16_BUCKET_BITS shrinks the table so that a small walk fills bucket pairs and uses the stash (same equalities), and so that the stash overflows
(the call is re-run and still answers as the oracle)."""
import numpy as np
import pytest

import test_gpu_row_filter8 as T8
from oracle import oracle as O
from util import assert_same_results, bits

pytestmark = pytest.mark.gpu

KNOBS = T8.KNOBS + ("COLTT_VIS16", "COLTT_VIS16_BUCKET_BITS", "COLTT_WAVES_PER_CU", "COLTT_ROWS_NT", "COLTT_WALK2_LDS", "COLTT_VISG", "COLTT_EV8")
SHAPES = {768: 6000, 256: 6000}   # phase A: one burst of 6 lines (the headline's form) | the other one-burst form, of 2
NQ, K = 48, 10
# The shrunken tables.  The header on the host, 2 000 random fills of the fixture's 6 000 slots per table size:
#   2^7 buckets (1 024 entries): the first slot goes to the stash after 710 .. 941 insertions (773 / 859 / 915 at 1 % / 50 % / 99 %), the stash overflows
#                                after 933 .. 1 005 (944 at 1 %);
#   2^8 buckets (2 048 entries): the stash after 1 450 .. 1 828 (1 527 / 1 695 / 1 793), overflow after 1 820 .. 1 948 (1 836 at 1 %).
# A traversal that visits a number of vertices in STASH_WINDOW[bits] — from about the median first use to under the least overflow seen — has probably used
# the stash and not overflowed it.  The fixture's walks visit 500 .. 1 960 vertices at ef 20 .. 64: the test asks the library's table how many each
# (query, ef) visits, runs the STASH_CALLS fullest of those inside a window ONE QUERY PER CALL on that small table, and asserts that every one answers as
# the 32-bit table and the oracle and that the stash was in use in some of them.
# 2^4 buckets hold 128 entries + 16 in the stash, fewer than any ef 128 walk visits.
STASH_WINDOW = {7: (840, 915), 8: (1680, 1810)}
STASH_EFS, STASH_CALLS = range(20, 66, 4), 24
OVERFLOW_BITS, OVERFLOW_EF = 4, 128


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    monkeypatch.setenv("COLTT_MW_MAX_NQ", "0")   # batches of any size on the one-wave-per-query kernels
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("COLTT_ROW_FILTER", "1")  # (the default takes the filter for row arrays far larger than the caches only)


_CASES = {}


def _case(gpu, d):
    """the Gaussian index of this width (M 16, the default 8-bit shadow), its queries and the oracle's answers per ef — built once"""
    if d not in _CASES:
        n = SHAPES[d]
        X = O.fill_normal(16000 + d, (n, d)); lv = O.levels(16001 + d, n)
        gh = T8._gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=60), batch=256)
        assert gh.cfg.m == 16 and gh.RowFilterStats()["shadow_bits"] == (8,)
        _CASES[d] = {"gh": gh, "Q": O.fill_normal(16002 + d, (NQ, d)), "g": gh.ExportRaw(), "rows": gh.FetchRows(), "oracle": {}}
    return _CASES[d]


def _oracle(c, ef):
    if ef not in c["oracle"]:
        g = c["g"]
        c["oracle"][ef] = O.csr_search(c["rows"], O.Q_NONE, g["adj0"], g["upper_off"], g["adjU"], c["gh"].dim, O.COSINE, g["entry"], g["entry_level"], c["Q"], K, ef, threads=4)
    return c["oracle"][ef]


def _run(c, ef, monkeypatch, qi=None, **env):
    """one call (all queries, or query qi alone) under the given knobs: (answers + traversal counters, the row filter's counter deltas, the visited set's report)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gh = c["gh"]
    a = gh.RowFilterStats(); n0 = gh.VisitedStats()["launches16"]
    res = gh.Search(c["Q"] if qi is None else c["Q"][qi:qi + 1], K, ef=ef, with_stats=True)
    b = gh.RowFilterStats(); vs = gh.VisitedStats()
    vs["launches16"] -= n0
    for k in env:
        monkeypatch.delenv(k)
    return res, {kk: b[kk] - a[kk] for kk in ("rejected", "f32_rows", "shadow_rows", "launches")}, vs


def _assert_equal_runs(a, b, tag):
    (i0, s0, c0, st0), f0, _ = a
    (i1, s1, c1, st1), f1, _ = b
    assert np.array_equal(i0, i1) and np.array_equal(bits(s0), bits(s1)) and np.array_equal(c0, c1), f"{tag}: answers differ"
    assert st0 == st1, (tag, st0, st1)        # n_dist / n_exp / n_hops
    assert f0 == f1, (tag, f0, f1)            # rejected / f32 rows / shadow rows / launches


def _assert_oracle(c, ef, run, tag):
    sl, sc, cn, ost, _ = _oracle(c, ef)
    (i1, s1, c1, st1), f, _ = run
    for qi in range(NQ):
        assert_same_results(i1[qi, :c1[qi]], s1[qi, :c1[qi]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], f"{tag} q{qi}")
    assert {k_: st1[k_] for k_ in ost} == ost, (tag, st1, ost)
    assert f["launches"] == 1 and f["rejected"] > 0


@pytest.mark.parametrize("d,ef", [(768, 128), (768, 32), (256, 128)])
def test_the_16_bit_table_answers_as_the_32_bit_one_and_the_oracle(gpu, monkeypatch, d, ef):
    c = _case(gpu, d)
    for nt in ("0", "1"):   # both load-hint twins of the instance
        tag = f"d{d} ef{ef} nt{nt}"
        r16 = _run(c, ef, monkeypatch, COLTT_ROWS_NT=nt)
        r32 = _run(c, ef, monkeypatch, COLTT_ROWS_NT=nt, COLTT_VIS16="0")
        print(f"{tag}: 16-bit {r16[2]}  32-bit {r32[2]}  filter {r16[1]}")
        assert r16[2]["kind"] == 16 and r16[2]["launches16"] == 1 and r16[2]["waves_per_cu"] > 4, r16[2]
        assert r32[2]["kind"] == 32 and r32[2]["launches16"] == 0 and r32[2]["waves_per_cu"] == 4, r32[2]
        assert r16[2]["grid"] == NQ and 0 < r16[2]["visited_max"] <= 6144 and r16[2]["stash_max"] <= 16
        _assert_equal_runs(r16, r32, tag)
        _assert_oracle(c, ef, r16, tag + " 16-bit")
        _assert_oracle(c, ef, r32, tag + " 32-bit")


def test_a_small_table_fills_buckets_and_uses_the_stash(gpu, monkeypatch):
    c = _case(gpu, 768)
    fill = {(ef, qi): _run(c, ef, monkeypatch, qi=qi)[2]["visited_max"] for ef in STASH_EFS for qi in range(NQ)}   # vertices each walk visits (the library's table)
    picked = [(b, k_) for b, (lo, hi) in STASH_WINDOW.items() for k_, v in fill.items() if lo <= v <= hi]
    picked = sorted(picked, key=lambda t: -fill[t[1]] / (8 << t[0]))[:STASH_CALLS]   # the fullest tables first
    print(f"walks inside a window: {[(b, fill[k_]) for b, k_ in picked]} (of {len(fill)} walks visiting {min(fill.values())} .. {max(fill.values())} vertices)")
    assert len(picked) >= 8, "the fixture has too few walks that fill a small table to where its stash is in use"
    used = []
    for b, (ef, qi) in picked:
        tag = f"2^{b} buckets, ef {ef}, q{qi}"
        r16 = _run(c, ef, monkeypatch, qi=qi, COLTT_VIS16_BUCKET_BITS=str(b))
        r32 = _run(c, ef, monkeypatch, qi=qi, COLTT_VIS16="0")
        assert r16[2]["launches16"] == 1 and r32[2]["kind"] == 32
        sl, sc, cn, _, _ = _oracle(c, ef)
        for r in (r16, r32):
            (i1, s1, c1, _), _, _ = r
            assert_same_results(i1[0, :c1[0]], s1[0, :c1[0]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], tag)
        if r16[2]["kind"] == 16:   # answered on the small table (else its stash overflowed and the call was re-run: the next test's subject)
            assert r16[2]["visited_max"] == fill[(ef, qi)] and r16[2]["stash_max"] <= 16
            _assert_equal_runs(r16, r32, tag)
            used.append(r16[2]["stash_max"])
    print("stash entries per call answered on a small table:", used)
    assert len(used) >= len(picked) // 2 and max(used) > 0, "no walk used the stash"


def test_a_stash_that_overflows_reruns_the_call(gpu, monkeypatch):
    c = _case(gpu, 768)
    tag = f"2^{OVERFLOW_BITS} buckets, ef {OVERFLOW_EF}"
    r16 = _run(c, OVERFLOW_EF, monkeypatch, COLTT_VIS16_BUCKET_BITS=str(OVERFLOW_BITS))
    print(f"{tag}: {r16[2]}")
    # the 16-bit launch happened, gave up, and the launch that answered kept a 32-bit table (hnsw_dev.hpp: search_level)
    assert r16[2]["launches16"] == 1 and r16[2]["kind"] == 32 and r16[2]["stash_max"] == 0, r16[2]
    sl, sc, cn, ost, _ = _oracle(c, OVERFLOW_EF)
    (i1, s1, c1, st1), f, _ = r16
    for qi in range(NQ):
        assert_same_results(i1[qi, :c1[qi]], s1[qi, :c1[qi]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], f"{tag} q{qi}")
    assert {k_: st1[k_] for k_ in ost} == ost and f["launches"] == 0   # (only the launch that answered counts, and it is not a filtered one)


def test_the_knob_and_the_limits_choose_the_table(gpu, monkeypatch):
    c = _case(gpu, 768)
    # ef above 128 walks over the HBM byte map, the unfiltered walk and the f32-query filter keep the 32-bit table
    assert _run(c, 200, monkeypatch)[2]["kind"] == 0
    assert _run(c, 64, monkeypatch, COLTT_ROW_FILTER="0")[2]["kind"] == 32
    monkeypatch.setenv("COLTT_ROW_FILTER", "1")
    assert _run(c, 64, monkeypatch, COLTT_ROW_FILTER_BITS="8")[2]["kind"] == 32
    # COLTT_WAVES_PER_CU overrides the seven
    for wv in (4, 5, 6, 7):
        r = _run(c, 64, monkeypatch, COLTT_WAVES_PER_CU=str(wv))
        assert r[2]["kind"] == 16 and r[2]["waves_per_cu"] == wv, r[2]
