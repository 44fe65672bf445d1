"""The launch does what the plan says.  For small indexes of four row formats, under each knob setting that moves the decision: take
Hnsw.SearchPlan(nq, k, ef) (coltt_hnsw_search_plan_host over the index's facts — the function the search itself decides by), run the search, and compare
what the launch left in the counters — the visited set's kind, the traversals per CU, the grid, launches on the 16-bit table; row-filter launches and
filtered descents; launches that read line-transposed rows as such — with the plan; and the answers with the oracle's canonical search over the arrays
copied out of HBM, so that a wrong kernel instance cannot hide behind a matching counter."""
import numpy as np
import pytest

import test_gpu_row_filter as TRF
from oracle import oracle as O
from util import assert_same_results

pytestmark = pytest.mark.gpu

N, M, K = 3000, 8, 10
NQS, EFS = (1, 300), (32, 128, 160)
# dim 256 f32: the smallest shape that is line-transposed by default, and its 1 024-byte rows meet the latency kernel's stride rule; dim 128: natural order
INDEXES = {"f32_256_cos": (256, O.COSINE, O.Q_NONE), "f32_128_cos": (128, O.COSINE, O.Q_NONE), "f16_256_cos": (256, O.COSINE, O.Q_F16), "f8_256_l2": (256, O.L2, O.Q_F8)}
KNOBS = ("COLTT_ROW_FILTER", "COLTT_ROW_FILTER_BITS", "COLTT_ROW_FILTER_UPPER", "COLTT_VIS16", "COLTT_VIS16_BUCKET_BITS", "COLTT_ROWS_NT", "COLTT_ROWS_NT_MIN_MB",
         "COLTT_EV8", "COLTT_WALK2", "COLTT_WALK2_LDS", "COLTT_VISG", "COLTT_BLOOM_KB", "COLTT_WAVES_PER_CU", "COLTT_DESCENT_NT", "COLTT_LAT_MAX_NQ", "COLTT_MW_MAX_NQ",
         "COLTT_LAT_SEQ", "COLTT_LAT_HELPERS", "COLTT_ROW_SHADOW", "COLTT_ROW_SHADOW_BITS", "COLTT_ROWS8")
SETTINGS = {
    "default": {},
    "filter8": {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": "8"},
    "filter16": {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": "16"},
    "filter8i": {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_BITS": "8i"},
    "filter_vis32": {"COLTT_ROW_FILTER": "1", "COLTT_VIS16": "0"},
    "filter_upper": {"COLTT_ROW_FILTER": "1", "COLTT_ROW_FILTER_UPPER": "1"},
    "rows_nt": {"COLTT_ROWS_NT": "1"},
    "ev8_off": {"COLTT_EV8": "0"},
    "walk2_off": {"COLTT_WALK2": "off"},
    "walk2_lds_off": {"COLTT_WALK2_LDS": "off"},
    "walk2_5": {"COLTT_WALK2": "5"},   # not compiled: the calls that would take it are refused, nothing is launched
}
E_UNSUPPORTED = -4


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


_CASES = {}


def _case(gpu, name, monkeypatch):
    """the index (random unit vectors, M 8; the f32 cosine ones keep both shadows, so that each COLTT_ROW_FILTER_BITS is served by its own), its queries,
    its arrays, the oracle's answers per ef — built once"""
    if name not in _CASES:
        d, metric, quant = INDEXES[name]
        seed = 23000 + 10 * list(INDEXES).index(name)
        X = O.fill_normal(seed, (N, d)); X /= np.linalg.norm(X, axis=1, keepdims=True)
        monkeypatch.setenv("COLTT_ROW_SHADOW_BITS", "both")
        gh = TRF._gpu_build(gpu, X.astype(np.float32), O.levels(seed + 1, N), metric, quant, gpu.HnswCfg.default(m=M, ef_construction=40), batch=256)
        monkeypatch.delenv("COLTT_ROW_SHADOW_BITS")
        Q = O.fill_normal(seed + 2, (max(NQS), d))
        gh.Search(Q[:1], K, ef=max(EFS))   # the first search above ef 128 makes the HBM visited workspace: from here on the facts hold still
        f = gh.PlanFacts()
        assert f.vis_ready and f.slots == N and f.m_max0 == 2 * M and bool(f.r8) == (d == 256 and quant != O.Q_F8)
        assert (f.shadow8, f.shadow16) == ((1, 1) if (d == 256 and quant == O.Q_NONE) else (0, 0))
        _CASES[name] = {"gh": gh, "Q": Q, "g": gh.ExportRaw(), "rows": gh.FetchRows(), "metric": metric, "quant": quant, "oracle": {}}
    return _CASES[name]


def _oracle(c, ef):
    if ef not in c["oracle"]:
        g = c["g"]
        c["oracle"][ef] = O.csr_search(c["rows"], c["quant"], g["adj0"], g["upper_off"], g["adjU"], c["gh"].dim, c["metric"], g["entry"], g["entry_level"], c["Q"], K, ef, threads=4)
    return c["oracle"][ef]


def _counters(gh):
    v, f = gh.VisitedStats(), gh.RowFilterStats()
    return {"kind": v["kind"], "per_cu": v["waves_per_cu"], "grid": v["grid"], "launches16": v["launches16"], "filter_launches": f["launches"],
            "upper_launches": f["upper_launches"], "rows8_launches": gh.Rows8()[0]}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", list(INDEXES))
def test_launch_follows_plan(gpu, monkeypatch, name, setting):
    c = _case(gpu, name, monkeypatch)
    gh = c["gh"]
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    refused = 0
    for nq in NQS:
        for ef in EFS:
            tag = f"{name} {setting} nq{nq} ef{ef}"
            before = _counters(gh)
            try:
                p = gh.SearchPlan(nq, K, ef)
            except gpu.ColttError as e:
                assert setting == "walk2_5" and e.code == E_UNSUPPORTED and "is not compiled into this build" in str(e), (tag, e)
                with pytest.raises(gpu.ColttError) as e2:
                    gh.Search(c["Q"][:nq], K, ef=ef)
                assert e2.value.code == E_UNSUPPORTED and "is not compiled into this build" in str(e2.value), tag
                assert _counters(gh) == before, f"{tag}: a refused call launched"
                refused += 1
                continue
            gi, gs, gc = gh.Search(c["Q"][:nq], K, ef=ef)
            after = _counters(gh)
            print(tag, p, after)
            assert (after["kind"], after["per_cu"], after["grid"]) == (p["vis_kind"], p["per_cu"], p["grid"]), (tag, p, after)
            assert after["launches16"] - before["launches16"] == (1 if p["vis_kind"] == 16 else 0), (tag, p)
            assert after["filter_launches"] - before["filter_launches"] == (1 if p["filter"] else 0), (tag, p)
            assert after["upper_launches"] - before["upper_launches"] == (1 if p["filter"] and p["upper"] & 1 else 0), (tag, p)
            assert after["rows8_launches"] - before["rows8_launches"] == p["rows8_launch"], (tag, p)
            sl, sc, cn, _, _ = _oracle(c, ef)
            for qi in range(nq):
                assert_same_results(gi[qi, :gc[qi]], gs[qi, :gc[qi]], sl[qi, :cn[qi]].astype(np.uint64), sc[qi, :cn[qi]], f"{tag} q{qi}")
    assert (refused > 0) == (setting == "walk2_5"), (name, setting, refused)


def test_the_settings_reach_the_instances(gpu, monkeypatch):
    """on the line-transposed f32 cosine index the settings above take the plans they are there for"""
    gh = _case(gpu, "f32_256_cos", monkeypatch)["gh"]

    def plan(setting, nq, ef):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in SETTINGS[setting].items():
            monkeypatch.setenv(k, v)
        return gh.SearchPlan(nq, K, ef)

    G = gpu.hnsw
    p = plan("default", 300, 128); assert (p["family"], p["w2"], p["ev8"], p["filter"], p["vis_kind"], p["nt"]) == (G.PLAN_WALK2, 4, 1, 0, 32, 0)
    p = plan("default", 300, 160); assert (p["family"], p["w2"], p["vis_kind"]) == (G.PLAN_WALK2, 7, 0) and p["bloom_words"] > 0
    assert plan("default", 1, 128)["family"] == G.PLAN_LATENCY
    assert [plan(s, 300, 128)["filter"] for s in ("filter8", "filter16", "filter8i")] == [8, 16, 80]
    assert plan("filter8i", 300, 128)["vis_kind"] == 16 and plan("filter_vis32", 300, 128)["vis_kind"] == 32 and plan("filter_vis32", 300, 128)["filter"] == 80
    assert plan("filter8i", 300, 160)["vis_kind"] == 0 and plan("filter8i", 300, 160)["filter"] == 80
    assert plan("filter_upper", 300, 128)["upper"] & G.ROWF_UPPER_FILTER
    assert plan("rows_nt", 300, 128)["nt"] == 1
    p = plan("ev8_off", 300, 128); assert (p["ev8"], p["r8"], p["rows8_launch"]) == (0, 1, 0)
    assert plan("walk2_off", 300, 160)["family"] == G.PLAN_ONE_WAVE and plan("walk2_lds_off", 300, 128)["family"] == G.PLAN_ONE_WAVE
