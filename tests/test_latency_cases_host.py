"""The latency kernel's case table (tests/latency_cases.py) against the plan function, without a device: every case plans the launch it claims — family,
walk, helpers, row layout — under its knobs, the table names all 28 compiled instances of hnsw_search_lat_kernel, the capacity-edge bisection ends on the
hash-capacity rule, and one element past LAT_MAX_STRIDE leaves the kernel.  test_gpu_latency_instances.py runs the same table on a device; when the plan
moves, this file says which case no longer reaches its instance."""
import pytest

import latency_cases as LC
from coltt_amd import hnsw as H


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in LC.KNOBS:
        monkeypatch.delenv(k, raising=False)


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


def _plan_of(c, vis_ready):
    f = LC.facts(c, vis_ready)
    return lambda nq, k, ef: H.search_plan_host(f, nq, k, ef)


def test_table_constants_are_the_librarys():
    assert (LC.PLAN_LATENCY, LC.COSINE, LC.L2) == (H.PLAN_LATENCY, H.L.COSINE, H.L.EUCLIDEAN)
    assert (LC.Q_NONE, LC.Q_F16, LC.Q_F8, LC.Q_BF16) == (H.L.Q_NONE, H.L.Q_F16, H.L.Q_F8, H.L.Q_BF16)


@pytest.mark.parametrize("vis_ready", [0, 1])
@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c.name)
def test_case_plans_what_it_claims(monkeypatch, c, vis_ready):
    _set(monkeypatch, LC.search_knobs(c))
    plan = _plan_of(c, vis_ready)
    assert LC.LAT_MIN_STRIDE <= LC.stride(c) <= LC.LAT_MAX_STRIDE
    for nq in LC.NQS:
        for k, ef in LC.SEARCHES + (((LC.TIES_K, LC.TIES_K),) if c.group == "D" else ()):
            p = plan(nq, k, ef)
            if (k, ef) == (10, 200) and not c.ef200:
                assert p["family"] != H.PLAN_LATENCY, (c.name, p)
                continue
            assert p["family"] == H.PLAN_LATENCY, (c.name, nq, k, ef, p)
            assert (p["lat_seq"], p["lat_helpers"], p["r8"], p["rows8_launch"]) == (LC.lat_seq(c), 0, LC.r8(c), LC.r8(c)), (c.name, nq, k, ef, p)
            assert (p["vis_kind"], p["per_cu"], p["grid"], p["ef"]) == (32, 1, nq, max(k, ef)), (c.name, nq, k, ef, p)
    # the instance: what launch_search_lat makes of the plan and the facts
    f = LC.facts(c)
    assert LC.tp_of(f["r8"], f["stride"], LC.lat_seq(c)) == LC.tp(c)
    if c.group in "AB":
        assert LC.r8(c) == 1 and LC.lat_seq(c) == (c.group == "B")
    if c.group == "C":
        assert LC.tp(c) == LC.TP_STAGED


def test_table_reaches_all_28_instances():
    want = LC.all_instances()
    assert len(want) == 28
    got = {LC.instance(c) for c in LC.CASES}
    assert got == want, f"not reached: {sorted(want - got)}; not compiled: {sorted(got - want)}"
    # the shapes no other test launches: 25 lines = LAT_MAX_PIECES in both line-transposed formats, stride = LAT_MAX_STRIDE staged, two-chunk rows
    lines = {(c.quant, LC.stride(c) >> 7) for c in LC.CASES if LC.r8(c)}
    assert {(LC.Q_NONE, 25), (LC.Q_F16, 25), (LC.Q_F16, 8), (LC.Q_F16, 16), (LC.Q_NONE, 16), (LC.Q_NONE, 12), (LC.Q_F16, 12), (LC.Q_BF16, 12), (LC.Q_F16, 24), (LC.Q_NONE, 24)} <= lines
    assert any(LC.stride(c) == LC.LAT_MAX_STRIDE and not LC.r8(c) for c in LC.CASES)
    assert {c.group for c in LC.CASES if c.m == 24} == {"B", "C"}
    for names in (LC.EDGE_CASES, LC.SECOND_QUERY_CASES):
        assert {LC.BY_NAME[n].group for n in names} == {"A", "B", "C"}
    assert [LC.BY_NAME[n].group for n in LC.HELPER_CASES] == ["A", "C"] and LC.BY_NAME[LC.HELPER_SEQ_CASE].group == "B"


def test_801_elements_leave_the_latency_kernel():
    c799, c801 = LC.BY_NAME["c-f32-799-cos-pipelined"], LC.CASE_801
    assert (LC.stride(c799), LC.stride(c801)) == (3200, 3216)
    for vis_ready in (0, 1):
        for nq in LC.NQS:
            for k, ef in LC.SEARCHES:
                assert _plan_of(c801, vis_ready)(nq, k, ef)["family"] != H.PLAN_LATENCY, (nq, k, ef)
                if ef <= 128:
                    assert _plan_of(c799, vis_ready)(nq, k, ef)["family"] == H.PLAN_LATENCY, (nq, k, ef)


@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c.name)
def test_capacity_edge_bisection(monkeypatch, c):
    """the bisection ends with a latency plan below and another family above, and what it ends on is the hash-capacity rule (3/4 of the table against
    34 evaluations per result slot + 64), not the LDS limit: the table the plan gave is too small for one ef more"""
    _set(monkeypatch, LC.search_knobs(c))
    for vis_ready in (0, 1):
        plan = _plan_of(c, vis_ready)
        e = LC.largest_latency_ef(plan)
        assert e is not None and 128 <= e < 4096, (c.name, e)
        below, above = plan(1, 10, e), plan(1, 10, e + 1)
        assert below["family"] == H.PLAN_LATENCY and above["family"] != H.PLAN_LATENCY, (c.name, e, below, above)
        assert (below["hcap"] // 4) * 3 >= e * 34 + 64 > (below["hcap"] // 4) * 3 - 34, (c.name, e, below)
        assert c.ef200 == (e >= 200), (c.name, e)
        assert all(plan(1, 10, x)["family"] == H.PLAN_LATENCY for x in range(10, e + 1, 7)), c.name
    assert LC.largest_latency_ef(_plan_of(LC.CASE_801, 1)) is None


@pytest.mark.parametrize("name", LC.SECOND_QUERY_CASES)
def test_second_query_call_plans_a_grid_of_256(monkeypatch, name):
    c = LC.BY_NAME[name]
    _set(monkeypatch, LC.search_knobs(c))
    assert _plan_of(c, 1)(LC.SECOND_QUERY_NQ, 10, 64)["family"] != H.PLAN_LATENCY     # beyond the default COLTT_LAT_MAX_NQ of 256
    monkeypatch.setenv("COLTT_LAT_MAX_NQ", "512")
    p = _plan_of(c, 1)(LC.SECOND_QUERY_NQ, 10, 64)
    assert (p["family"], p["grid"], p["lat_seq"]) == (H.PLAN_LATENCY, 256, LC.lat_seq(c)), p


@pytest.mark.parametrize("helpers", [1, 2, 3])
def test_helper_calls_plan_the_knob(monkeypatch, helpers):
    monkeypatch.setenv("COLTT_LAT_HELPERS", str(helpers))
    for name in LC.HELPER_CASES:
        c = LC.BY_NAME[name]
        assert LC.lat_seq(c) == 0
        for nq in LC.HELPER_NQS:          # nq 9 > LAT_MASTERS launches no helper; the plan field is set all the same
            for ef in LC.HELPER_EFS:
                p = _plan_of(c, 1)(nq, 10, ef)
                assert (p["family"], p["lat_helpers"], p["grid"]) == (H.PLAN_LATENCY, helpers, nq), (name, nq, ef, p)
    c = LC.BY_NAME[LC.HELPER_SEQ_CASE]
    _set(monkeypatch, LC.search_knobs(c))
    p = _plan_of(c, 1)(1, 10, 64)
    assert (p["family"], p["lat_seq"], p["lat_helpers"]) == (H.PLAN_LATENCY, 1, 0), p     # the sequential walk takes none
