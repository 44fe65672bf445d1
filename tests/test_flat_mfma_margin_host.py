"""The candidate margin of the FLAT matrix-core search, without a device (tests/flat_mfma_ref.py is the model).

MODE_MFMA promises the exact scan's ids, ranks and score bits.  That rests on ONE claim: the pick margin is at least twice the worst
error of the approximate candidate value, so the kept set holds every true top-k member.  For every point of the grid below either
coltt_flat_mfma_eligible_host — the function search_prepared itself calls — answers no for the store's real norm bounds (the store then
takes the exact scan), or the model's kept set is a superset of the float64 top-k for every query.  The data sets put near ties at the
k-th place (random rows never do: their gap at the k-th place is 10 - 1000 times the error), take away the cancellation the margins'
derivations do not rely on, and scale the store down into binary16's subnormal range, where rounding f32 rows is an ABSOLUTE error.

Sensitivity: on the near-tie bands a margin of zero must lose a true top-k member for f32 rows — the data sets fail a wrong margin.
For 2-byte rows the model has NO rounding error (the codes are exact binary16 operands and the model's dot product is exact; what is left
on the device is the f32 accumulation order, ~1e-6, which this model leaves out), so a zero margin loses nothing there: those rows are
left out of the sensitivity check, and tests/test_gpu_flat_mfma_margin.py runs them on the device."""
import numpy as np
import pytest

import flat_mfma_ref as R
from oracle import oracle as O

KS = (1, 10, 100)
SHAPE = {32: (16, 2800), 128: (16, 2800), 768: (8, 1000), 4096: (4, 300)}     # d -> (queries, filler rows); 200 planted rows per query
SCALED_N = {32: 20000, 128: 20000, 768: 3000, 4096: 600}
SCALES = (1.0, 1e-3, 1e-5, 1e-6, 3e-7, 1e-7)
METRICS = {"cos": O.COSINE, "l2": O.L2}
QUANTS = {"none": O.Q_NONE, "f16": O.Q_F16}
CONSTS = R.constants()


def scores(metric, quant, X, Q, loaded=False):
    vals = (R.loaded_rows(quant, X) if loaded else R.stored_rows(metric, quant, X))[1]
    return R.Scores(metric, quant, vals, R.prepared_queries(metric, quant, Q))


def superset_or_closed(sc, tag, must_be_open=None):
    """the contract of one grid point; returns whether the matrix cores serve it"""
    is_open = R.eligible(sc.metric, sc.quant, sc.dim, sc.min_norm, sc.max_norm)
    if must_be_open is not None:
        assert bool(is_open) == must_be_open, (tag, sc.min_norm, sc.max_norm)
    if not is_open:
        return False
    for nearest in (True, False):
        for k in KS:
            ok, kept, missed = sc.kept_superset(k, nearest, consts=CONSTS)
            assert ok.all(), f"{tag} k{k} nearest{nearest}: {int(missed.sum())} true top-k members of {int((~ok).sum())} queries are outside the kept set " \
                             f"(kept {kept.tolist()}, min/max norm {sc.min_norm} {sc.max_norm})"
    return True


def test_the_parsed_constants_are_the_derived_ones():
    """flat.hip / flat_mfma.hpp state a derivation beside each constant; the numbers must not be below what the derivation gives."""
    c = CONSTS
    assert c["L2_ULP"] == np.float32(2.0 ** -24) and c["L2_ACC_TERMS"] == 4
    assert 2.0 ** -10 + 2.0 ** -22 <= c["L2_ROUND_F16"] < 1.01 * (2.0 ** -10 + 2.0 ** -22)
    want = (1.5 + 2.0 ** -11) * 2.0 ** -24
    assert want <= c["L2_ABS_F16"] < 1.001 * want
    # cosine over unit rows, D <= 4096: accumulation D * 2^-24 * sum|a_i b_i| <= 2.5e-4; f32 rows add (2^-10 + 2^-22) for the two roundings
    assert c["MF_MARGIN"] >= 2 * 4096 * 2.0 ** -24 and c["MF_MARGIN_F32"] >= 2 * (4096 * 2.0 ** -24 + 2.0 ** -10 + 2.0 ** -22)
    assert c["QN_MAX"] == np.float32(4.0e9)


def test_eligibility_truth_table():
    """coltt_flat_mfma_eligible_host(metric, quant, dim, min_norm, max_norm, f8_expanded): the latches of flat.hip, one by one"""
    E, nan, inf = R.eligible, float("nan"), float("inf")
    for q in (O.Q_NONE, O.Q_F16, O.Q_BF16):
        assert E(O.COSINE, q, 128, 1.0, 1.0) and E(O.COSINE, q, 128, 0.25, 4.0)
        assert not E(O.COSINE, q, 128, 0.2499, 1.0) and not E(O.COSINE, q, 128, 1.0, 4.001) and not E(O.COSINE, q, 128, 0.0, 1.0)
        assert not E(O.COSINE, q, 128, nan, nan) and not E(O.COSINE, q, 128, 1.0, inf)
        assert E(O.L2, q, 128, 0.0, 1.0) and E(O.L2, q, 128, 1e-14, 1e-12) and not E(O.L2, q, 128, nan, nan) and not E(O.L2, q, 128, 0.0, inf)
        for dim, want in ((7, 0), (8, 1), (33, 1), (4096, 1), (4097, 0)):
            assert E(O.L2, q, dim, 1.0, 2.0) == want and E(O.COSINE, q, dim, 1.0, 1.0) == want, (q, dim)
    # f32 rows are cast to binary16: ||row||^2 <= 4e9 keeps every element finite; 2-byte codes are finite by construction
    assert E(O.L2, O.Q_NONE, 128, 1.0, 4.0e9) and not E(O.L2, O.Q_NONE, 128, 1.0, 4.1e9)
    assert E(O.L2, O.Q_F16, 128, 1.0, 1e30) and not E(O.L2, O.Q_F16, 128, 1.0, 3.1e38)
    # "f8": cosine only, and only with the expanded binary16 copy; any finite norms
    assert E(O.COSINE, O.Q_F8, 128, 1e-12, 1e-10, 1) and not E(O.COSINE, O.Q_F8, 128, 1e-12, 1e-10, 0)
    assert not E(O.L2, O.Q_F8, 128, 1.0, 1.0, 1) and not E(O.COSINE, O.Q_F8, 128, 1.0, inf, 1)
    assert not E(2, O.Q_NONE, 128, 1.0, 1.0) and not E(O.COSINE, 7, 128, 1.0, 1.0)


@pytest.mark.parametrize("metric,quant", [(O.COSINE, O.Q_NONE), (O.COSINE, O.Q_F16), (O.L2, O.Q_F16), (O.L2, O.Q_NONE)])
def test_the_model_reads_the_stores_rows(metric, quant):
    """stored_rows / prepared_queries restate Normalize + Lower: the codes are the oracle store's own"""
    X, Q = R.scaled_set(11, 40, 24, 2, 1e-6 if metric == O.L2 else 1.0)
    of = O.Flat(24, metric, quant); of.upsert(np.arange(40, dtype=np.uint64), X)
    codes, _ = R.stored_rows(metric, quant, X)
    for i in (0, 7, 39):
        assert np.array_equal(of.get(i).view(np.uint8), codes[i].view(np.uint8)), i


@pytest.mark.parametrize("d", sorted(SHAPE))
@pytest.mark.parametrize("base", [0.05, 0.9, 1.9])
@pytest.mark.parametrize("quant", sorted(QUANTS))
def test_near_tie_bands_cosine(quant, base, d):
    nq, fill = SHAPE[d]
    X, Q = R.band_set(7000 + d, d, nq, fill, base)
    assert superset_or_closed(scores(O.COSINE, QUANTS[quant], X, Q), f"cos {quant} d{d} base{base}", must_be_open=True)


@pytest.mark.parametrize("d", sorted(SHAPE))
@pytest.mark.parametrize("base", [0.05, 0.9, 1.9])
@pytest.mark.parametrize("norm", [1.0, 100.0])
@pytest.mark.parametrize("quant", sorted(QUANTS))
def test_near_tie_bands_euclidean(quant, norm, base, d):
    nq, fill = SHAPE[d]
    X, Q = R.band_set(7100 + d, d, nq, fill, base, scale=norm)
    assert superset_or_closed(scores(O.L2, QUANTS[quant], X, Q), f"l2 {quant} d{d} base{base} norm{norm}", must_be_open=True)


@pytest.mark.parametrize("metric", sorted(METRICS))
@pytest.mark.parametrize("quant", sorted(QUANTS))
def test_all_positive_rows_at_4096(quant, metric):
    X, Q = R.positive_set(7200, 1500, 4096, 8)
    assert superset_or_closed(scores(METRICS[metric], QUANTS[quant], X, Q), f"{metric} {quant} positive", must_be_open=True)


@pytest.mark.parametrize("d", sorted(SCALED_N))
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("quant", sorted(QUANTS))
def test_scaled_euclidean_stores(quant, s, d):
    """f32 rows at s <= 3e-6 are the points the relative margin alone misses (binary16 subnormals round with an ABSOLUTE error of 2^-25 per
    element); the absolute term of l2_abs covers them."""
    X, Q = R.scaled_set(7300 + d, SCALED_N[d], d, 32 if d <= 128 else 8, s)
    assert superset_or_closed(scores(O.L2, QUANTS[quant], X, Q), f"l2 {quant} d{d} s{s}", must_be_open=True)


@pytest.mark.parametrize("d", sorted(SCALED_N))
@pytest.mark.parametrize("quant", sorted(QUANTS))
def test_scaled_cosine_streams_are_latched(quant, d):
    """a loaded stream is stored as it is: Gaussian rows times s have ||row||^2 ~ d s^2, outside [1/4, 4] for every s here — the latch says no"""
    for s in SCALES:
        X, Q = R.scaled_set(7400 + d, 500, d, 4, s)
        assert not superset_or_closed(scores(O.COSINE, QUANTS[quant], X, Q, loaded=True), f"cos {quant} d{d} s{s}", must_be_open=False)
    # ... and a stream of unit rows is served by the matrix cores, inside the margin
    X, Q = R.scaled_set(7400 + d, 500, d, 4, 1.0)
    assert superset_or_closed(scores(O.COSINE, QUANTS[quant], O.normalize(X), Q, loaded=True), f"cos {quant} d{d} unit stream", must_be_open=True)


@pytest.mark.parametrize("d", [32, 128, 768, 4096])
@pytest.mark.parametrize("quant", sorted(QUANTS))
def test_mixed_euclidean_store(quant, d):
    X, Q = R.mixed_set(7500 + d, 2000 if d <= 768 else 400, d, 8)
    sc = scores(O.L2, QUANTS[quant], X, Q)
    assert sc.max_norm > 0.9e6 and sc.min_norm < 1.1e-10
    assert superset_or_closed(sc, f"l2 {quant} d{d} mixed", must_be_open=True)
    assert sc.kept_superset(10, True, consts=CONSTS)[1].min() == len(X) - 1   # everything but the far row is within the margin: legal


@pytest.mark.parametrize("metric", sorted(METRICS))
def test_a_zero_margin_fails_the_bands(metric):
    """f32 rows, d = 128, 16 queries x 200 planted rows in a band 4e-4 wide: without the margin the rounding of rows and query to binary16
    reorders the k-th place and true members are lost — so these data sets do fail a margin that is wrong.  (2-byte rows: see the module
    docstring — the model has no error to lose them with.)"""
    lost = 0
    for base in (0.05, 0.9, 1.9):
        X, Q = R.band_set(7000 + 128, 128, 16, SHAPE[128][1], base)
        sc = scores(METRICS[metric], O.Q_NONE, X, Q)
        for k in KS:
            ok, kept, missed = sc.kept_superset(k, base < 1.0, margin_override=0.0)
            assert (kept >= k).all()
            lost += int((~ok).sum())
            if k == 10 and base == 0.05:
                assert not ok.all(), (metric, "margin 0 must lose a top-10 member of the 0.05 band")
    assert lost > 0
