"""The margin of the level-0 row filter over the 8-bit shadow with a QUANTISED QUERY is a theorem, not a tolerance (coltt_amd/csrc/row_filter8i.hpp).

The header is compiled with the host compiler — the very functions the kernel runs — and both quantisers are restated in numpy (the rows':
row_filter8_ref.py, the query's: row_filter8i_ref.py).  Phase A is an exact integer I = sum qh_i c_i, so there is ONE bound per pair.  Against exact
rational arithmetic (fractions.Fraction over the exact binary values of the f32 inputs):

    dot_exact_f32  <=  t s I + E_exact  <=  U = fl(fl(t s I) + E)            and            d_exact >= d_lo

where dot_exact_f32 / d_exact come from the oracle's AVX-order kernel (what the exact GPU kernel reproduces bit for bit), E_exact is the derivation's
steps (a)-(b) evaluated exactly with the TRUE sums (gamma_k P, t qh . (x - s c), (q - t qh) . x), and U / d_lo what the header returns from the f32
squared norms and the STORED (t, e_q, s, e) alone.  Both stored error norms are checked against the exact ones.  Zero violations: a condition, not a
rate."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import row_filter8i_ref as R8
from oracle import oracle as O
from row_filter8_ref import quantise

DIMS = (256, 768, 1536, 2304)


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    return R8.compile_header(tmp_path_factory.mktemp("rf8i"))


def _fr(a):
    return [Fr(float(v)) for v in a]


def _check(rf, q, x, tag, rows_quant=None):
    """every inequality of the docstring for one (query, row); rows_quant: (c, s, e) where the row's codes are chosen by the test"""
    q = np.ascontiguousarray(q, np.float32); x = np.ascontiguousarray(x, np.float32)
    dim = q.size
    c, s, e = rows_quant if rows_quant is not None else quantise(x)
    t, qh, h, l, eq = R8.quantise_query(q)
    assert np.isfinite(e) and np.isfinite(eq) and t > 0, tag
    assert np.array_equal(128 * h.astype(np.int64) + l.astype(np.int64), qh)
    # the header's scalar steps are the restatement's
    assert rf.rf8i_scale(float(np.max(np.abs(q))), 0) == t
    for i in (0, dim // 3, dim - 1, int(np.argmax(np.abs(q)))):
        assert rf.rf8i_level(float(q[i]), float(t)) == qh[i], (tag, i)
    fq, fx, ft, fs = _fr(q), _fr(x), Fr(float(t)), Fr(float(s))
    iq = [int(v) for v in qh]; ic = [int(v) for v in c]
    bad = []
    # the stored error norms
    qerr2 = sum((a - ft * b) ** 2 for a, b in zip(fq, iq))
    if not Fr(float(eq)) ** 2 >= qerr2:
        bad.append((tag, "stored e_q below the exact error norm", float(eq), float(qerr2) ** 0.5))
    if not Fr(float(eq)) ** 2 <= qerr2 * Fr(1025, 1024) ** 2 + Fr(1, 2 ** 290):
        bad.append((tag, "stored e_q more than 2^-10 above the exact error norm", float(eq), float(qerr2) ** 0.5))
    xerr2 = sum((a - fs * b) ** 2 for a, b in zip(fx, ic))
    if not Fr(float(e)) ** 2 >= xerr2:
        bad.append((tag, "stored e below the exact error norm", float(e), float(xerr2) ** 0.5))
    I = sum(a * b for a, b in zip(iq, ic))
    assert I == int(R8.int_dot(qh, c[None, :])[0]) and abs(I) < 2 ** 34
    with np.errstate(over="ignore"):
        K, qn, rn = O.cosine_parts(q, x)                  # the exact kernel's dot product and the two squared norms, AVX order, f32
        d_exact = O.cosine(q, x)
    P = sum(abs(a * b) for a, b in zip(fq, fx))
    R1 = sum(ft * a * (b - fs * cc) for a, b, cc in zip(iq, fx, ic))   # t qh . (x - s c)
    R2 = sum((a - ft * b) * xx for a, b, xx in zip(fq, iq, fx))        # (q - t qh) . x
    k = dim // 8 + 4; u = Fr(1, 2 ** 24); gam = k * u / (1 - k * u)
    tsI = ft * fs * I
    assert tsI + R1 + R2 == sum(a * b for a, b in zip(fq, fx))         # the decomposition of step (b) is an identity
    e_exact = gam * P + R1 + R2
    args = (I, float(t), float(eq), float(s), float(e), dim, float(qn), float(rn))
    U = np.float32(rf.rf8i_upper(*args)); d_lo = np.float32(rf.rf8i_dlo(*args))
    if np.isfinite(U) and np.isfinite(K):
        if not (Fr(float(K)) <= tsI + e_exact):
            bad.append((tag, "theorem (a)-(b)", float(K), float(tsI), float(e_exact)))
        if not (tsI + e_exact <= Fr(float(U))):
            bad.append((tag, "f32 margin below the exact bound", float(tsI), float(e_exact), float(U)))
        if not (K <= U):
            bad.append((tag, "K > U", float(K), float(U)))
    if np.isfinite(d_lo) and not (d_exact >= d_lo):
        bad.append((tag, "d_exact < d_lo", float(d_exact), float(d_lo)))
    if np.isfinite(d_lo) and np.isfinite(d_exact):   # the verdict can never reject what the exact kernel would admit
        for lb in (d_exact, np.nextafter(d_exact, np.float32(4), dtype=np.float32)):
            if rf.rf_rejects(float(d_lo), float(lb)) and d_exact < lb:
                bad.append((tag, "rejected an admissible neighbour", float(d_exact), float(d_lo), float(lb)))
    return bad, bool(np.isfinite(d_lo))


def _unit(seed, dim):
    return O.normalize(O.fill_normal(seed, (dim,)))


@pytest.mark.parametrize("dim", DIMS)
def test_margin_covers_the_exact_kernel_on_every_adversarial_family(rf, dim):
    bad = []; n = 0; certified = 0
    rng = np.random.default_rng(20261018 + dim)

    def run(q, x, tag, **kw):
        nonlocal bad, n, certified
        b, cert = _check(rf, q, x, tag, **kw)
        bad += b; n += 1; certified += cert

    # random unit rows, random (not normalised) queries
    for t in range(6):
        run(O.fill_normal(100 * dim + t, (dim,)), _unit(7 * dim + t, dim), f"random d{dim} #{t}")
    # all-same-sign: no cancellation, every error adds up
    x = np.abs(_unit(900 + dim, dim)); q = np.abs(O.fill_normal(950 + dim, (dim,)))
    run(q, x, f"same-sign d{dim}"); run(-q, x, f"opposite-sign d{dim}")
    # the query PARALLEL / anti-parallel to the rows' quantisation error x - s c: Cauchy-Schwarz with the stored e is tight
    for t in range(2):
        x = _unit(1200 + dim + t, dim); c, s, e = quantise(x)
        r = (x.astype(np.float64) - np.float64(s) * c.astype(np.float64))
        q = (r / np.linalg.norm(r) * (1.0 if t % 2 == 0 else 37.0)).astype(np.float32)
        run(q, x, f"error-parallel d{dim} #{t}"); run(-q, x, f"error-antiparallel d{dim} #{t}")
    # the ROW parallel / anti-parallel to the QUERY's own quantisation error q - t qh: Cauchy-Schwarz with the stored e_q is tight
    for t in range(2):
        q = O.fill_normal(1300 + dim + t, (dim,)) * np.float32(1.0 if t == 0 else 1e-3)
        tq, qh, _, _, eq = R8.quantise_query(q)
        r = q.astype(np.float64) - np.float64(tq) * qh.astype(np.float64)
        x = (r / np.linalg.norm(r)).astype(np.float32)
        run(q, x, f"query-error-parallel d{dim} #{t}"); run(q, -x, f"query-error-antiparallel d{dim} #{t}")
        # ... and the query parallel to its own error's sign pattern on a dense row
        x = (np.abs(_unit(1350 + dim + t, dim)) * np.where(r >= 0, 1, -1)).astype(np.float32)
        run(q, x, f"query-error-aligned d{dim} #{t}")
    # one-hot queries, against a row that is one-hot there too, and a dense one
    for t in range(2):
        i = int(rng.integers(0, dim))
        q = np.zeros(dim, np.float32); q[i] = 0.75 if t else -2.5
        x = np.zeros(dim, np.float32); x[i] = 1.0
        run(q, x, f"one-hot/one-hot d{dim} #{t}"); run(q, _unit(1900 + dim + t, dim), f"one-hot d{dim} #{t}")
    # a 1e30 outlier element in the query: every other level is 0, e_q carries the rest of the query
    q = O.fill_normal(2000 + dim, (dim,)); q[int(rng.integers(0, dim))] = np.float32(1e30)
    assert np.count_nonzero(R8.quantise_query(q)[1]) == 1
    run(q, _unit(2010 + dim, dim), f"query outlier d{dim}")
    # query norms from 1e-6 to 1e12 (queries are not normalised)
    for t, sc in enumerate((1e-6, 1e-3, 37.0, 1e6, 1e12)):
        run(O.fill_normal(2100 + dim + t, (dim,)) * np.float32(sc), _unit(2150 + dim + t, dim), f"|q| x{sc} d{dim}")
    # near-duplicates of the query: the distances the walk's lowerBound lives among
    for t in range(3):
        x = _unit(2300 + dim + t, dim); q = x + O.fill_normal(2350 + dim + t, (dim,)) * np.float32(1e-3 * 16 ** t)
        run(q, x, f"near d{dim} #{t}")
    # constant-sign SATURATED rows against a constant-sign saturated query: every code +-127, every level +-16256 — |128 H| = 128 * 127 * 127 * dim
    # passes 2^31 at 2304-d (the overflow case of the 32-bit combination); I is the largest the width allows
    for sq, sx in ((1, 1), (1, -1), (-1, -1)):
        q = np.full(dim, 3.0 * sq, np.float32); x = np.full(dim, 0.25 * sx, np.float32)
        _, qh, h, l, _ = R8.quantise_query(q); c, _, _ = quantise(x)
        assert np.all(qh == sq * 16256) and np.all(c == sx * 127) and np.all(l == 0)
        if dim == 2304:
            assert 128 * abs(int(h.astype(np.int64) @ c.astype(np.int64))) > 2 ** 31
        run(q, x, f"saturated {sq}{sx} d{dim}")
    assert n >= 30
    assert certified >= n - 2, "the families above are certifiable (the 1e30 query overflows its squared norm)"
    assert not bad, bad[:10]


def test_nothing_is_certified_for_queries_without_an_error_norm_or_inputs_out_of_range(rf):
    """zero queries, queries with inf / NaN, a scale that underflows: the quantiser gives t = 0, e_q = +inf and the header no verdict; the same for
    rows without an error norm, vanishing or overflowing norms, NaN anywhere"""
    inf = float("inf"); nan = float("nan")
    for q in (np.zeros(256, np.float32), np.r_[np.ones(255, np.float32), np.float32(inf)], np.r_[np.float32(nan), np.ones(255, np.float32)],
              np.r_[np.float32(-inf), np.zeros(767, np.float32)], np.full(256, 1e-45, np.float32)):
        t, qh, h, l, eq = R8.quantise_query(q)
        assert eq == np.inf and t == 0 and not np.any(qh) and not np.any(h) and not np.any(l)
        assert rf.rf8i_scale(float(np.nanmax(np.abs(q))) if np.isfinite(q).all() else 1.0, 0 if np.isfinite(q).all() else 1) == 0
        for I in (0, 1000, -10 ** 10):
            d = rf.rf8i_dlo(I, float(t), float(eq), 0.01, 0.01, q.size, max(float(np.sum(q[np.isfinite(q)] ** 2)), 1.0), 1.0)
            for lb in (-1.0, 0.0, 0.5, 2.0):
                assert not rf.rf_rejects(d, lb), (q[:4], I, d, lb)
    ok = dict(I=1000, t=1e-4, eq=1e-4, s=.01, e=.01, qn=1.0, rn=1.0)
    assert rf.rf_rejects(rf.rf8i_dlo(ok["I"], ok["t"], ok["eq"], ok["s"], ok["e"], 768, ok["qn"], ok["rn"]), -1.0), "the base case of the sweep below is certified"
    for ch in (dict(t=0.0), dict(t=nan), dict(t=inf), dict(t=-1.0), dict(eq=inf), dict(eq=nan), dict(eq=-1.0), dict(s=0.0), dict(s=nan), dict(s=inf), dict(e=inf),
               dict(e=nan), dict(e=-1.0), dict(qn=0.0), dict(qn=1e-20, rn=1e-20), dict(qn=inf), dict(qn=1e30, rn=1e30), dict(qn=nan), dict(rn=nan),
               dict(I=2 ** 40, t=3e38, s=3e38)):
        a = dict(ok, **ch)
        d = rf.rf8i_dlo(a["I"], a["t"], a["eq"], a["s"], a["e"], 768, a["qn"], a["rn"])
        for lb in (-1.0, 0.0, 0.5, 2.0):
            assert not rf.rf_rejects(d, lb), (ch, d, lb)
    assert not rf.rf_rejects(rf.rf8i_dlo(ok["I"], ok["t"], ok["eq"], ok["s"], ok["e"], 16384, 1.0, 1.0), -1.0), "dim beyond ROW_FILTER_MAX_DIM"


def test_the_digits_and_the_error_norm_are_what_the_header_says(rf):
    """every level splits into two signed bytes; e_q from the header's own step equals the restatement's"""
    import ctypes as C
    h, l = C.c_int(0), C.c_int(0)
    for qh in list(range(-16256, -16256 + 300)) + list(range(-300, 300)) + list(range(16256 - 300, 16257)):
        rf.rf8i_digits(qh, C.byref(h), C.byref(l))
        assert 128 * h.value + l.value == qh and -127 <= h.value <= 127 and -64 <= l.value <= 63, qh
    for seed in range(8):
        q = O.fill_normal(3000 + seed, (768,)) * np.float32(10.0 ** (seed - 3))
        t, qh, _, _, eq = R8.quantise_query(q)
        d = q.astype(np.float64) - np.float64(t) * qh.astype(np.float64)
        assert np.float32(rf.rf8i_err(float(np.sum(d * d)))) == eq
        assert np.max(np.abs(qh)) == 16256


def test_the_margin_is_small_enough_to_filter(rf):
    """not a correctness condition — the size the design was reasoned with: the quantised query adds about 1 % to the 8-bit margin of 768-d Gaussian
    rows (e = 0.0076 ||x||, e_q = 6e-5 ||q||)"""
    x = _unit(42, 768); c, s, e = quantise(x)
    q = _unit(43, 768); t, qh, _, _, eq = R8.quantise_query(q)
    assert 0.006 < float(e) < 0.009 and 3e-5 < float(eq) < 1.2e-4
    den = 1.0
    U0 = rf.rf8i_upper(0, float(t), float(eq), float(s), float(e), 768, 1.0, 1.0)
    assert float(e) < U0 < 1.01 * float(e) + 1.5 * float(eq) + 3e-5, (U0, e, eq, den)
