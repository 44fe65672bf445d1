"""The reference of the row-filter probe (tests/row_filter_probe_ref.py) stays inside its own condition: for every width and every family of rows and
queries the GPU test uses, two sums a conforming kernel may form — the fused kernel-order sum (8 partial sums by i % 8 in increasing i, fmaf, the
3-level tree; restated in C) and the exact sum rounded once — lie inside [G_lo, G_hi], for the 8-bit codes and for the binary16 values; and d_lo, as
compiled from the headers, is non-increasing in the shadow sum, which is what turns the interval of sums into an interval of bounds."""
import numpy as np
import pytest

import row_filter_probe_ref as R
from oracle import oracle as O
from row_filter8_ref import quantise


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    return R.compile_headers(tmp_path_factory.mktemp("rfp"))


def _stored(dim):
    """the raw rows as a cosine index stores them, with their 8-bit shadow"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rows = O.normalize(R.raw_rows(dim))
    rows[~np.isfinite(rows).all(axis=1)] = 0
    qz = [quantise(r) for r in rows]
    codes = np.stack([c for c, _, _ in qz]); meta = np.array([[s, e] for _, s, e in qz], np.float32)
    return rows, codes, meta


@pytest.mark.parametrize("dim", R.DIMS)
def test_conforming_sums_lie_inside_the_interval(rf, dim):
    rows, codes, meta = _stored(dim)
    n = len(rows)
    assert n >= 300
    with np.errstate(over="ignore"):
        h16 = rows.astype(np.float16)
    assert np.all(np.isfinite(h16))
    rng = np.random.default_rng(dim)
    hot = R.one_hot_queries(dim)[np.r_[0, 7, 8, dim - 1, rng.integers(0, dim, 12)]]
    dense, _ = R.dense_queries(dim, rows, codes, meta)
    bad = []; seen = 0
    for name, Q, width in (("one-hot", hot, n), ("dense", dense, 64)):
        Qe = O.normalize(Q)
        for qi, q in enumerate(Qe):
            sel = (np.arange(width) + qi * 61) % n
            for kind, sh in (("codes", codes[sel]), ("binary16", h16[sel])):
                lo, hi, S, A = R.sum_interval(q, sh)
                assert np.all(lo <= hi)
                shf = sh.astype(np.float32)
                for j in range(len(sel)):
                    fused = R.fused_kernel_order_sum(rf, q, shf[j]); once = np.float32(S[j])
                    seen += 1
                    if not (lo[j] <= fused <= hi[j]) or not (lo[j] <= once <= hi[j]):
                        bad.append((name, qi, kind, int(sel[j]), float(lo[j]), float(fused), float(once), float(hi[j])))
    assert seen > 2000
    assert not bad, bad[:10]


def test_one_hot_intervals_are_a_few_ulps_wide(rf):
    """A = |S| for a one-hot query: the interval is S rounded outwards and gamma_k |S| either side — what makes the element-mapping check sharp"""
    dim = 1024
    rows, codes, meta = _stored(dim)
    q = O.normalize(R.one_hot_queries(dim)[[3, 500]])
    for qv in q:
        lo, hi, S, A = R.sum_interval(qv, codes[:R.N_RAMP])
        assert np.array_equal(A, np.abs(S))
        k = dim // 8 + 4
        assert np.all(hi.astype(np.float64) - lo.astype(np.float64) <= 2.2 * k * 2.0 ** -24 * np.abs(S) + 2.0 ** -148)
    # the ramp rows are what that check needs: every stored code differs from its neighbours of the same residue
    assert R.distinct_share(codes[:R.N_RAMP]) >= 0.99
    with np.errstate(over="ignore"):
        assert R.distinct_share(rows[:R.N_RAMP].astype(np.float16)) >= 0.99


def test_dlo_is_non_increasing_in_the_shadow_sum(rf):
    rng = np.random.default_rng(7)
    n = 1000
    G1 = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(np.float32)
    G2 = np.where(rng.random(n) < 0.5, R.f32_above(G1), (G1 + np.abs(rng.standard_normal(n)).astype(np.float32) * np.abs(G1)).astype(np.float32))
    s = (10 ** rng.uniform(-5, 0, n)).astype(np.float32); e = (10 ** rng.uniform(-5, 0, n)).astype(np.float32)
    qn = (10 ** rng.uniform(-2, 2, n)).astype(np.float32); rn = (10 ** rng.uniform(-2, 2, n)).astype(np.float32)
    for dim in (256, 1024, 2304):
        a, b = R.dlo8(rf, G1, s, e, dim, qn, rn), R.dlo8(rf, G2, s, e, dim, qn, rn)
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)) and np.all(G1 <= G2)
        assert np.all(a >= b), "row_filter8_dlo is not monotone"
        a, b = R.dlo16(rf, G1, dim, qn, rn), R.dlo16(rf, G2, dim, qn, rn)
        assert np.all(np.isfinite(a)) and np.all(a >= b), "row_filter_dlo is not monotone"
    # the vectorised wrappers are the scalar functions
    for i in range(20):
        assert R.dlo8(rf, G1[i:i + 1], s[i], e[i], 768, qn[i], rn[i])[0] == np.float32(rf.rf8_dlo(float(G1[i]), float(s[i]), float(e[i]), 768, float(qn[i]), float(rn[i])))
        assert R.dlo16(rf, G1[i:i + 1], 768, qn[i], rn[i])[0] == np.float32(rf.rf_dlo(float(G1[i]), 768, float(qn[i]), float(rn[i])))
