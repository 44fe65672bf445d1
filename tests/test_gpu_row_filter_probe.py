"""What the GPU sums per pair.  The row filter rejects a neighbour on a proof; the margin half of the proof is checked against exact rationals on the
CPU (test_row_filter_bound.py, test_row_filter8_bound.py), the other half is a premise about the kernels: that phase A forms sum q_i * c_i over the
RIGHT element pairs of the RIGHT row, with the RIGHT row's norm and (scale, error norm), for every width the dispatch in Group8FilterEval::filtered
treats differently.  coltt_hnsw_row_filter_probe makes one call of that very function on chosen (query, slot) pairs and hands back what the walk
would have been handed; tests/row_filter_probe_ref.py says what a conforming kernel may return (an interval that follows from the headers' own
derivation, no tolerance of this test's).  Everything is computed from what ingest stored (FetchRows, FetchShadow8).

One index per width (both shadows), shared by the parametrisations over the shadow read and the load hint.

A cosine index normalises what it stores and what it is asked: the rows scaled to 1e-15 / 1e15 and the queries scaled by 1e-6 ... 1e6 reach the
kernels as unit vectors, and the row with a 1e30 element is stored as a zero row (its squared norm overflows).  The pairs without a certificate are
therefore those of the zero rows; the check of the certified set is written against the headers' full conditions all the same."""
import numpy as np
import pytest

import row_filter_probe_ref as R
from oracle import oracle as O
from util import bits

pytestmark = pytest.mark.gpu

KNOBS = ("COLTT_ROW_FILTER", "COLTT_ROW_FILTER_BITS", "COLTT_ROW_SHADOW", "COLTT_ROW_SHADOW_BITS")
BIG = np.float32(3e38)
NONE = np.uint32(R.NBR_NONE)
NSQ_LO, NSQ_HI = np.float32(2.0 ** -100), np.float32(3.0e38)   # the headers' range of qnorm * rnorm


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    return R.compile_headers(tmp_path_factory.mktemp("rfp_gpu"))


_CASES = {}


def _case(gpu, dim):
    """the index of this width, what it stored, the queries and their host references — built once"""
    if dim in _CASES:
        return _CASES[dim]
    import torch
    X = R.raw_rows(dim)
    n = len(X)
    lv = O.levels(9100 + dim, n)
    with pytest.MonkeyPatch.context() as mp:
        for k in KNOBS:
            mp.delenv(k, raising=False)
        mp.setenv("COLTT_ROW_SHADOW_BITS", "both")
        gh = gpu.Hnsw(dim, O.COSINE, gpu.HnswCfg.default(ef_construction=24), quantization=O.Q_NONE)
        xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
        i = 0
        while i < n:
            b = int(min(n - i, max(1, min(64, i // 16))))
            gh.InsertBatchDevice(xd.data_ptr() + i * dim * 4, b, lv[i:i + b], batch=b, first_id=i)
            i += b
    assert gh.RowFilterStats()["shadow_bits"] == (8, 16)
    rows = gh.FetchRows(); codes, meta, _ = gh.FetchShadow8()
    assert rows.shape == (n, dim) and n % 32 == 0
    with np.errstate(over="ignore"):
        h16 = rows.astype(np.float16)
    c = {"gh": gh, "dim": dim, "n": n, "rows": rows, "codes": codes, "meta": meta, "h16": h16, "h16_ok": np.isfinite(h16).all(axis=1)}
    nch = n // 32
    # element mapping: dim one-hot queries against the chunk of ramp rows
    Qh = R.one_hot_queries(dim)
    c["hot"] = _refs(c, Qh, np.tile(np.arange(32, dtype=np.uint32), (dim, 1)))
    # sum and bound: dense queries, each against three chunks (the chunk of the row it was derived from first)
    Qd, src = R.dense_queries(dim, rows, codes, meta)
    qsel, slots = [], []
    for j in range(len(Qd)):
        first = int(src[j]) // 32 if src[j] >= 0 else j % nch
        for ch in (first, (first + 3 + j) % nch, (first + 7 + 2 * j) % nch):
            qsel.append(j); slots.append(np.arange(32 * ch, 32 * ch + 32, dtype=np.uint32))
    c["dense"] = _refs(c, Qd[qsel], np.stack(slots))
    _CASES[dim] = c
    return c


def _refs(c, Q, slots):
    """per (query, position): the oracle's exact distance and the intervals of conforming shadow sums over the codes and over the binary16 values"""
    Qe = O.normalize(Q)
    nq = len(Q)
    out = {"Q": np.ascontiguousarray(Q, np.float32), "slots": np.ascontiguousarray(slots, np.uint32),
           "d_exact": np.empty((nq, 32), np.float32), "qn": np.empty(nq, np.float32)}
    for kind in ("8", "16"):
        out["lo" + kind] = np.zeros((nq, 32), np.float32); out["hi" + kind] = np.zeros((nq, 32), np.float32)
    for i in range(nq):
        sl = slots[i]
        out["d_exact"][i] = O.dist_rows(O.COSINE, Qe[i], c["rows"][sl])
        out["qn"][i] = O.cosine_parts(Qe[i], Qe[i])[1]
        out["lo8"][i], out["hi8"][i], _, _ = R.sum_interval(Qe[i], c["codes"][sl])
        ok = c["h16_ok"][sl]
        lo, hi, _, _ = R.sum_interval(Qe[i], c["h16"][sl][ok])
        out["lo16"][i, ok] = lo; out["hi16"][i, ok] = hi
    return out


def _same(a, b):
    """the same f32 bits (any NaN equals any NaN: the payload of 0 / 0 is the platform's, not the kernel's)"""
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def _uncertified(c, kind, slots, qn, rn):
    """the pairs the headers give no verdict for — by their own conditions, from what the index stored and the norms the probe reported"""
    with np.errstate(over="ignore", invalid="ignore"):
        nsq = (qn[:, None] * rn).astype(np.float32)
    out = ~((nsq >= NSQ_LO) & (nsq <= NSQ_HI))
    inside = ~out
    # every other norm product stays a factor 2^10 away from the two thresholds: the set below is then the same under any rounding of nsq
    assert np.all((nsq[inside] >= NSQ_LO * np.float32(1024)) & (nsq[inside] <= NSQ_HI / np.float32(1024)))
    if kind == 8:
        out |= ~np.isfinite(c["meta"][slots, 1])
    else:
        out |= ~c["h16_ok"][slots]   # row_filter.hpp (c): an element beyond binary16's range makes the sum infinite or NaN
    return out


def _dlo_interval(rf, c, kind, ref, qn, rn):
    """[dlo(G_hi), dlo(G_lo)] per pair with the norms the probe reported and the stored (s, e)"""
    sl = ref["slots"]; qn2 = np.broadcast_to(qn[:, None], sl.shape)
    if kind == 8:
        s, e = c["meta"][sl, 0], c["meta"][sl, 1]
        return R.dlo8(rf, ref["hi8"], s, e, c["dim"], qn2, rn), R.dlo8(rf, ref["lo8"], s, e, c["dim"], qn2, rn)
    return R.dlo16(rf, ref["hi16"], c["dim"], qn2, rn), R.dlo16(rf, ref["lo16"], c["dim"], qn2, rn)


def _two_calls(c, ref, kind, nt):
    """lower_bound = +3e38: every pair through phase B (the exact kernel's distance); -3e38: every certified pair rejected (its d_lo)"""
    gh = c["gh"]
    ex, qn, rn, cnt_e = gh.RowFilterProbe(ref["Q"], ref["slots"], BIG, bits=kind, nt=nt)
    dl, qn2, rn2, cnt_d = gh.RowFilterProbe(ref["Q"], ref["slots"], -BIG, bits=kind, nt=nt)
    assert np.array_equal(bits(qn), bits(qn2)) and np.array_equal(bits(rn), bits(rn2))
    assert np.array_equal(bits(qn), bits(ref["qn"])), "the probe's queries are not prepared as Search prepares them"
    assert np.all(cnt_e == np.array([0, 32, 32], np.uint32)), cnt_e[:4]
    return ex, dl, qn, rn, cnt_d


def _check_pairs(rf, c, ref, kind, nt, tag):
    ex, dl, qn, rn, cnt_d = _two_calls(c, ref, kind, nt)
    # the exact side: phase B hands every lane ITS neighbour's distance, the oracle's bits
    okx = _same(ex, ref["d_exact"])
    assert okx.all(), f"{tag}: {np.count_nonzero(~okx)} exact distances differ from the oracle's, first at {np.argwhere(~okx)[:5].tolist()}"
    # which pairs came back with the exact bits from the call that rejects everything it can
    exact_back = _same(dl, ex)
    unc = _uncertified(c, kind, ref["slots"], qn, rn)
    print(f"{tag}: {unc.size} pairs, {np.count_nonzero(unc)} without a certificate, {np.count_nonzero(exact_back)} came back exact")
    assert np.array_equal(exact_back, unc), f"{tag}: certified set differs at {np.argwhere(exact_back != unc)[:8].tolist()}"
    assert np.array_equal(cnt_d[:, 0], np.count_nonzero(~unc, axis=1)) and np.all(cnt_d[:, 2] == 32) and np.all(cnt_d[:, 0] + cnt_d[:, 1] == 32)
    cert = ~unc
    lo, hi = _dlo_interval(rf, c, kind, ref, qn, rn)
    assert np.all(np.isfinite(lo[cert])) and np.all(np.isfinite(hi[cert])) and np.all(lo[cert] <= hi[cert])
    inside = (dl >= lo) & (dl <= hi)
    width = (hi[cert].astype(np.float64) - lo[cert]).max() if cert.any() else 0.0
    print(f"{tag}: widest interval of d_lo {width:.3e}; outside: {np.count_nonzero(cert & ~inside)} of {np.count_nonzero(cert)}")
    bad = np.argwhere(cert & ~inside)
    assert not len(bad), (f"{tag}: d_lo outside what a conforming sum allows for {len(bad)} pairs, first (query, position) {bad[:6].tolist()}: "
                          f"{[(float(lo[i, j]), float(dl[i, j]), float(hi[i, j])) for i, j in bad[:3]]}")
    below = dl <= ref["d_exact"]
    assert below[cert].all(), f"{tag}: d_lo above the exact distance at {np.argwhere(cert & ~below)[:6].tolist()}"
    return ex, dl, unc


PARAMS = [(b, nt, d) for d in R.DIMS for b in (8, 16) for nt in (0, 1)]


@pytest.mark.parametrize("kind,nt,dim", PARAMS, ids=[f"{b}bit-nt{nt}-d{d}" for b, nt, d in PARAMS])
def test_the_kernel_sums_what_the_proof_assumes(gpu, rf, kind, nt, dim):
    c = _case(gpu, dim)
    gh = c["gh"]
    # ---- element mapping: a one-hot query sees ONE code of each row; A = |S|, the interval is a few ulps wide
    vals = c["codes"][:R.N_RAMP] if kind == 8 else c["h16"][:R.N_RAMP]
    share = R.distinct_share(vals)
    print(f"d{dim} {kind} bits: {100 * share:.2f} % of the ramp rows' (element, row) pairs differ from every same-residue value within 64 elements")
    assert share >= 0.99
    assert bits(O.cosine(O.normalize(c["hot"]["Q"][5]), c["rows"][3])) == bits(c["hot"]["d_exact"][5, 3])
    _check_pairs(rf, c, c["hot"], kind, nt, f"d{dim} {kind}b nt{nt} one-hot")
    # ---- sum and bound, the certified set
    ref = c["dense"]
    ex, dl, unc = _check_pairs(rf, c, ref, kind, nt, f"d{dim} {kind}b nt{nt} dense")
    assert unc.any() and (~unc).any()
    nq = len(ref["Q"])

    # ---- with the set still filling up: every fresh neighbour straight to the exact stream
    r0, _, _, cnt0 = gh.RowFilterProbe(ref["Q"], ref["slots"], np.float32(0.9), bits=kind, nt=nt, full_at_pop=0)
    assert _same(r0, ex).all() and np.all(cnt0 == np.array([0, 32, 0], np.uint32))

    # ---- chunk shapes: the same pairs through every count of fresh neighbours, masks with holes, a slot twice
    for qi in (0, nq // 2, nq - 1):
        q = ref["Q"][qi]; full = ref["slots"][qi]
        fin = np.isfinite(ex[qi])
        med = np.float32(np.median(ex[qi][fin]))
        variants = []
        for nf in (0, 1, 7, 8, 9, 15, 16, 17, 24, 25, 31, 32):
            v = np.full(32, NONE, np.uint32); v[:nf] = full[:nf]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[::2] = full[::2]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[1::2] = full[1::2]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[31] = full[31]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[[0, 31]] = full[[0, 31]]; variants.append(v)
        v = full.copy(); v[9] = full[2]; v[31] = full[2]; variants.append(v)           # the same slot three times
        v = np.full(32, NONE, np.uint32); v[[4, 20]] = full[11]; variants.append(v)    # ... and twice with nothing else
        V = np.stack(variants); QV = np.tile(q, (len(V), 1))
        for lb in (BIG, -BIG, med):
            rfull, _, _, _ = gh.RowFilterProbe(q[None, :], full[None, :], lb, bits=kind, nt=nt)
            want_of = {int(s): rfull[0, p] for p, s in enumerate(full)}
            rv, _, _, cv = gh.RowFilterProbe(QV, V, lb, bits=kind, nt=nt)
            for vi, v in enumerate(V):
                fresh = v != NONE
                want = np.array([want_of[int(s)] if s != NONE else np.float32(0) for s in v], np.float32)
                assert _same(rv[vi], want).all(), f"d{dim} {kind}b nt{nt} q{qi} lb{lb} variant {vi}: {np.flatnonzero(~_same(rv[vi], want)).tolist()}"
                assert np.all(bits(rv[vi][~fresh]) == 0), "a position without a fresh neighbour did not come back 0"
                nf = int(np.count_nonzero(fresh))
                came_exact = _same(rv[vi], np.array([ex[qi][list(full).index(s)] if s != NONE else 0 for s in v], np.float32)) & fresh
                n_rej = nf - int(np.count_nonzero(came_exact))
                assert tuple(cv[vi]) == ((n_rej, nf - n_rej, nf) if nf else (0, 0, 0)), (vi, tuple(cv[vi]), n_rej, nf)

    # ---- the verdict: a neighbour the exact kernel would admit always comes back exact; a rejected one carries a bound in [lower_bound, d_exact]
    for qi in (1, nq // 3, nq - 2):
        q = ref["Q"][qi]; sl = ref["slots"][qi]; de = ex[qi]
        fin = np.flatnonzero(np.isfinite(de))
        m = fin[len(fin) // 2]
        lbs = np.concatenate([[np.float32(np.median(de[fin])), R.f32_below(de[m]), de[m], R.f32_above(de[m])], de[fin]]).astype(np.float32)
        rv, _, _, cv = gh.RowFilterProbe(np.tile(q, (len(lbs), 1)), np.tile(sl, (len(lbs), 1)), lbs, bits=kind, nt=nt)
        n_rej_seen = 0
        for li, lb in enumerate(lbs):
            came_exact = _same(rv[li], de)
            must = de < lb
            assert came_exact[must].all(), f"d{dim} {kind}b nt{nt} q{qi} lb {lb}: admissible neighbours came back with a bound at {np.flatnonzero(must & ~came_exact).tolist()}"
            rej = ~came_exact
            assert np.all((rv[li][rej] >= lb) & (rv[li][rej] <= de[rej])), (float(lb), rv[li][rej], de[rej])
            assert tuple(cv[li]) == (np.count_nonzero(rej), 32 - np.count_nonzero(rej), 32), (tuple(cv[li]), np.count_nonzero(rej))
            n_rej_seen += int(np.count_nonzero(rej))
        print(f"d{dim} {kind}b nt{nt} q{qi}: {len(lbs)} lower bounds, {n_rej_seen} rejections")
        assert n_rej_seen > 0


def test_the_probe_refuses_what_it_cannot_serve(gpu):
    c = _case(gpu, 256)
    gh = c["gh"]
    q = c["dense"]["Q"][:1]; sl = c["dense"]["slots"][:1].copy()
    with pytest.raises(Exception):
        gh.RowFilterProbe(q, sl, 0.5, bits=4)
    sl[0, 3] = c["n"]   # one past the last slot
    with pytest.raises(Exception):
        gh.RowFilterProbe(q, sl, 0.5, bits=8)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("COLTT_ROW_SHADOW_BITS", "16")
        g16 = gpu.Hnsw(256, O.COSINE)
        g16.Insert(0, c["rows"][40], 0)
        with pytest.raises(Exception):
            g16.RowFilterProbe(q, np.zeros((1, 32), np.uint32), 0.5, bits=8)
        r, _, _, cnt = g16.RowFilterProbe(q, np.zeros((1, 32), np.uint32), BIG, bits=16)
        assert np.all(bits(r) == bits(r[0, 0])) and tuple(cnt[0]) == (0, 32, 32)
