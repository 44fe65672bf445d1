"""The level-0 row filter over the 8-bit shadow with a QUANTISED QUERY ("8i": coltt_amd/csrc/row_filter8i.hpp; rows8.hpp: query_digits8i,
group8_burst_bi / group8_stream_bi; hnsw_walk2.hpp: Group8FilterEval<.., ROW_FILTER_8I>) changes what a search computes in phase A, never what it
answers.  One index keeps both shadows and answers the same call with the filter off, over the 8-bit shadow with the f32 query and with the quantised
one: ids, score bits, counts and the traversal counters equal the oracle's and each other's.  Through the probe (coltt_hnsw_row_filter_probe_ex) the
integer sum of every (query, slot) pair EQUALS numpy's exact integer dot product of the restated digits and the fetched codes, and the bound is the
header's own function of that integer."""
import numpy as np
import pytest

import row_filter8i_ref as R8
import row_filter_probe_ref as R
import test_gpu_row_filter8 as T8
from oracle import oracle as O
from util import bits

pytestmark = pytest.mark.gpu

BIG = np.float32(3e38)
NONE = np.uint32(R.NBR_NONE)
SIDES = ("off", "8", "8i")
SHAPES = [(256, 5000), (768, 3000), (512, 2000), (1536, 1500)]   # phase A: one burst of 2 lines | one burst of 6 | stream of bursts of 2 | stream of bursts of 6


@pytest.fixture(autouse=True)
def _throughput_kernels(monkeypatch):
    monkeypatch.setenv("COLTT_MW_MAX_NQ", "0")   # batches of any size on the one-wave-per-query kernels (the latency kernel is not filtered)
    for k in T8.KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("COLTT_ROW_SHADOW_BITS", "both")


@pytest.fixture(scope="module")
def rf8i(tmp_path_factory):
    return R8.compile_header(tmp_path_factory.mktemp("rf8i_gpu"))


@pytest.fixture(scope="module")
def rf(tmp_path_factory):
    return R.compile_headers(tmp_path_factory.mktemp("rf8_gpu"))


_WALKS = {}


def _walk_case(gpu, d, n):
    """the Gaussian index of this width (both shadows) and its queries — built once, shared by the two load hints"""
    if d not in _WALKS:
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("COLTT_ROW_SHADOW_BITS", "both")
            X = O.fill_normal(8000 + d, (n, d)); lv = O.levels(8001 + d, n)
            gh = T8._gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=60), batch=256)
        assert gh.RowFilterStats()["shadow_bits"] == (8, 16)
        _WALKS[d] = (gh, O.fill_normal(8002 + d, (48, d)))
    return _WALKS[d]


def _host_bounds(rf, rf8i, gh, Q, n_rows=64, seed=5):
    """d_lo of both kinds on the CPU for every query against n_rows stored rows: (d_lo of the f32-query bound, d_lo of the quantised-query bound)"""
    rows = gh.FetchRows(); codes, meta, _ = gh.FetchShadow8()
    sel = np.random.default_rng(seed).choice(len(rows), n_rows, replace=False)
    Qe = O.normalize(Q)
    a = np.empty((len(Q), n_rows), np.float32); b = np.empty_like(a)
    for i, q in enumerate(Qe):
        qn = O.cosine_parts(q, q)[1]
        rn = np.array([O.cosine_parts(rows[j], rows[j])[1] for j in sel], np.float32)
        G = np.array([R.fused_kernel_order_sum(rf, q, codes[j].astype(np.float32)) for j in sel], np.float32)
        a[i] = R.dlo8(rf, G, meta[sel, 0], meta[sel, 1], gh.dim, qn, rn)
        t, qh, _, _, eq = R8.quantise_query(q)
        b[i] = R8.dlo8i(rf8i, R8.int_dot(qh, codes[sel]), t, eq, meta[sel, 0], meta[sel, 1], gh.dim, qn, rn)
    return a, b


@pytest.mark.parametrize("nt", ["0", "1"], ids=["default-loads", "non-temporal-twins"])
@pytest.mark.parametrize("d,n", SHAPES)
def test_three_sides_equal_the_oracle(gpu, rf, rf8i, monkeypatch, d, n, nt):
    """ef 32 / 128 on the LDS-hash kernel, 256 on the HBM-visited one (walk variants 6 / 7)"""
    monkeypatch.setenv("COLTT_ROWS_NT", nt)
    gh, Q = _walk_case(gpu, d, n)
    if nt == "0":
        # the convention asserted below, checked on the CPU first: on these fixtures the quantised-query bound is (almost) never above the f32-query
        # one — its margin grows by e_q (||x|| + e), Cauchy-Schwarz's worst case, while t s I differs from s G by e_q ||x|| / sqrt(dim) or so
        a, b = _host_bounds(rf, rf8i, gh, Q)
        both = np.isfinite(a) & np.isfinite(b)
        above = np.count_nonzero(b[both] > a[both])
        print(f"d{d}: host d_lo of {both.sum()} pairs: quantised-query bound above the f32-query bound for {above}; mean gap {np.mean(a[both] - b[both]):.3e}")
        assert both.sum() > 0.9 * a.size and above <= both.sum() // 100
    seen = T8._check(gh, Q, (32, 128, 256), monkeypatch, sides=SIDES)
    for ef in (32, 128, 256):
        f8, f8i = seen[(ef, "8")], seen[(ef, "8i")]
        assert f8["shadow_rows"] == f8i["shadow_rows"], (ef, f8, f8i)   # the same walk meets the same full-set neighbours whichever phase A it runs
        assert f8i["rejected"] > 0
        assert f8i["rejected"] <= f8["rejected"] + f8["shadow_rows"] // 100, (ef, f8, f8i)
        print(f"d{d} ef{ef}: survivors 8: {f8['shadow_rows'] - f8['rejected']}, 8i: {f8i['shadow_rows'] - f8i['rejected']} of {f8['shadow_rows']} shadow rows")


def test_an_unset_knob_takes_the_quantised_query(gpu, monkeypatch):
    """COLTT_ROW_FILTER_BITS unset on an index that keeps the 8-bit shadow: a filtered launch runs the integer phase A (the documented default).  The
    two 8-bit kinds are told apart by their counters: on this fixture the quantised-query bound leaves a few more survivors than the f32-query one"""
    gh, Q = _walk_case(gpu, 256, 5000)
    r = T8._sides(gh, Q, 10, 128, monkeypatch, sides=("off", "8", "8i"))
    assert r["8"][1]["rejected"] != r["8i"][1]["rejected"], "the fixture does not tell the two 8-bit kinds apart"
    monkeypatch.setenv("COLTT_ROW_FILTER", "1")
    a = gh.RowFilterStats(); res = gh.Search(Q, 10, ef=128, with_stats=True); b = gh.RowFilterStats()
    got = {k: b[k] - a[k] for k in ("rejected", "f32_rows", "shadow_rows", "launches")}
    assert got == r["8i"][1], (got, r["8"][1], r["8i"][1])
    for x, y in zip(res[:3], r["off"][0][:3]):
        assert np.array_equal(bits(x) if x.dtype == np.float32 else x, bits(y) if y.dtype == np.float32 else y)


def test_ties_and_near_ties_with_lower_bound(gpu, monkeypatch):
    """the construction of test_gpu_row_filter8.py: every base vector stored six times — exact duplicates and copies that differ in one low bit of one
    or two elements — queried by those vectors and small perturbations of them.  No shadow can tell such rows from the set's worst member: they reach
    the exact f32 evaluation, and admissions at d == lowerBound and one ulp either side of it come out as the oracle's"""
    d, nb, copies = 256, 400, 6
    rng = np.random.default_rng(99)
    base = O.fill_normal(8300, (nb, d))
    base /= np.linalg.norm(base, axis=1, keepdims=True).astype(np.float32)
    X = np.repeat(base, copies, axis=0)
    for i in range(len(X)):
        c = i % copies
        if c % 3 == 1:
            j = int(rng.integers(0, d)); X[i, j] = np.nextafter(X[i, j], np.float32(4), dtype=np.float32)
        elif c % 3 == 2:
            for j in rng.integers(0, d, 2):
                X[i, j] = np.nextafter(X[i, j], np.float32(-4), dtype=np.float32)
    X = X[rng.permutation(len(X))]
    lv = O.levels(8301, len(X))
    gh = T8._gpu_build(gpu, X, lv, gpu.HnswCfg.default(ef_construction=80), batch=64)
    Q = np.concatenate([base[:16], base[16:32] + O.fill_normal(8302, (16, d)) * np.float32(1e-4), O.fill_normal(8303, (16, d))])
    T8._check(gh, Q, (32, 64, 128, 256), monkeypatch, k=20, sides=("off", "8i"), want_survivors=True)


# ---- the probe: what phase A sums, and the bound formed from it ------------------------------------------------------------------------------------
PROBE_DIMS = (256, 768, 512, 1536, 2304)   # the four forms of phase A, and the width at which 128 H leaves 32 bits
_CASES = {}


def _probe_case(gpu, dim):
    if dim in _CASES:
        return _CASES[dim]
    import torch
    X = R.raw_rows(dim)
    n = len(X)
    lv = O.levels(9100 + dim, n)
    with pytest.MonkeyPatch.context() as mp:
        for k in T8.KNOBS:
            mp.delenv(k, raising=False)
        mp.setenv("COLTT_ROW_SHADOW_BITS", "both")
        gh = gpu.Hnsw(dim, O.COSINE, gpu.HnswCfg.default(ef_construction=24), quantization=O.Q_NONE)
        xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
        i = 0
        while i < n:
            b = int(min(n - i, max(1, min(64, i // 16))))
            gh.InsertBatchDevice(xd.data_ptr() + i * dim * 4, b, lv[i:i + b], batch=b, first_id=i)
            i += b
    rows = gh.FetchRows(); codes, meta, _ = gh.FetchShadow8()
    assert rows.shape == (n, dim) and n % 32 == 0
    c = {"gh": gh, "dim": dim, "n": n, "rows": rows, "codes": codes, "meta": meta}
    nch = n // 32
    sat = [int(i) for i in range(n) if np.all(np.abs(codes[i]) == 127) and np.all(codes[i] == codes[i][0])]   # the constant rows: every code +-127
    assert sat, "raw_rows holds constant rows"
    Qd, _ = R.dense_queries(dim, rows, codes, meta)
    Qd = np.concatenate([Qd, np.ones((1, dim), np.float32), -np.ones((1, dim), np.float32), np.zeros((1, dim), np.float32)])   # saturated queries; a zero query
    qsel, slots = [], []
    for j in range(len(Qd)):
        for ch in (sat[0] // 32 if j >= len(Qd) - 3 else j % nch, (3 + 5 * j) % nch):
            qsel.append(j); slots.append(np.arange(32 * ch, 32 * ch + 32, dtype=np.uint32))
    c["dense"] = (np.ascontiguousarray(Qd[qsel]), np.stack(slots))
    hot = R.one_hot_queries(dim)
    c["hot"] = (hot, np.tile(np.arange(32, dtype=np.uint32), (dim, 1)))
    c["sat"] = sat
    _CASES[dim] = c
    return c


def _same(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def _check_pairs(rf8i, c, Q, slots, nt, tag):
    gh, dim = c["gh"], c["dim"]
    ex, qn, rn, cnt_e = gh.RowFilterProbe(Q, slots, BIG, bits="8i", nt=nt)
    dl, qn2, rn2, cnt_d, isum, qte = gh.RowFilterProbe(Q, slots, -BIG, bits="8i", nt=nt, sums=True)
    assert np.array_equal(bits(qn), bits(qn2)) and np.array_equal(bits(rn), bits(rn2))
    assert np.all(cnt_e == np.array([0, 32, 32], np.uint32)), cnt_e[:4]
    Qe = O.normalize(Q)
    want_I = np.empty(slots.shape, np.int64); d_exact = np.empty(slots.shape, np.float32)
    n_eq_diff = 0
    for i in range(len(Q)):
        t, qh, _, _, eq = R8.quantise_query(Qe[i])
        assert np.float32(qte[i, 0]).view(np.uint32) == np.float32(t).view(np.uint32), f"{tag} q{i}: scale {qte[i, 0]} != {t}"
        if np.isfinite(eq):   # the device sums the squared differences in another order: the same conditions as the restatement, not its bits
            exact = float(np.linalg.norm(Qe[i].astype(np.float64) - np.float64(t) * qh.astype(np.float64)))
            assert exact <= float(qte[i, 1]) <= exact * (1 + 2.0 ** -10) + 1e-300, f"{tag} q{i}: e_q {qte[i, 1]} against {exact}"
            n_eq_diff += int(np.float32(qte[i, 1]).view(np.uint32) != np.float32(eq).view(np.uint32))
        else:
            assert qte[i, 1] == np.inf and qte[i, 0] == 0
        want_I[i] = R8.int_dot(qh, c["codes"][slots[i]])
        d_exact[i] = O.dist_rows(O.COSINE, Qe[i], c["rows"][slots[i]])
    okx = _same(ex, d_exact)
    assert okx.all(), f"{tag}: {np.count_nonzero(~okx)} exact distances differ from the oracle's"
    assert np.array_equal(isum, want_I), f"{tag}: integer sums differ at {np.argwhere(isum != want_I)[:6].tolist()}: {isum[isum != want_I][:6]} != {want_I[isum != want_I][:6]}"
    s, e = c["meta"][slots, 0], c["meta"][slots, 1]
    t2 = np.broadcast_to(qte[:, :1], slots.shape); e2 = np.broadcast_to(qte[:, 1:], slots.shape); qn_b = np.broadcast_to(qn[:, None], slots.shape)
    want = R8.dlo8i(rf8i, isum, t2, e2, s, e, dim, qn_b, rn)   # the header on the host, from the device's integers and (t, e_q)
    cert = np.isfinite(want)
    exact_back = _same(dl, ex)
    # (a certified bound that happens to carry the exact distance's bits would be counted as uncertified here; the counters below say it was not)
    assert np.array_equal(exact_back | cert, np.ones_like(cert)) and np.array_equal(cnt_d[:, 0], np.count_nonzero(cert, axis=1)), f"{tag}: certified set"
    assert _same(dl[cert], want[cert]).all(), (f"{tag}: d_lo differs from the header's value for {np.count_nonzero(~_same(dl[cert], want[cert]))} pairs, first "
                                               f"{[(float(a), float(b)) for a, b in zip(dl[cert][~_same(dl[cert], want[cert])][:4], want[cert][~_same(dl[cert], want[cert])][:4])]}")
    assert np.all(dl[cert] <= d_exact[cert]), f"{tag}: d_lo above the exact distance"
    print(f"{tag}: {cert.size} pairs, {np.count_nonzero(~cert)} without a certificate; max |I| {np.abs(isum).max()}; e_q bits differ from the restatement's for {n_eq_diff} queries")
    return ex, dl, isum, cert


PARAMS = [(nt, d) for d in PROBE_DIMS for nt in (0, 1)]


@pytest.mark.parametrize("nt,dim", PARAMS, ids=[f"nt{nt}-d{d}" for nt, d in PARAMS])
def test_the_kernel_sums_the_integers_the_proof_assumes(gpu, rf8i, nt, dim):
    c = _probe_case(gpu, dim)
    gh = c["gh"]
    # ---- element mapping: a one-hot query has ONE non-zero level (16256 = digits (127, 0)): I = +-16256 * that code of each ramp row
    Qh, Sh = c["hot"]
    if dim > 768:   # every 3rd element still visits every residue, every line and every dword of a line
        Qh, Sh = Qh[::3], Sh[::3]
    _check_pairs(rf8i, c, Qh, Sh, nt, f"d{dim} nt{nt} one-hot")
    # ---- dense queries, the saturated pair, a zero query
    Q, S = c["dense"]
    ex, dl, isum, cert = _check_pairs(rf8i, c, Q, S, nt, f"d{dim} nt{nt} dense")
    assert cert.any() and (~cert).any()
    assert not cert[-2:].any(), "a zero query has no certificate"
    sat_I = 127 * 16256 * dim
    assert np.abs(isum).max() == sat_I, "the saturated query met the saturated row"
    if dim == 2304:
        assert 128 * 127 * 127 * dim > 2 ** 31 and sat_I > 2 ** 31

    # ---- with the set still filling up: every fresh neighbour straight to the exact stream
    r0, _, _, cnt0 = gh.RowFilterProbe(Q, S, np.float32(0.9), bits="8i", nt=nt, full_at_pop=0)
    assert _same(r0, ex).all() and np.all(cnt0 == np.array([0, 32, 0], np.uint32))

    # ---- chunk shapes: the same pairs through every count of fresh neighbours, masks with holes, a slot twice
    nq = len(Q)
    for qi in (0, nq // 2, nq - 6):
        q = Q[qi]; full = S[qi]
        med = np.float32(np.median(ex[qi][np.isfinite(ex[qi])]))
        variants = []
        for nf in (0, 1, 7, 8, 9, 16, 17, 25, 31, 32):
            v = np.full(32, NONE, np.uint32); v[:nf] = full[:nf]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[::2] = full[::2]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[1::2] = full[1::2]; variants.append(v)
        v = np.full(32, NONE, np.uint32); v[[0, 31]] = full[[0, 31]]; variants.append(v)
        v = full.copy(); v[9] = full[2]; v[31] = full[2]; variants.append(v)           # the same slot three times
        v = np.full(32, NONE, np.uint32); v[[4, 20]] = full[11]; variants.append(v)    # ... and twice with nothing else
        V = np.stack(variants); QV = np.tile(q, (len(V), 1))
        for lb in (BIG, -BIG, med):
            rfull, _, _, _, ifull, _ = gh.RowFilterProbe(q[None, :], full[None, :], lb, bits="8i", nt=nt, sums=True)
            assert np.array_equal(ifull[0], isum[qi])
            r_of = {int(s): rfull[0, p] for p, s in enumerate(full)}; i_of = {int(s): ifull[0, p] for p, s in enumerate(full)}
            rv, _, _, cv, iv, _ = gh.RowFilterProbe(QV, V, lb, bits="8i", nt=nt, sums=True)
            for vi, v in enumerate(V):
                fresh = v != NONE
                want = np.array([r_of[int(s)] if s != NONE else np.float32(0) for s in v], np.float32)
                assert _same(rv[vi], want).all(), f"d{dim} nt{nt} q{qi} lb{lb} variant {vi}: {np.flatnonzero(~_same(rv[vi], want)).tolist()}"
                assert np.array_equal(iv[vi], np.array([i_of[int(s)] if s != NONE else 0 for s in v], np.int64)), f"d{dim} nt{nt} q{qi} lb{lb} variant {vi}: sums"
                nf = int(np.count_nonzero(fresh))
                assert int(cv[vi][2]) == nf and int(cv[vi][0]) + int(cv[vi][1]) == nf

    # ---- the verdict: a neighbour the exact kernel would admit always comes back exact; a rejected one carries a bound in [lower_bound, d_exact]
    for qi in (1, nq // 3):
        q = Q[qi]; sl = S[qi]; de = ex[qi]
        fin = np.flatnonzero(np.isfinite(de))
        m = fin[len(fin) // 2]
        lbs = np.concatenate([[np.float32(np.median(de[fin])), R.f32_below(de[m]), de[m], R.f32_above(de[m])], de[fin]]).astype(np.float32)
        rv, _, _, cv = gh.RowFilterProbe(np.tile(q, (len(lbs), 1)), np.tile(sl, (len(lbs), 1)), lbs, bits="8i", nt=nt)
        n_rej_seen = 0
        for li, lb in enumerate(lbs):
            came_exact = _same(rv[li], de)
            assert came_exact[de < lb].all(), f"d{dim} nt{nt} q{qi} lb {lb}: admissible neighbours came back with a bound"
            rej = ~came_exact
            assert np.all((rv[li][rej] >= lb) & (rv[li][rej] <= de[rej])), (float(lb), rv[li][rej], de[rej])
            assert tuple(cv[li]) == (np.count_nonzero(rej), 32 - np.count_nonzero(rej), 32)
            n_rej_seen += int(np.count_nonzero(rej))
        assert n_rej_seen > 0


def test_the_probe_refuses_what_it_cannot_serve(gpu):
    c = _probe_case(gpu, 256)
    gh = c["gh"]
    q = c["dense"][0][:1]; sl = c["dense"][1][:1].copy()
    with pytest.raises(Exception):
        gh.RowFilterProbe(q, sl, 0.5, bits=8, sums=True)
    sl[0, 3] = c["n"]   # one past the last slot
    with pytest.raises(Exception):
        gh.RowFilterProbe(q, sl, 0.5, bits="8i")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("COLTT_ROW_SHADOW_BITS", "16")
        g16 = gpu.Hnsw(256, O.COSINE)
        g16.Insert(0, c["rows"][40], 0)
        with pytest.raises(Exception):
            g16.RowFilterProbe(q, np.zeros((1, 32), np.uint32), 0.5, bits="8i")
