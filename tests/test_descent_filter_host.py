"""The greedy descent through the certified filter (coltt_amd/csrc/hnsw_walk2.hpp: greedy_level8_filtered; COLTT_ROW_FILTER_UPPER) takes the decisions
of the exact descent.  No GPU: row_filter8.hpp / row_filter8i.hpp are compiled with the host compiler, and descent_filter_ref.py replays the descent
over a small layered graph twice — every listed neighbour evaluated exactly, and the headers' bound against curd first, the exact distance only for
what it cannot reject.  The records of (level, cur, curd bits, n_dist, n_hops) after every hop must be EQUAL, on Gaussian rows and on the constructed
cases: a neighbour AT curd (no move), one ulp below it (move), two equal survivors (the lower adjacency index wins), a zero row and a row with a
non-finite element (no verdict: the exact path), a tombstone (skipped, not counted), entry_level == 0, and an entrypoint that is the only upper vertex."""
import numpy as np
import pytest

import descent_filter_ref as D
import row_filter8i_ref as R8
import row_filter_probe_ref as R
from oracle import oracle as O

NONE = D.NONE
KINDS = ("8", "8i")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    return R.compile_headers(tmp_path_factory.mktemp("dflt8")), R8.compile_header(tmp_path_factory.mktemp("dflt8i"))


def _unit(X):
    return np.stack([O.normalize(x) for x in np.ascontiguousarray(X, np.float32)])


def _layered(rows, lv, m):
    """(upper_off, adjU, entry, entry_level): at every level >= 1 a member lists its m nearest members (f64 cosine, non-finite elements read as 0;
    any graph serves the replay)"""
    n = len(rows); lv = np.asarray(lv)
    upper_off = np.zeros(n, np.uint32); nrows = 0
    for v in range(n):
        upper_off[v] = nrows; nrows += int(lv[v])
    adjU = np.full((max(nrows, 1), m), NONE, np.uint32)
    X = np.nan_to_num(rows.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    nr = np.linalg.norm(X, axis=1); nr[nr == 0] = 1.0
    S = (X / nr[:, None]) @ (X / nr[:, None]).T
    for l in range(1, int(lv.max()) + 1):
        mem = np.flatnonzero(lv >= l)
        for v in mem:
            order = [int(u) for u in mem[np.argsort(-S[v, mem], kind="stable")] if u != v][:m]
            adjU[int(upper_off[v]) + l - 1, :len(order)] = order
    entry = int(np.argmax(lv))
    return upper_off, adjU, entry, int(lv[entry])


def _both(libs, sh, graph, Q, deleted=None):
    """the exact and the two filtered replays of every query; returns the summed events and the filtered counters"""
    upper_off, adjU, entry, entry_level = graph
    tot = {}; cnt = {k: np.zeros(3, np.int64) for k in KINDS}
    for qi, q in enumerate(Q):
        qe = O.normalize(q)
        want, ev, _ = D.descend(sh, upper_off, adjU, entry, entry_level, qe, deleted)
        for k, v in ev.items():
            tot[k] = tot.get(k, 0) + v
        for kind in KINDS:
            got, ev2, c = D.descend(sh, upper_off, adjU, entry, entry_level, qe, deleted, D.Bound(kind, libs, sh, qe))
            assert got == want, f"q{qi} kind {kind}: the filtered descent left the exact one at hop {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
            cnt[kind] += np.array(c)
            tot["no_verdict_" + kind] = tot.get("no_verdict_" + kind, 0) + ev2["no_verdict"]
    return tot, cnt


@pytest.mark.parametrize("dim,m", [(256, 4), (768, 4), (512, 16), (1536, 16)])
def test_filtered_descent_equals_exact_on_gaussian_rows(libs, dim, m):
    """M = 4: five or six levels, long descents; M = 16: wide hops.  The filter must have acted (it does not decide anything it cannot prove)"""
    n = 600
    rows = _unit(O.fill_normal(7100 + dim, (n, dim)))
    lv = O.levels(7101 + dim, n, m=m)
    graph = _layered(rows, lv, m)
    assert graph[3] >= (3 if m == 4 else 1)
    sh = D.Shadow(rows)
    Q = O.fill_normal(7102 + dim, (24, dim))
    tot, cnt = _both(libs, sh, graph, Q)
    for kind in KINDS:
        s, r, f = cnt[kind]
        print(f"d{dim} M{m} kind {kind}: {tot['hops']} hops, shadow rows {s}, rejected {r} ({100.0 * r / s:.1f} %), f32 rows {f}")
        assert s > 0 and r > 0 and f < s and r + f == s


def _nudge_to(qe, base, want_bits, rng, tries=40):
    """a copy of `base` with a few elements moved by some ulps whose distance to qe has exactly the bits want_bits"""
    dim = base.size
    for _ in range(tries):
        C = np.tile(base, (4096, 1))
        j = rng.integers(0, dim, 4096); k = rng.integers(-4096, 4097, 4096)
        C[np.arange(4096), j] = (C[np.arange(4096), j].view(np.int32) + k.astype(np.int32)).view(np.float32)
        d = D.exact_distances(qe, C)
        hit = np.flatnonzero(d.view(np.uint32) == np.uint32(want_bits))
        if len(hit):
            return C[hit[0]].copy()
    raise AssertionError("no nudged copy of the row lands on the wanted distance")


def _constructed(dim, seed):
    """rows, levels, queries, deleted: Gaussian filler around groups (A, B...) placed so that the descent stands ON A with B among A's neighbours:
    A lives one level above B, so the first hop of B's top level compares B against the curd handed down from the level above"""
    rng = np.random.default_rng(seed)
    n_fill, groups = 160, 6
    fill = _unit(O.fill_normal(seed, (n_fill, dim)))
    rows = [fill]; lv = [np.minimum(O.levels(seed + 1, n_fill, m=4), 2)]
    Q = []
    for g in range(groups):
        A = _unit(O.fill_normal(seed + 10 + g, (1, dim)))[0]
        q = A + O.fill_normal(seed + 40 + g, (dim,)) * np.float32(2.3 / np.sqrt(dim))   # cos(q, A) about 0.4: d in (0.5, 1), where 1 - cos reaches EVERY f32
        qe = O.normalize(q)
        dA = D.exact_distances(qe, A[None, :])[0]
        kind = g % 3
        if kind == 0:      # B == A: the neighbour's distance EQUALS curd
            B = [A.copy()]
        elif kind == 1:    # B one ulp below curd
            B = [_nudge_to(qe, A, D.f32bits(dA) - 1, rng)]
        else:              # two different rows at the SAME distance below curd: the lower adjacency index wins
            lo = D.f32bits(dA) - 3
            B = [_nudge_to(qe, A, lo, rng), _nudge_to(qe, A, lo, rng)]
            assert not np.array_equal(B[0], B[1])
        rows.append(np.stack([A] + B)); lv.append(np.array([4] + [3] * len(B)))
        Q.append(q)
    zero = np.zeros((1, dim), np.float32)
    bad = _unit(O.fill_normal(seed + 90, (2, dim))); bad[0, 5] = np.float32(np.inf); bad[1, 9] = np.float32(np.nan)
    rows.append(zero); lv.append(np.array([3])); rows.append(bad); lv.append(np.array([3, 4]))
    rows = np.ascontiguousarray(np.concatenate(rows), np.float32); lv = np.concatenate(lv)
    top = len(rows); rows = np.concatenate([rows, _unit(O.fill_normal(seed + 95, (1, dim)))]); lv = np.concatenate([lv, [5]])   # the entrypoint, alone on level 5
    deleted = np.zeros(len(rows), bool)
    deleted[rng.choice(n_fill, 30, replace=False)] = True
    Q = np.ascontiguousarray(np.concatenate([np.stack(Q), O.fill_normal(seed + 96, (12, dim))]), np.float32)
    return rows, lv, Q, deleted, top


@pytest.mark.parametrize("dim", [256, 768])
def test_constructed_cases(libs, dim):
    rows, lv, Q, deleted, top = _constructed(dim, 7300 + dim)
    m = 8
    upper_off, adjU, entry, entry_level = _layered(rows, lv, m)
    assert entry == top and entry_level == 5
    # the rows without a verdict are listed by every level-3 vertex next to them: put them into the groups' adjacency rows by hand
    special = [int(i) for i in np.flatnonzero(~np.isfinite(rows).all(axis=1) | ~rows.any(axis=1))]
    assert len(special) == 3
    for v in np.flatnonzero(lv >= 3):
        if v in special:
            continue
        r = adjU[int(upper_off[v]) + 3 - 1]
        keep = [int(x) for x in r if x != NONE and int(x) not in special][:m - 3]
        r[:] = NONE; r[:len(keep) + 3] = keep + special
    sh = D.Shadow(rows)
    assert not np.isfinite(sh.e[special]).any(), "a zero row and rows with a non-finite element carry no certificate"
    tot, cnt = _both(libs, sh, (upper_off, adjU, entry, entry_level), Q, deleted)
    print(f"d{dim}: events {tot}; counters {cnt}")
    assert tot["equal_no_move"] > 0 and tot["ulp_below_move"] > 0 and tot["tie_of_survivors"] > 0
    assert tot["no_verdict_8"] > 0 and tot["no_verdict_8i"] > 0 and tot["tombstone"] > 0
    for kind in KINDS:
        assert cnt[kind][1] > 0

    # entry_level == 0: nothing to descend — one evaluation, no hop
    flat = (np.zeros(len(rows), np.uint32), np.full((1, m), NONE, np.uint32), 3, 0)
    for kind in KINDS:
        qe = O.normalize(Q[0])
        a = D.descend(sh, *flat, qe)[0]; b = D.descend(sh, *flat, qe, None, D.Bound(kind, libs, sh, qe))[0]
        assert a == b and len(a) == 1 and a[0][3:] == (1, 0)

    # the entrypoint is the only upper vertex: one hop per level over an empty row, no evaluation beyond the entrypoint's own
    lone_lv = np.zeros(len(rows), np.int64); lone_lv[7] = 3
    lone = _layered(rows, lone_lv, m)
    for kind in KINDS:
        qe = O.normalize(Q[1])
        a = D.descend(sh, *lone, qe)[0]; b, _, c = D.descend(sh, *lone, qe, None, D.Bound(kind, libs, sh, qe))
        assert a == b and a[-1][1] == 7 and a[-1][3:] == (1, 3) and c == (0, 0, 0)
