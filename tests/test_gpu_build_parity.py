"""The write path held against a definition, for the instances of hnsw_build_search_kernel<METRIC, QUANT, VISG, R8> and the edges of
hnsw_link_kernel that search parity on a GPU-built graph cannot see (a builder that linked vertices to the wrong neighbours would still
leave a graph whose searches agree with the oracle's walk over that same graph).

Part A: whole-graph equality with the oracle's Hnsw (levels, tombstones, every edge list, stored distance bits, entrypoint, ids) after every
        stage of one sequence: a batched build on a growing schedule, single Inserts, ~15 % Removes, single Inserts, one batch.
Part B: the frozen-graph replay (insert_replay_ref.py, pinned on the CPU by test_insert_replay_ref.py) for cosine x quantised rows, which the
        oracle's f32 index cannot express: one batch of level-0 vectors against a GPU-built graph with tombstones, the own rows from the
        oracle's walk over the arrays copied out of HBM.

The conditions that keep a case from passing vacuously (fan-in, overflows that meet a tombstone, ties) are counted on the reference's side —
the oracle's exports around each batch (Part A), the replay's bookkeeping (Part B) — never on what the GPU returned."""
import numpy as np
import pytest

from oracle import oracle as O
import insert_replay_ref as R
from test_gpu_hnsw import _graph_equal
from util import assert_same_results

pytestmark = pytest.mark.gpu


def _decode(quant, X):
    """the f32 values a quantised index's distance sees: decode(lower(X))"""
    if quant == O.Q_NONE:
        return X
    c = O.lower(quant, X)
    return O.f8_decode(c) if quant == O.Q_F8 else O.f16_decode(c)      # the reference's "bf16" codes are binary16


class Case:
    """One Part A sequence.  n1 vertices in batches of sched(i), n2 single Inserts, 15 % Removes, n4 single Inserts, one batch of n5.
    r8: the index is meant to keep line-transposed rows.  ties: half the rows are copies, and the oracle runs its canonical forms (the literal
    Go heaps have no defined order among equal priorities); every other case runs the literal restatement for single Inserts and Removes,
    which for these seeds gives the same graph as the canonical forms.  fan: the m = 32 fan-in conditions."""

    def __init__(self, name, metric, quant, d, r8, m=16, efc=64, n1=1000, cap=128, n2=40, n4=40, n5=300, seed=1, ties=False, fan=False, sched=None):
        self.name, self.metric, self.quant, self.d, self.r8, self.m, self.efc = name, metric, quant, d, r8, m, efc
        self.n1, self.n2, self.n4, self.n5, self.seed, self.ties, self.fan = n1, n2, n4, n5, seed, ties, fan
        self.sched = sched or (lambda i: max(1, min(cap, i // 16)))
        self.n = n1 + n2 + n4 + n5
        self.canonical = ties

    def data(self):
        X = O.fill_normal(self.seed, (self.n, self.d)); lv = O.levels(self.seed + 1, self.n, self.m)
        if self.ties:   # every odd block of 50 rows repeats the block before it: exact distance ties in selection and prune
            for a in range(50, self.n - 49, 100):
                X[a:a + 50] = X[a - 50:a]
        ids = np.arange(self.n, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
        return X, lv, ids


PART_A = [
    # ------------------------------------------------------------------------------ builder instance <METRIC, QUANT, VISG, R8>
    Case("f32-256d-cosine", O.COSINE, O.Q_NONE, 256, True, seed=9100),                           # <COS, NONE, lds, r8>, 8 lines, 8-bit shadow
    Case("f32-256d-l2", O.L2, O.Q_NONE, 256, True, seed=9110),                                   # <L2, NONE, lds, r8>
    Case("f32-768d-cosine", O.COSINE, O.Q_NONE, 768, True, n1=800, n5=200, seed=9120),           # <COS, NONE, lds, r8>, 24 lines
    Case("f16-77d-l2", O.L2, O.Q_F16, 77, False, seed=9130),                                     # <L2, F16, lds, natural>, scalar tail
    Case("bf16-256d-l2", O.L2, O.Q_BF16, 256, True, seed=9140),                                  # <L2, F16, lds, r8>, 4 lines
    Case("f8-40d-l2", O.L2, O.Q_F8, 40, False, seed=9150),                                       # <L2, F8, lds, natural>
    Case("f32-16d-l2-m4", O.L2, O.Q_NONE, 16, False, m=4, efc=40, seed=9160),                    # <L2, NONE, lds, natural>, mMax0 = 8
    Case("f32-16d-l2-m24", O.L2, O.Q_NONE, 16, False, m=24, efc=80, seed=9170),                  # mMax0 = 48
    Case("f32-16d-l2-m32", O.L2, O.Q_NONE, 16, False, m=32, efc=100, n1=1400, n5=450, seed=1, fan=True,   # mMax0 = 64 = LINK_W
         sched=lambda i: 600 if i >= 800 else max(1, min(64, i // 16))),
    Case("f32-8d-cosine-m8-ties", O.COSINE, O.Q_NONE, 8, False, m=8, efc=48, seed=9180, ties=True),   # <COS, NONE, lds, natural>
    Case("f32-32d-cosine-efc8", O.COSINE, O.Q_NONE, 32, False, efc=8, n5=600, seed=9190),                # result set shorter than m
    Case("f32-48d-l2-efc200", O.L2, O.Q_NONE, 48, False, efc=200, seed=9200),                    # <L2, NONE, hbm, natural>
    Case("f32-256d-cosine-efc200", O.COSINE, O.Q_NONE, 256, True, efc=200, seed=9210),           # <COS, NONE, hbm, r8>
]


def drive(c, gpu=None, log=print):
    """Run the sequence on the oracle and, when `gpu` is the package, on the GPU beside it, comparing after every stage.  Returns the
    oracle-side counts (per-batch max fan-in; overflow / tombstone / tie counts before and after the Removes) and the oracle's last export."""
    X, lv, ids = c.data()
    Xo = _decode(c.quant, X)                         # quantised L2: the oracle indexes the decoded rows, the GPU gets the raw ones
    d = c.d
    oh = O.Hnsw(d, c.metric, O.default_cfg(m=c.m, efConstruction=c.efc), canonical_build=c.canonical)
    gh = xd = None
    if gpu is not None:
        import torch
        gh = gpu.Hnsw(d, c.metric, gpu.HnswCfg.default(m=c.m, ef_construction=c.efc), quantization=c.quant)
        assert gh.cfg.m_max0 == oh.cfg.mMax0 == 2 * c.m and gh.cfg.m_max == oh.cfg.mMax
        xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
    fans, books = [], [{}, {}]                       # books[0]: before the Removes, books[1]: after them
    state = {"g": oh.export(with_vectors=False), "phase": 0}

    def account(batched):
        g = oh.export(with_vectors=False)
        b = R.link_bookkeeping(state["g"], g, oh.cfg.mMax0, oh.cfg.mMax)
        state["g"] = g
        R.add_books(books[state["phase"]], b)
        if batched:
            fans.append(b["max_fan_in"])

    def same(stage):
        if gh is None:
            return
        go = gh.Export()
        assert np.array_equal(go["ids"], state["g"]["ids"]), stage
        try:
            _graph_equal(go, state["g"])
        except AssertionError as e:
            raise AssertionError(f"{c.name}, after {stage}: {e}") from None

    def batch(lo, b):
        oh.insert_batched(ids[lo:lo + b], Xo[lo:lo + b], lv[lo:lo + b], b)
        account(True)
        if gh is not None:
            gh.InsertBatchDevice(xd.data_ptr() + lo * d * 4, b, lv[lo:lo + b], batch=b, ids=ids[lo:lo + b])

    def singles(lo, cnt):
        for i in range(lo, lo + cnt):
            if c.canonical:
                oh.insert_batched(ids[i:i + 1], Xo[i:i + 1], lv[i:i + 1], 1)     # batch == 1 is the sequential canonical Insert
            else:
                assert oh.insert(ids[i], Xo[i], int(lv[i])) == 0                   # the literal restatement (Go heaps)
            account(False)
        if gh is not None:
            gh.InsertBatchDevice(xd.data_ptr() + lo * d * 4, cnt, lv[lo:lo + cnt], batch=1, ids=ids[lo:lo + cnt])

    # 1. batched build, growing schedule
    i = 0
    while i < c.n1:
        b = min(c.sched(i), c.n1 - i)
        batch(i, b); i += b
    same("the batched build")
    if gh is not None:
        assert gh.Rows8()[1] is c.r8, "the layout rule moved this case off its builder instance"
    # 2. single Inserts
    singles(i, c.n2); i += c.n2
    same("the single Inserts")
    # 3. ~15 % Removes: random victims, the entrypoint, and the vertex most rows list without being listed back (its Remove re-prunes only
    #    the rows of its OWN neighbours, so those rows go on listing a tombstone)
    g = state["g"]; first = R.first_rows(g)
    rng = np.random.default_rng(c.seed)
    victims = [int(v) for v in rng.choice(i, int(0.15 * i), replace=False)]
    owner = np.repeat(np.repeat(np.arange(i), g["levels"] + 1), np.diff(g["row_offsets"]))
    fwd = set(zip(owner.tolist(), g["nbr"].tolist()))
    one_way = np.zeros(i, np.int64)
    for a, b_ in fwd:
        if (b_, a) not in fwd:
            one_way[b_] += 1
    lonely = int(np.argmax(one_way))
    assert one_way[lonely] > 0
    for v in (lonely, int(g["entry"])):
        if v in victims:
            victims.remove(v)
    victims.insert(len(victims) // 2, int(g["entry"]))          # removing the entrypoint re-elects one (hnsw.go:197-217)
    victims.append(lonely)
    for v in victims:
        assert oh.remove(ids[v]) == 0
        if gh is not None:
            gh.Remove(ids[v])
    g = state["g"] = oh.export(with_vectors=False); state["phase"] = 1
    listed_dead = int(g["deleted"][g["nbr"]].sum())
    assert g["deleted"][lonely] and (g["nbr"] == lonely).any() and listed_dead > 0     # rows still list tombstones
    same("the Removes")
    if gh is not None:
        assert gh.Len() == len(oh)
    # 4. single Inserts, then one batch
    singles(i, c.n4); i += c.n4
    same("the single Inserts after the Removes")
    batch(i, c.n5); i += c.n5
    same("the batch after the Removes")
    assert i == c.n
    log(f"{c.name}: per-batch max fan-in {max(fans)} (batches > 64: {sum(f > 64 for f in fans)}, > 128: {sum(f > 128 for f in fans)}); "
        f"before the Removes {books[0]}; after {books[1]}; tombstoned entries listed after the Removes {listed_dead}")
    # ---- the conditions, from the oracle's side
    assert books[1]["overflow_with_tombstone"] >= 5, books
    if c.fan:   # the link kernel merges LINK_CH = 64 requests per round: two rounds and three, with a prune in between
        assert any(64 < f <= 128 for f in fans) and any(f > 128 for f in fans), fans
    if c.ties:
        assert books[0]["tie_rows"] + books[1]["tie_rows"] >= 20, books
    # ---- the derived arrays (adj0_n, the line-transposed copy, the shadows) read once after the mutations
    if gh is not None:
        Q = O.fill_normal(c.seed + 2, (16, d)); Qo = _decode(c.quant, Q)
        for ef in (64, 200):
            gi, gs, gc = gh.Search(Q, 10, ef=ef)
            for qi in range(len(Q)):
                wi, ws = oh.search(Qo[qi], 10, mode=1, ef=ef)
                assert_same_results(gi[qi, :gc[qi]], gs[qi, :gc[qi]], wi, ws, f"{c.name} q{qi} ef{ef}")
    return fans, books, state["g"]


@pytest.mark.parametrize("case", PART_A, ids=[c.name for c in PART_A])
def test_build_sequence_equals_oracle(gpu, case):
    drive(case, gpu)


# ------------------------------------------------------------------------------------------------------------------ Part B
# quant, dim, efConstruction, line-transposed                                          builder instance <METRIC, QUANT, VISG, R8>
PART_B = [
    pytest.param(O.Q_F16, 77, 64, False, id="cosine-f16-77d"),                       # <COS, F16, lds, natural>
    pytest.param(O.Q_F16, 768, 200, True, id="cosine-f16-768d-efc200"),              # <COS, F16, hbm, r8>, 12 lines
    pytest.param(O.Q_BF16, 256, 64, True, id="cosine-bf16-256d"),                    # <COS, F16, lds, r8>, 4 lines
    pytest.param(O.Q_F8, 64, 64, False, id="cosine-f8-64d"),                         # <COS, F8, lds, natural>
    pytest.param(O.Q_NONE, 256, 64, True, id="cosine-f32-256d-control"),             # <COS, NONE, lds, r8>: Part A covers it too
]


@pytest.mark.parametrize("quant,d,efc,r8", PART_B)
def test_batch_equals_frozen_graph_replay(gpu, quant, d, efc, r8):
    import torch
    n0, B, m, removes = 1500, 300, 16, 200
    X = O.fill_normal(9300 + d, (n0 + B, d)); lv = O.levels(9301 + d, n0 + B); lv[n0:] = 0
    ids = np.arange(n0 + B, dtype=np.uint64) * np.uint64(3) + np.uint64(7)
    gh = gpu.Hnsw(d, O.COSINE, gpu.HnswCfg.default(ef_construction=efc), quantization=quant)
    assert gh.cfg.m == m
    xd = torch.from_numpy(X).cuda(); torch.cuda.synchronize()
    i = 0
    while i < n0:
        b = min(max(1, min(128, i // 16)), n0 - i)
        gh.InsertBatchDevice(xd.data_ptr() + i * d * 4, b, lv[i:i + b], batch=b, ids=ids[i:i + b])
        i += b
    assert gh.Rows8()[1] is r8
    for v in np.random.default_rng(d).choice(n0, removes, replace=False):
        gh.Remove(ids[v])
    g0 = gh.Export(); raw = gh.ExportRaw(); rows = gh.FetchRows()
    assert raw["entry"] == g0["entry"] and raw["n"] == n0
    # the oracle's walk over the very arrays copied out of HBM: query = the raw new vector (Normalize, Lower, decode, as Insert stores it)
    sl, sc, cn, _, _ = O.csr_search(rows, quant, raw["adj0"], raw["upper_off"], raw["adjU"], d, O.COSINE, raw["entry"], raw["entry_level"],
                                    X[n0:], m, efc, del_bits=R.del_bits(g0["deleted"]), threads=4)
    want, book = R.replay_insert_batch(g0, ids[n0:], sl, sc, cn, m, gh.cfg.m_max0)
    print(f"{quant=} {d=} {efc=}: replay bookkeeping {book}")
    assert book["full_own_rows"] == B and book["overflow"] >= 50 and book["overflow_with_tombstone"] >= 5, book
    gh.InsertBatchDevice(xd.data_ptr() + n0 * d * 4, B, lv[n0:], batch=B, ids=ids[n0:])
    got = gh.Export()
    assert np.array_equal(got["ids"], want["ids"])
    for k in ("levels", "deleted", "row_offsets", "nbr"):
        assert np.array_equal(got[k], want[k]), k
    if not np.array_equal(got["nbr_dist"].view(np.uint32), want["nbr_dist"].view(np.uint32)):
        # same neighbours, other distance bits: the builder's query norm (the stored norms[vi]) and the search's disagree; name the one that
        # differs from the oracle's ||q||^2 of the decoded stored row
        new_rows = _decode_codes(quant, gh.FetchRows(n0, B))
        oracle_qn = np.array([O.cosine_parts(r_, r_)[1] for r_ in new_rows], np.float32)
        bad = np.nonzero(got["nbr_dist"].view(np.uint32) != want["nbr_dist"].view(np.uint32))[0]
        raise AssertionError(f"edge distances differ at {len(bad)} entries (first {bad[:5]}): got {got['nbr_dist'][bad[:5]]}, replay "
                             f"{want['nbr_dist'][bad[:5]]}; the oracle's query norms of the new rows start {oracle_qn[:4]}")
    assert got["entry"] == want["entry"]


def _decode_codes(quant, codes):
    if quant == O.Q_NONE:
        return np.asarray(codes, np.float32)
    return O.f8_decode(codes) if quant == O.Q_F8 else O.f16_decode(codes)
