"""coltt_hnsw_carry_bits_host (no device): the definition of a bitmap carried through a compaction — the bits of the live slots, in their order,
repacked — against numpy (tests/carry_ref.py), and the word function (bits_compress, the one the kernel compiles) against a bit loop."""
import ctypes as C

import numpy as np
import pytest

import coltt_amd as G
from coltt_amd._lib import vp

from carry_ref import N_BIG, carry_numpy, dead_patterns, pack

SIZES = [0, 1, 31, 32, 33, 64, N_BIG]


def bitmaps(n, dead, rng):
    """the source bitmaps of one case: dense, sparse, set exactly on the dead slots, all ones with stray bits past n in the ragged word"""
    words = (n + 31) // 32
    out = {"random-half": pack(rng.random(n) < 0.5), "sparse": pack(rng.random(n) < 0.01), "only-dead": pack(dead),
           "ones-and-stray": np.full(words, 0xFFFFFFFF, np.uint32)}
    if words > 1:   # fewer words than the slots need: the coverage lies below n
        out["short"] = pack(rng.random(n) < 0.5)[:words // 2].copy()
        out["short-by-one"] = np.full(words - 1, 0xFFFFFFFF, np.uint32)
    out["no-words"] = np.zeros(0, np.uint32)
    return out


@pytest.mark.parametrize("n", SIZES)
def test_carry_bits_host_equals_numpy(n):
    rng = np.random.default_rng(n + 17)
    for pname, dead in dead_patterns(n).items():
        dw = pack(dead)
        for bname, b in bitmaps(n, dead, rng).items():
            want = carry_numpy(b, dead, n)
            got = G.carry_bits_host(b, dw, n)
            assert got[1:] == want[1:], (n, pname, bname, got[1:], want[1:])
            assert np.array_equal(got[0], want[0]), (n, pname, bname)
            if bname == "only-dead":
                assert got[1] == 0                      # a bit on a dead slot does not survive
            if bname == "ones-and-stray":
                assert got[1] == got[2]                 # ... nor one past n_slots: exactly the live slots
    # no tombstone bitmap at all = nothing is dead
    b = pack(rng.random(n) < 0.5)
    got = G.carry_bits_host(b, None, n)
    assert np.array_equal(got[0], b) and got[2] == n


def test_tombstone_words_past_the_slots_and_stray_tombstone_bits_are_ignored():
    n = 45
    dead = np.zeros(64, bool); dead[3] = True; dead[50] = True     # slot 50 does not exist
    b = np.full(2, 0xFFFFFFFF, np.uint32)
    out, allowed, live = G.carry_bits_host(b, pack(dead), n)
    assert (allowed, live) == (44, 44) and np.array_equal(out, pack(np.ones(44, bool)))


def test_the_word_function_against_a_bit_loop():
    """n_slots = 32: out word = bits_compress(x, m) with m = the live slots of the one word"""
    L = G.lib()
    rng = np.random.default_rng(99)
    N = 100_000
    xs = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    ms = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
    # every density of mask, and the corners
    ms[:N // 4] &= rng.integers(0, 1 << 32, N // 4, dtype=np.uint64).astype(np.uint32)
    ms[N // 4:N // 2] |= rng.integers(0, 1 << 32, N // 4, dtype=np.uint64).astype(np.uint32)
    xs[:4] = [0xFFFFFFFF, 0xFFFFFFFF, 0, 0x80000001]; ms[:4] = [0xFFFFFFFF, 0, 0xFFFFFFFF, 0x80000001]
    # the bit loop, vectorised over the pairs: walk the 32 positions, append the selected bit at the running count
    want = np.zeros(N, np.uint32); cnt = np.zeros(N, np.uint32)
    for j in range(32):
        sel = (ms >> np.uint32(j)) & np.uint32(1)
        bit = (xs >> np.uint32(j)) & np.uint32(1)
        want |= (bit & sel) << cnt
        cnt += sel
    x1 = np.zeros(1, np.uint32); d1 = np.zeros(1, np.uint32); o1 = np.zeros(1, np.uint32)
    al = C.c_uint64(0); lv = C.c_uint64(0)
    fn = L.coltt_hnsw_carry_bits_host
    px, pd, po, n32, one = vp(x1), vp(d1), vp(o1), C.c_uint64(32), C.c_uint64(1)
    got = np.zeros(N, np.uint32); lives = np.zeros(N, np.uint32)
    for i in range(N):
        x1[0] = xs[i]; d1[0] = ~ms[i]; o1[0] = 0
        assert fn(px, one, pd, n32, po, C.byref(al), C.byref(lv)) == 0
        got[i] = o1[0]; lives[i] = lv.value
    assert np.array_equal(lives, cnt)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(hex(xs[i]), hex(ms[i]), hex(got[i]), hex(want[i])) for i in bad[:5]]


def test_argument_checks():
    L = G.lib()
    assert L.coltt_hnsw_carry_bits_host(None, C.c_uint64(3), None, C.c_uint64(64), None, None, None) == -1        # NULL bits with words
    lv = C.c_uint64(0); al = C.c_uint64(7)
    assert L.coltt_hnsw_carry_bits_host(None, C.c_uint64(0), None, C.c_uint64(64), None, C.byref(al), C.byref(lv)) == 0
    assert (al.value, lv.value) == (0, 64)                                                                       # every output may be NULL
    assert L.coltt_hnsw_carry_bits_host(None, C.c_uint64(0), None, C.c_uint64(1 << 31), None, None, None) == -4  # COLTT_E_UNSUPPORTED
