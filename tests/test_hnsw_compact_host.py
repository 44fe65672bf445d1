"""coltt_hnsw_compact_map_host (no device): the plan of Hnsw.Compact against numpy — new(s) = live slots below s by cumsum, the new upper-row
offsets by a prefix sum over the live levels."""
import numpy as np
import pytest

import coltt_amd as G

NONE = 0xFFFFFFFF
SIZES = [0, 1, 31, 32, 33, 701]


def dead_patterns(n):
    rng = np.random.default_rng(1000 + n)
    pats = {"none": np.zeros(n, bool), "all": np.ones(n, bool)}
    first = np.zeros(n, bool); first[:1] = True
    last = np.zeros(n, bool); last[-1:] = True
    run = np.zeros(n, bool); run[max(0, min(n, 27)):min(n, 38)] = True          # crosses the boundary between words 0 and 1 when n > 32
    pats.update({"slot0": first, "last": last, "run-across-word": run, "random": rng.random(n) < 0.3})
    return pats


def pack(dead):
    words = np.zeros((len(dead) + 31) // 32, np.uint32)
    for s in np.flatnonzero(dead):
        words[s >> 5] |= np.uint32(1) << np.uint32(s & 31)
    return words


def expected(dead, levels):
    live = ~dead
    new_of_old = np.where(live, np.cumsum(live) - live, NONE).astype(np.uint32)
    lv = levels[live].astype(np.int64)
    off = np.where(lv > 0, np.cumsum(lv) - lv, NONE).astype(np.uint32)
    return new_of_old, off, int(live.sum()), int(lv.sum())


@pytest.mark.parametrize("n", SIZES)
def test_compact_map_host_equals_numpy_prefix_sums(n):
    rng = np.random.default_rng(n)
    levels = np.where(rng.random(n) < 0.2, rng.integers(1, 4, n), 0).astype(np.int32)
    for name, dead in dead_patterns(n).items():
        want = expected(dead, levels)
        got = G.compact_map_host(pack(dead), n, levels)
        assert np.array_equal(got[0], want[0]), (n, name, "new_of_old")
        assert np.array_equal(got[1], want[1]), (n, name, "new_upper_off")
        assert got[2:] == want[2:], (n, name, got[2:], want[2:])
    # no bitmap at all = nothing is dead
    got = G.compact_map_host(None, n, levels)
    assert np.array_equal(got[0], np.arange(n, dtype=np.uint32)) and got[2] == n


def test_compact_map_host_survivors_keep_their_order():
    n = 701
    dead = np.random.default_rng(5).random(n) < 0.5
    new_of_old, _, live, _ = G.compact_map_host(pack(dead), n, np.zeros(n, np.int32))
    kept = new_of_old[new_of_old != NONE]
    assert np.array_equal(kept, np.arange(live, dtype=np.uint32))               # monotone, dense
    assert (new_of_old[~dead] <= np.flatnonzero(~dead)).all()                   # new(s) <= s: the in-place sweep's premise


def test_compact_map_host_needs_levels_for_the_upper_rows():
    import ctypes as C
    from coltt_amd._lib import vp
    L = G.lib()
    words = np.zeros(1, np.uint32); up = C.c_uint64(0)
    assert L.coltt_hnsw_compact_map_host(vp(words), C.c_uint64(5), None, None, None, None, C.byref(up)) == -1   # COLTT_E_INVALID
    live = C.c_uint64(0)
    assert L.coltt_hnsw_compact_map_host(vp(words), C.c_uint64(5), None, None, None, C.byref(live), None) == 0 and live.value == 5
