"""coltt_flat_search_ids_batch without a device: the three symbols are declared and exported, the tile plan of the one-pass path
(coltt_flat_ids_plan_host — the code the search itself calls) covers every (query, position of its list) pair exactly once with tiles
that never cross a list, and the argument errors that need no device are refused."""
import ctypes as C

import numpy as np
import pytest

import coltt_amd

SYMS = ("coltt_flat_search_ids_batch", "coltt_flat_ids_batch_stats", "coltt_flat_ids_plan_host")
E_INVALID, E_NOT_FOUND = -1, -3


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def plan(lens, list_of, nq, chunk, qpt, cap=None):
    L = coltt_amd.lib()
    lens = np.ascontiguousarray(lens, np.uint64)
    lo = None if list_of is None else np.ascontiguousarray(list_of, np.uint32)
    if cap is None:
        n = C.c_uint64(0)
        order = np.zeros(max(nq, 1), np.uint32)
        L.coltt_flat_ids_plan_host(vp(lens), C.c_size_t(len(lens)), vp(lo), C.c_size_t(nq), C.c_uint32(chunk), C.c_uint32(qpt), None, vp(order),
                                   C.c_uint64(0), C.byref(n))
        cap = n.value
    guard = 7
    tiles = np.full((cap + guard, 5), 0xDEADBEEF, np.uint32)
    order = np.full(nq + guard, 0xDEADBEEF, np.uint32)
    n = C.c_uint64(0)
    rc = L.coltt_flat_ids_plan_host(vp(lens), C.c_size_t(len(lens)), vp(lo), C.c_size_t(nq), C.c_uint32(chunk), C.c_uint32(qpt), vp(tiles), vp(order),
                                    C.c_uint64(cap), C.byref(n))
    assert (tiles[cap:] == 0xDEADBEEF).all() and (order[nq:] == 0xDEADBEEF).all(), "the planner wrote past its buffers"
    return rc, tiles[:cap], order[:nq], n.value


def closed_form(lens, list_of, nq, chunk, qpt):
    lo = np.arange(nq) if list_of is None else np.asarray(list_of, np.int64)
    per = np.bincount(lo, minlength=len(lens))
    return int(sum(-(-int(n) // chunk) * -(-int(c) // qpt) for n, c in zip(lens, per)))


def check_plan(lens, list_of, nq, chunk, qpt):
    tag = (list(map(int, lens)), None if list_of is None else list(map(int, list_of)), chunk, qpt)
    rc, tiles, order, n = plan(lens, list_of, nq, chunk, qpt)
    assert rc == 0, (coltt_amd.lib().coltt_last_error(), tag)
    assert n == len(tiles) == closed_form(lens, list_of, nq, chunk, qpt), tag
    lo = np.arange(nq) if list_of is None else np.asarray(list_of, np.int64)
    assert sorted(order.tolist()) == list(range(nq)), tag             # every query appears once, the queries of empty lists included
    assert (np.diff(lo[order]) >= 0).all(), tag                       # ... ordered by list
    seen = {}
    for l, s0, s1, q0, g in tiles.tolist():
        assert 0 <= s0 < s1 <= lens[l], tag                           # inside ONE list, never empty
        assert s1 - s0 <= chunk and s0 % chunk == 0 and s0 % 32 == 0, tag
        assert s1 == lens[l] or s1 % 32 == 0, tag                     # every chunk boundary but a list's last is a multiple of 32
        assert 1 <= g <= qpt and q0 + g <= nq, tag
        qs = order[q0:q0 + g]
        assert (lo[qs] == l).all(), tag                               # one list per tile
        for q in qs.tolist():
            cov = seen.setdefault(q, np.zeros(int(lens[l]), np.int32))
            cov[s0:s1] += 1
    for q in range(nq):
        if lens[lo[q]] == 0:
            assert q not in seen, tag                                 # an empty list has no tile
        else:
            assert q in seen and (seen[q] == 1).all(), tag            # every (query, position) pair exactly once


def test_symbols_are_declared_and_exported():
    L = coltt_amd.lib()
    syms = coltt_amd.declared_symbols()
    for s in SYMS:
        assert s in syms, f"{s} is not declared in include/coltt_gpu.h"
        assert hasattr(L, s), f"{s} is not exported"


@pytest.mark.parametrize("qpt", [1, 4, 8])
@pytest.mark.parametrize("chunk", [32, 96, 256, 4096])
def test_plan_covers_every_pair_exactly_once(chunk, qpt):
    rng = np.random.default_rng(chunk * 16 + qpt)
    edge = [0, 1, 31, 32, 33, chunk - 1, chunk, chunk + 1, 3 * chunk, 3 * chunk + 5]
    for trial in range(6):
        n_lists = int(rng.integers(1, 14))
        lens = np.array([edge[int(rng.integers(len(edge)))] if rng.random() < 0.7 else int(rng.integers(0, 5 * chunk)) for _ in range(n_lists)], np.uint64)
        nq = int(rng.integers(1, 40))
        popular = rng.integers(0, n_lists)                            # a popular filter: many queries share one list, some lists stay unnamed
        list_of = np.where(rng.random(nq) < 0.5, popular, rng.integers(0, n_lists, nq)).astype(np.uint32)
        check_plan(lens, list_of, nq, chunk, qpt)
    lens = np.array(edge, np.uint64)
    check_plan(lens, None, len(lens), chunk, qpt)                     # list_of = NULL: query i uses list i
    check_plan(np.zeros(3, np.uint64), np.array([2, 2, 0], np.uint32), 3, chunk, qpt)   # only empty lists: no tile, every query still ordered


def test_a_cap_that_is_too_small_is_reported_and_respected():
    lens = np.array([100, 0, 70], np.uint64); list_of = np.array([0, 2, 2, 0, 0], np.uint32)
    want = closed_form(lens, list_of, 5, 32, 1)
    rc, tiles, order, n = plan(lens, list_of, 5, 32, 1, cap=want - 3)  # plan() checks the guard rows behind cap
    assert rc == E_INVALID and n == want and b"cap" in coltt_amd.lib().coltt_last_error()
    full = plan(lens, list_of, 5, 32, 1)
    assert full[0] == 0 and np.array_equal(tiles, full[1][:want - 3]) and np.array_equal(order, full[2])


def test_plan_argument_errors():
    L = coltt_amd.lib()
    lens = np.array([10, 20], np.uint64); order = np.zeros(4, np.uint32); tiles = np.zeros((64, 5), np.uint32); n = C.c_uint64(0)

    def call(lens_, n_lists, list_of, nq, chunk, qpt, tiles_=tiles, order_=order, n_=C.byref(n)):
        return L.coltt_flat_ids_plan_host(vp(lens_), C.c_size_t(n_lists), vp(list_of), C.c_size_t(nq), C.c_uint32(chunk), C.c_uint32(qpt),
                                          vp(tiles_), vp(order_), C.c_uint64(64), n_)
    lo = np.array([0, 1, 1], np.uint32)
    assert call(lens, 2, lo, 3, 32, 4) == 0
    assert call(lens, 2, lo, 3, 33, 4) == E_INVALID and b"multiple of 32" in L.coltt_last_error()
    assert call(lens, 2, lo, 3, 0, 4) == E_INVALID
    assert call(lens, 2, lo, 3, 32, 0) == E_INVALID
    assert call(lens, 2, None, 3, 32, 4) == E_INVALID and b"n_lists" in L.coltt_last_error()
    assert call(lens, 2, np.array([0, 1, 2], np.uint32), 3, 32, 4) == E_INVALID and b"list_of[2]" in L.coltt_last_error()
    assert call(None, 2, lo, 3, 32, 4) == E_INVALID
    assert call(lens, 2, lo, 3, 32, 4, order_=None) == E_INVALID
    assert call(lens, 2, lo, 3, 32, 4, tiles_=None) == E_INVALID
    assert call(lens, 2, lo, 3, 32, 4, n_=None) == E_INVALID


def test_unknown_handle_is_refused_before_anything_else():
    L = coltt_amd.lib()
    h = C.c_uint64(987654321)
    q = (C.c_float * 8)(); off = (C.c_uint64 * 2)(0, 1); cand = (C.c_uint64 * 1)(5)
    oi = (C.c_uint64 * 4)(); os_ = (C.c_float * 4)(); oc = (C.c_uint32 * 1)()
    assert L.coltt_flat_search_ids_batch(h, q, C.c_size_t(1), C.c_uint32(4), 1, cand, off, C.c_size_t(1), None, oi, os_, oc) == E_NOT_FOUND
    assert b"unknown handle" in L.coltt_last_error()
    # ... before the NULL checks, the empty batch and the k / select checks
    assert L.coltt_flat_search_ids_batch(h, None, C.c_size_t(1), C.c_uint32(4), 1, None, None, C.c_size_t(1), None, None, None, None) == E_NOT_FOUND
    assert L.coltt_flat_search_ids_batch(h, None, C.c_size_t(0), C.c_uint32(0), 7, None, None, C.c_size_t(0), None, None, None, None) == E_NOT_FOUND
    a = C.c_uint64(0)
    assert L.coltt_flat_ids_batch_stats(h, C.byref(a), None, None) == E_NOT_FOUND and b"unknown handle" in L.coltt_last_error()
