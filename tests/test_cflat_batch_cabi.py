"""coltt_cflat_search_batch and coltt_cflat_get at the C ABI, without a device: declared in the header, exported, and an unknown
handle is refused before anything else is looked at."""
import ctypes as C

import coltt_amd


def test_batch_and_get_are_declared_and_exported():
    L = coltt_amd.lib()
    syms = coltt_amd.declared_symbols()    # test_cabi.py's export check walks this list
    for s in ("coltt_cflat_search_batch", "coltt_cflat_get"):
        assert s in syms, f"{s} is not declared in include/coltt_gpu.h"
        assert hasattr(L, s), f"{s} is not exported"


def test_unknown_handle_is_not_found():
    L = coltt_amd.lib()
    h = C.c_uint64(987654321)
    buf = (C.c_float * 8)()
    assert L.coltt_cflat_get(h, C.c_uint64(1), buf) == -3
    assert b"unknown handle" in L.coltt_last_error()
    q = (C.c_float * 8)(); r = (C.c_uint32 * 2)(); inc = (C.c_uint8 * 2)(); oi = (C.c_uint64 * 4)(); os_ = (C.c_float * 4)(); oc = (C.c_uint32 * 1)()
    assert L.coltt_cflat_search_batch(h, q, r, inc, C.c_size_t(1), C.c_uint32(4), oi, os_, oc) == -3
    assert b"unknown handle" in L.coltt_last_error()


def test_empty_batch_on_an_unknown_handle_is_still_not_found():
    L = coltt_amd.lib()
    assert L.coltt_cflat_search_batch(C.c_uint64(987654321), None, None, None, C.c_size_t(0), C.c_uint32(4), None, None, None) == -3
