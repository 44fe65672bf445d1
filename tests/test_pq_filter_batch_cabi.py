"""coltt_hnsw_pq_search_filtered_batch at the C ABI, without a device: declared in the header, listed by the binding, exported by the
built library, usable from a plain-C translation unit, and an unknown index handle is refused before anything else is looked at."""
import ctypes as C
import os
import shutil
import subprocess

import coltt_amd

SYM = "coltt_hnsw_pq_search_filtered_batch"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "coltt_gpu.h")).read()
    assert f"int {SYM}(coltt_handle_t hnsw, const coltt_handle_t* filters" in hdr
    # the single-filter call no longer lists a filter per query among what is not served
    assert "Not served: device pointers, a filter per query" not in hdr


def test_declared_by_the_binding_and_exported():
    assert SYM in coltt_amd.declared_symbols(), f"{SYM} is not declared in include/coltt_gpu.h"
    L = coltt_amd.lib()
    assert hasattr(L, SYM), f"{SYM} is not exported"
    assert hasattr(coltt_amd.Hnsw, "PqSearchFilteredBatch")


def test_unknown_index_handle_is_not_found():
    L = coltt_amd.lib()
    fn = getattr(L, SYM)
    assert fn(C.c_uint64(987654321), None, None, C.c_size_t(0), C.c_uint32(4), C.c_uint32(0), C.c_uint32(0), C.c_int(0), None, None, None, None, None) == -3
    assert b"unknown index handle" in L.coltt_last_error()


def test_a_plain_c_translation_unit_takes_its_address(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc, "a C compiler is needed"
    src = tmp_path / "takes_address.c"
    src.write_text('#include "coltt_gpu.h"\n'
                   "typedef int (*fn_t)(coltt_handle_t, const coltt_handle_t*, const float*, size_t, uint32_t, uint32_t, uint32_t, int,\n"
                   "                    uint64_t*, float*, uint32_t*, int32_t*, coltt_hnsw_filter_stats*);\n"
                   f"fn_t the_entry_point(void) {{ return &{SYM}; }}\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "takes_address.o")])
