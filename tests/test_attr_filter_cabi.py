"""The attribute-column entry points at the C ABI, without a device: declared in the header, listed by the binding, exported by the built
library, reachable from the Python classes, usable from a plain-C translation unit, and an unknown index or column handle is refused before
anything else is looked at."""
import ctypes as C
import os
import shutil
import subprocess

import coltt_amd

SYMS = ["coltt_hnsw_attr_create", "coltt_hnsw_attr_destroy", "coltt_hnsw_attr_set", "coltt_hnsw_attr_get", "coltt_hnsw_attr_info",
        "coltt_hnsw_filter_eval_attr", "coltt_hnsw_filter_eval_attr_batch", "coltt_attr_cmp_host"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_FOUND = -3
BAD = C.c_uint64(987654321)


def test_declared_in_the_header():
    hdr = open(os.path.join(ROOT, "include", "coltt_gpu.h")).read()
    for s in SYMS:
        assert f"int {s}(" in hdr, s
    for name, v in (("COLTT_ATTR_I64", 0), ("COLTT_ATTR_F64", 1), ("COLTT_CMP_EQ", 0), ("COLTT_CMP_NE", 1), ("COLTT_CMP_GT", 2), ("COLTT_CMP_GE", 3),
                    ("COLTT_CMP_LT", 4), ("COLTT_CMP_LE", 5), ("COLTT_CMP_SET", 6)):
        assert f"#define {name} {v}" in hdr, name
    assert "} coltt_attr_pred;" in hdr


def test_declared_by_the_binding_exported_and_reachable():
    L = coltt_amd.lib()
    for s in SYMS:
        assert s in coltt_amd.declared_symbols(), f"{s} is not declared in include/coltt_gpu.h"
        assert hasattr(L, s), f"{s} is not exported"
    for name in ("AttrColumn", "FilterEvalAttr", "FilterEvalAttrBatch"):
        assert hasattr(coltt_amd.Hnsw, name), name
    for name in ("set", "get", "info", "close"):
        assert hasattr(coltt_amd.HnswAttrColumn, name), name
    assert (coltt_amd.ATTR_I64, coltt_amd.ATTR_F64) == (0, 1)
    assert (coltt_amd.CMP_EQ, coltt_amd.CMP_NE, coltt_amd.CMP_GT, coltt_amd.CMP_GE, coltt_amd.CMP_LT, coltt_amd.CMP_LE, coltt_amd.CMP_SET) == tuple(range(7))


def test_unknown_handles_are_not_found_before_anything_else():
    L = coltt_amd.lib()
    h = C.c_uint64(0)
    # an unknown index: NULL out, an unknown type, NULL programmes and NULL preds with n_preds > 0 are all behind it
    assert L.coltt_hnsw_attr_create(BAD, C.c_int(99), None) == NOT_FOUND and b"unknown index handle" in L.coltt_last_error()
    assert L.coltt_hnsw_filter_eval_attr(BAD, None, C.c_size_t(0), None, C.c_size_t(3), None, C.c_size_t(2), None, None) == NOT_FOUND
    assert b"unknown index handle" in L.coltt_last_error()
    assert L.coltt_hnsw_filter_eval_attr_batch(BAD, None, None, C.c_size_t(5), None, C.c_size_t(3), None, C.c_size_t(2), None, None) == NOT_FOUND
    assert b"unknown index handle" in L.coltt_last_error()
    # an unknown column
    assert L.coltt_hnsw_attr_destroy(BAD) == NOT_FOUND and b"unknown column handle" in L.coltt_last_error()
    assert L.coltt_hnsw_attr_set(BAD, None, None, C.c_size_t(4), None) == NOT_FOUND and b"unknown column handle" in L.coltt_last_error()
    assert L.coltt_hnsw_attr_get(BAD, None, C.c_size_t(4), None, None) == NOT_FOUND and b"unknown column handle" in L.coltt_last_error()
    assert L.coltt_hnsw_attr_info(BAD, None, None, None, None) == NOT_FOUND and b"unknown column handle" in L.coltt_last_error()
    assert h.value == 0


def test_the_predicate_is_24_bytes_on_both_sides(tmp_path):
    assert C.sizeof(coltt_amd.AttrPred) == 24
    assert (coltt_amd.AttrPred.column.offset, coltt_amd.AttrPred.op.offset, coltt_amd.AttrPred.reserved.offset, coltt_amd.AttrPred.value.offset) == (0, 8, 12, 16)
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc, "a C compiler is needed"
    src = tmp_path / "size.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "coltt_gpu.h"\n'
                   'int main(void) { printf("%d %d %d %d %d\\n", (int)sizeof(coltt_attr_pred), (int)offsetof(coltt_attr_pred, column), (int)offsetof(coltt_attr_pred, op),\n'
                   "                        (int)offsetof(coltt_attr_pred, reserved), (int)offsetof(coltt_attr_pred, value)); return 0; }\n")
    exe = tmp_path / "size"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"24", b"0", b"8", b"12", b"16"]


def test_a_plain_c_translation_unit_fills_a_predicate_and_takes_the_addresses(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    assert gcc, "a C compiler is needed"
    src = tmp_path / "takes_address.c"
    src.write_text('#include "coltt_gpu.h"\n'
                   "coltt_attr_pred a_predicate(coltt_handle_t column) {\n"
                   "  coltt_attr_pred p;\n"
                   "  p.column = column; p.op = COLTT_CMP_LT; p.reserved = 0; p.value.f64 = 37.5;\n"
                   "  return p;\n"
                   "}\n"
                   "coltt_attr_pred an_integer_predicate(coltt_handle_t column) {\n"
                   "  coltt_attr_pred p;\n"
                   "  p.column = column; p.op = COLTT_CMP_GE; p.reserved = 0; p.value.i64 = 5;\n"
                   "  return p;\n"
                   "}\n"
                   "typedef int (*create_t)(coltt_handle_t, int, coltt_handle_t*);\n"
                   "typedef int (*destroy_t)(coltt_handle_t);\n"
                   "typedef int (*set_t)(coltt_handle_t, const uint64_t*, const void*, size_t, uint64_t*);\n"
                   "typedef int (*get_t)(coltt_handle_t, const uint64_t*, size_t, void*, uint8_t*);\n"
                   "typedef int (*info_t)(coltt_handle_t, coltt_handle_t*, int32_t*, uint64_t*, uint64_t*);\n"
                   "typedef int (*eval_t)(coltt_handle_t, const int32_t*, size_t, const coltt_handle_t*, size_t, const coltt_attr_pred*, size_t, uint64_t*, coltt_handle_t*);\n"
                   "typedef int (*batch_t)(coltt_handle_t, const int32_t*, const uint64_t*, size_t, const coltt_handle_t*, size_t, const coltt_attr_pred*, size_t,\n"
                   "                       uint64_t*, coltt_handle_t*);\n"
                   "typedef int (*cmp_t)(int, int, const void*, const void*, int);\n"
                   "create_t e0(void) { return &coltt_hnsw_attr_create; }\n"
                   "destroy_t e1(void) { return &coltt_hnsw_attr_destroy; }\n"
                   "set_t e2(void) { return &coltt_hnsw_attr_set; }\n"
                   "get_t e3(void) { return &coltt_hnsw_attr_get; }\n"
                   "info_t e4(void) { return &coltt_hnsw_attr_info; }\n"
                   "eval_t e5(void) { return &coltt_hnsw_filter_eval_attr; }\n"
                   "batch_t e6(void) { return &coltt_hnsw_filter_eval_attr_batch; }\n"
                   "cmp_t e7(void) { return &coltt_attr_cmp_host; }\n")
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "takes_address.o")])
