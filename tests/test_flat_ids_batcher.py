"""The micro-batcher for FLAT filtered searches (include/coltt_batcher.hpp: IdsBatcher over FlatIdsBackend = coltt_flat_search_ids_batch):
tests/cpp/flat_ids_batcher_test.cpp drives it from 32 threads, each with its own candidate list, on the GPU — every caller its own direct
call's answer, shared batches, k = 0 and refused calls isolated."""
import os
import shutil
import subprocess

import pytest

pytestmark = pytest.mark.gpu


def test_cpp_ids_batcher_over_the_flat_store(gpu, tmp_path):
    import torch
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the C++ consumer"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(gpu.lib_path())
    exe = tmp_path / "flat_ids_batcher_test"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-pthread", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "flat_ids_batcher_test.cpp"), "-o", str(exe), "-L", libdir, "-lcoltt_gpu", f"-Wl,-rpath,{libdir}"])
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(os.path.dirname(torch.__file__), "lib") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([str(exe)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "flat ids batcher ok" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
