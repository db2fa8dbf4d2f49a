"""Launches in two parts without a GPU: the host bookkeeping (madronalib_amd/csrc/launch_parts.cpp, plain C++ driven by
tests/cpp/launch_parts_test.cpp under the address and undefined-behaviour sanitizers) and the entry points as the header declares
them."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
C_TO_CTYPES = {"mlgpu_engine*": ctypes.c_void_p, "uint64_t*": ctypes.POINTER(ctypes.c_uint64), "int": ctypes.c_int}
DECLARED = {
    "mlgpu_engine_set_launch_parts": ("int", ["e", "parts"]),
    "mlgpu_engine_get_launch_parts": ("int", ["e"]),
    "mlgpu_engine_launch_parts_possible": ("int", ["e"]),
    "mlgpu_engine_launch_stats": ("int", ["e", "split_launches", "joins"]),
}


def test_bookkeeping_on_the_cpu_under_sanitizers(tmp_path):
    """launch_parts.cpp is plain C++: built by g++ from that one file with no HIP include path, as a stand-alone program with
    -fsanitize=address,undefined. Where a bank is cut in each mode; which launch follows pending ones with no join and which does
    not (tests/cpp/launch_parts_test.cpp)."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "launch_parts_test")
    src = os.path.join(CSRC, "launch_parts.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "launch_parts_test.cpp"), src, "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", src], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "launch_parts.hpp" in used
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_entry_points_are_exported_and_declared_like_the_header():
    from madronalib_amd import _lib
    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mlgpu.h")).read(), flags=re.S)
    for name, (res, want_names) in DECLARED.items():
        fn = getattr(L, name)   # AttributeError: not exported
        m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"include/mlgpu.h does not declare {name}"
        params = [" ".join(p.split()) for p in m.group(2).split(",")]
        assert [p.split()[-1] for p in params] == want_names, name
        assert m.group(1) == res
        assert [C_TO_CTYPES[p.rsplit(" ", 1)[0]] for p in params] == list(fn.argtypes), name
        assert fn.restype is C_TO_CTYPES[res], name
    assert L.mlgpu_abi_version() == 2   # additive: the version stays
    import madronalib_amd as ml
    for method in ("set_launch_parts", "get_launch_parts", "launch_parts_possible", "launch_stats"):
        assert callable(getattr(ml.Engine, method))
