"""Sparse, stream-ordered updates of per-voice params, coefficients and state (mlgpu_graph_apply_updates / mlgpu_bank_apply_updates):
what needs no GPU - the host planner (madronalib_amd/csrc/param_updates.cpp) under the sanitizers, the exported symbols and their
Python declarations, the record's layout, and the refusal of a graph that has no device."""
import ctypes
import os
import re
import subprocess

import pytest

import madronalib_amd as ml
from madronalib_amd import _lib, constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mlgpu.h")
SYMBOLS = ["mlgpu_graph_reserve_updates", "mlgpu_graph_apply_updates", "mlgpu_graph_update_device_records", "mlgpu_bank_reserve_updates",
           "mlgpu_bank_apply_updates", "mlgpu_graph_get_param", "mlgpu_graph_get_coeff"]


def test_planner_under_sanitizers(tmp_path):
    """tests/cpp/param_updates_test.cpp: hand-written lists against hand-written packed records (single records, CLEAR of a SineGen, a
    TempoLock, a 68-word LinearGlide and of every node, overlap cutting, every refusal with the output untouched, the device-record
    count) and 2 000 random lists against "apply in order", built with g++ -fsanitize=address,undefined from the planner's one
    file - which includes no HIP header."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    # is the sanitizers' runtime installed? asked with a program of one line, so that no error in the code under test can pass as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = str(tmp_path / "param_updates_test")
    planner = os.path.join(CSRC, "param_updates.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "param_updates_test.cpp"), planner, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", planner], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "param_updates.hpp" in used
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_symbols_are_exported_and_declared():
    L = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) >= 2, name
    assert L.mlgpu_graph_update_device_records.restype is ctypes.c_size_t
    assert L.mlgpu_abi_version() == 2   # additive
    assert "updates.hip" in _lib._sources() and "param_updates.cpp" in _lib._sources() and "param_updates.hpp" in _lib._sources()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bMLGPU_UPDATE_([A-Z_]+)\s*=\s*(\d+)", header)}
    assert vals == {k: v for k, v in vars(constants.UpdateTarget).items() if not k.startswith("_")} and len(vals) == 5


def test_update_struct_has_the_c_layout(tmp_path):
    """ml.Update against sizeof / offsetof of mlgpu_update as a C compiler lays it out from include/mlgpu.h."""
    if not os.path.exists("/usr/bin/gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "layout.c"
    fields = [n for n, _ in ml.Update._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mlgpu.h"\nint main(void) { printf("%zu", sizeof(mlgpu_update));\n'
                   + "".join('printf(" %%zu", offsetof(mlgpu_update, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    b = subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True, timeout=120)
    assert b.returncode == 0, b.stderr[-2000:]
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [ctypes.sizeof(ml.Update)] + [getattr(ml.Update, f).offset for f in fields]
    assert ctypes.sizeof(ml.Update) == 20


def test_update_constructors():
    u = ml.Update.param(3, 16, 16, 0.5)
    assert (u.node, u.target, u.index, u.first_voice, u.n_voices, u.bits) == (3, 0, 0, 16, 16, 0x3F000000)
    u = ml.Update.coeff(5, 2, 0, 1, -0.0)
    assert (u.node, u.target, u.index, u.first_voice, u.n_voices, u.bits) == (5, 1, 2, 0, 1, 0x80000000)
    u = ml.Update.state(7, 67, 79, 1, 0xFFFFFFFF)
    assert (u.node, u.target, u.index, u.first_voice, u.n_voices, u.bits) == (7, 2, 67, 79, 1, 0xFFFFFFFF)
    u = ml.Update.input_const(60, 10, 1e-40)   # a denormal stays one
    assert (u.target, u.first_voice, u.n_voices, u.bits) == (3, 60, 10, 71362)
    u = ml.Update.clear(-1, 64, 16)
    assert (u.node, u.target, u.first_voice, u.n_voices) == (-1, 4, 64, 16)


def test_offline_graph_refuses_updates_with_a_message():
    """A graph without an engine is never compiled: apply_updates, reserve_updates and the read-backs say so; nothing is counted."""
    from madronalib_amd.constants import Proc
    g = ml.Graph(ml.OfflineEngine(), 64)
    p = g.add("pitch", "param")
    s = g.add("saw", "proc", Proc.SAW_GEN, ["pitch"])
    g.add_output(s)
    recs = [ml.Update.param(p, 0, 16, 0.01)]
    with pytest.raises(ml.MlgpuError) as ei:
        g.apply_updates(recs)
    assert ei.value.status == ml.Status.ERR_INVALID and "graph_apply_updates: compile first" in str(ei.value)
    with pytest.raises(ml.MlgpuError) as ei:
        g.reserve_updates(100)
    assert ei.value.status == ml.Status.ERR_INVALID and "compile first" in str(ei.value)
    with pytest.raises(ml.MlgpuError) as ei:
        g.get_param(p)
    assert ei.value.status == ml.Status.ERR_INVALID
    with pytest.raises(ml.MlgpuError) as ei:
        g.get_coeff(s, 0)
    assert ei.value.status == ml.Status.ERR_INVALID
    assert g.update_device_records(recs) == 0
    assert g.L.mlgpu_graph_apply_updates(None, None, 0) == ml.Status.ERR_INVALID
    assert g.L.mlgpu_bank_apply_updates(None, None, 0) == ml.Status.ERR_INVALID
