"""MLGPU_UPDATE_CLEAR_RINGS (the per-voice clear of delay rings in mlgpu_graph_apply_updates) where no GPU is needed: the host
planner's ring records under the sanitizers, the new target's value through the layers, and the C++ wrapper's pass-through."""
import os
import re
import subprocess

import pytest

import madronalib_amd as ml
from madronalib_amd import constants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "mlgpu.h")


def test_ring_planner_under_sanitizers(tmp_path):
    """tests/cpp/ring_clear_plan_test.cpp: hand-written voice ranges against ring records worked out by hand for the three granules
    (one voice, ranges over the 256-voice block borders, a second node, a two-ring node, node = -1, the spare lanes of layout 2,
    ring-less nodes and banks, the refusals), and 2 400 random graphs whose covered words must equal a brute-force walk; built
    with g++ -fsanitize=address,undefined from the planner's one file and run directly."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = str(tmp_path / "ring_clear_plan_test")
    planner = os.path.join(CSRC, "param_updates.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "ring_clear_plan_test.cpp"), planner, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", planner], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "param_updates.hpp" in used
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_target_value_through_the_layers(tmp_path):
    """The header declares the new target as the enumerator after CLEAR (the five table targets keep their literal values, which
    tests/test_param_updates_cpu.py pins as the whole of UpdateTarget's own attributes): 5, as a C compiler reads it, and 5 in Python."""
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bMLGPU_UPDATE_CLEAR\s*=\s*4\b", header)
    assert re.search(r"\bMLGPU_UPDATE_CLEAR_RINGS\s*=\s*MLGPU_UPDATE_CLEAR\s*\+\s*1\b", header)
    if os.path.exists("/usr/bin/gcc"):
        src = tmp_path / "target.c"
        src.write_text('#include <stdio.h>\n#include "mlgpu.h"\nint main(void) { printf("%d %d", (int)MLGPU_UPDATE_CLEAR, (int)MLGPU_UPDATE_CLEAR_RINGS); return 0; }\n')
        exe = str(tmp_path / "target")
        b = subprocess.run(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True, timeout=120)
        assert b.returncode == 0, b.stderr[-2000:]
        assert subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split() == ["4", "5"]
    assert constants.UpdateTarget.CLEAR_RINGS == 5 and constants.UpdateTarget.CLEAR == 4
    assert ml.UpdateTarget is constants.UpdateTarget
    u = ml.Update.clear_rings(7, 64, 16)
    assert (u.node, u.target, u.index, u.first_voice, u.n_voices, u.bits) == (7, 5, 0, 64, 16, 0)
    u = ml.Update.clear_rings(-1, 0, 1)
    assert (u.node, u.target) == (-1, 5)


def test_cpp_wrapper_passes_every_target_on():
    """ml::gpu::VoiceBank::applyUpdates hands the list to mlgpu_bank_apply_updates as it is: it mirrors COEFF and INPUT_CONST into
    its host copies and neither drops nor rejects any other target."""
    src = open(os.path.join(ROOT, "include", "mlgpu", "mldsp_gpu.hpp")).read()
    body = src[src.index("void applyUpdates(const mlgpu_update* recs, size_t n)"):]
    body = body[:body.index("void applyUpdates(const std::vector<mlgpu_update>& recs)")]
    assert "mlgpu_bank_apply_updates(b_, recs, n)" in body
    assert "throw" not in body and "MLGPU_UPDATE_CLEAR" not in body and "return" not in body
