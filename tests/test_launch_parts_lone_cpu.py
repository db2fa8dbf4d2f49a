"""Which kernels of a bank launch in parts count as at most one workgroup per CU - the parts mlgpu_bank_process hands
MLGPU_KFLAG_LONE_WAVEFRONTS, whose wavefronts take no turns at the priority levels - without a GPU: mlparts::atMostAWorkgroupPerCu
(madronalib_amd/csrc/launch_parts.hpp) over the plans of the headline launch, the rt block and the test modes, at the boundary and
beside it (tests/cpp/launch_parts_lone_test.cpp, a stand-alone program under the address and undefined-behaviour sanitizers); and
that the host code uses that rule and the one workgroup size."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")


def test_which_parts_are_at_most_a_workgroup_per_cu(tmp_path):
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "launch_parts_lone_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "launch_parts_lone_test.cpp"), os.path.join(CSRC, "launch_parts.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_the_host_sets_the_flag_by_that_rule():
    """mlgpu_bank_process sets the bit on a part's arguments by the tested rule, with the workgroup size the plan is made with, and
    chains.hip holds that size to the kernels' own."""
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    assert re.search(r"if \(mlparts::atMostAWorkgroupPerCu\(w\.V, \(size_t\)e->cuCount, mlparts::kLanesPerWorkgroup\)\) w\.flags \|= MLGPU_KFLAG_LONE_WAVEFRONTS;", capi)
    assert "mlparts::splitPlan(V, T, e->launchParts, (size_t)e->cuCount, mlparts::kLanesPerWorkgroup)" in capi
    assert capi.count("MLGPU_KFLAG_LONE_WAVEFRONTS") == 1          # (no other launch sets it)
    assert "mlparts::kLanesPerWorkgroup == (size_t)kChainBlock" in open(os.path.join(CSRC, "chains.hip")).read()
