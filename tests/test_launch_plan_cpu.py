"""The plan of a launch in up to four kernels on two streams, without a GPU: mlparts::splitPlan (madronalib_amd/csrc/launch_parts.cpp,
plain C++) driven by tests/cpp/launch_plan_test.cpp under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")


def test_plan_on_the_cpu_under_sanitizers(tmp_path):
    """Built by g++ from launch_parts.cpp alone, as a stand-alone program with -fsanitize=address,undefined. For a sweep of voice
    counts (0, one workgroup, one unit and one voice more, ragged last parts, the headline's, a few hundred odd sizes) and every mode:
    the cuts ascend from 0 to V in whole units of 2 048, no part is empty, the streams divide the voices where the two-part launch
    does; the 2 + 2 plan at 8 448 and the halves at 4 096; the automatic mode on 256 and on 304 CUs; the gate on short launches at
    its threshold and one DSPVector either side."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "launch_plan_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "launch_plan_test.cpp"), os.path.join(CSRC, "launch_parts.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]

