"""The mixdown tree's shape without a GPU: madronalib_amd/csrc/mixdown_tree.hpp is plain C++, driven by
tests/cpp/mixdown_tree_test.cpp under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")


def test_tree_shape_and_pass_lists_on_the_cpu_under_sanitizers(tmp_path):
    """Built by g++ from the header alone with no HIP include path, as a stand-alone program with -fsanitize=address,undefined. The
    region's size, the pass lists against the launch loops they replaced, a shard's level and rows
    (tests/cpp/mixdown_tree_test.cpp)."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "mixdown_tree_test")
    src = os.path.join(ROOT, "tests", "cpp", "mixdown_tree_test.cpp")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", src, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    used = subprocess.run(["g++", "-std=c++17", "-M", src], capture_output=True, text=True, timeout=300).stdout
    assert "hip/" not in used and "hip_runtime" not in used and "mixdown_tree.hpp" in used
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_the_library_states_the_tree_arithmetic_once():
    """capi.hip and graph.hip size, check and walk the scratch through mixdown_tree.hpp: neither spells the region's sum out."""
    for name in ("capi.hip", "graph.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert "+ 63) / 64) *" not in text and "mixRegion" not in text, name
        assert "mlmix::" in text, name
