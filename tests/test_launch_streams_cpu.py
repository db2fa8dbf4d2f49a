"""The two-stream rule of launches that go out in parts without a GPU: mlparts::Streams (madronalib_amd/csrc/launch_parts.hpp) is plain
C++ templated on a stream API, driven here by a fake that logs every call and fails the n-th of a kind on demand
(tests/cpp/launch_streams_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
TEST = os.path.join(ROOT, "tests", "cpp", "launch_streams_test.cpp")


def test_streams_under_sanitizers(tmp_path):
    """The exact call log of a first launch (priority, stream, two events, record, wait, then main 0, side 0, main 1, side 1) for plans
    of 2, 3 and 4 kernels; later launches of the owner with nothing but their kernels; the lazy join, once; a join and a fork before
    a launch that is not admitted; fork() failing at each of its six calls (one part, nothing pending, counted or half made, the next
    launch succeeds); a part failing at each of four places; join() falling back to a host wait, and which error it keeps; what the
    destructor destroys. Built with g++ -fsanitize=address,undefined from the header and launch_parts.cpp - no HIP header is read -
    and run directly."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    # is the sanitizers' runtime installed? asked with a program of one line, so that no error in the code under test can pass as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = str(tmp_path / "launch_streams_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [TEST, os.path.join(CSRC, "launch_parts.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    deps = subprocess.run(["g++", "-std=c++17", "-M", TEST], capture_output=True, text=True, timeout=300)
    assert deps.returncode == 0, deps.stderr[-3000:]
    # every file the program includes, paths inside this checkout taken relative to it (wherever the checkout lies)
    headers = [os.path.relpath(h, ROOT) if os.path.abspath(h).startswith(ROOT + os.sep) else h
               for h in deps.stdout.replace("\\\n", " ").split() if not h.endswith(":")]
    assert any(h.endswith("launch_parts.hpp") for h in headers), headers
    assert not [h for h in headers if "hip/" in h or "rocm" in h], headers
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
