"""The turn-taking rule of the pinned staging sets without a GPU: madronalib_amd/csrc/staging_turns.hpp is plain C++ templated on
an event API, driven here by a fake that counts calls and fails on demand (tests/cpp/staging_turns_test.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "madronalib_amd", "csrc", "staging_turns.hpp")


def test_turns_under_sanitizers(tmp_path):
    """Two sets come out in the order 0, 1, 0, 1, 0 with 3 waits and 5 records; nothing submitted, nothing waited for; a failing
    record drains the stream once and leaves the set free; a failing wait leaves index and pending flag alone and the same set
    comes out next; drained() clears both sets without a wait; the event is created once, destroyed once and created again after a
    reset; a single turn used for a round trip. Built with g++ -fsanitize=address,undefined from the header alone - which includes
    nothing, HIP least of all - and run directly."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    # is the sanitizers' runtime installed? asked with a program of one line, so that no error in the code under test can pass as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = str(tmp_path / "staging_turns_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "staging_turns_test.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    assert "#include" not in open(HEADER).read()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
