"""Voice tails without a GPU: the host half (madronalib_amd/csrc/voice_tails.cpp) is plain C++ whose event calls come in through
an Api of function pointers, driven here by a fake whose events complete when the test says (tests/cpp/voice_tails_test.cpp); the
entry points as the header declares them; the Python restatement of the rule that the GPU tests compare against."""
import os
import re
import subprocess

import numpy as np
import pytest

import tails_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "madronalib_amd", "csrc")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "voice_tails_test.cpp"), os.path.join(CSRC, "voice_tails.cpp"), os.path.join(CSRC, "voice_list.cpp")]


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall"] + flags + SOURCES + ["-o", exe], capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def test_host_half_is_plain_cpp_and_keeps_the_rule(tmp_path):
    """Built by g++ alone, with no HIP header anywhere in what it includes. Hand-written cases - the strict > at the threshold, a hold
    reached exactly, resets by a must-set and by loudness, a list that was never noted, BUSY at depth, clear, RANGE and every refusal of
    a must-set leaving the state intact - and seeded random walks of 34 000 steps (lists of 0 .. 200 voices out of 1 000, 0 .. depth
    results outstanding) against a brute-force model over std::set: equal lists at every step, a superset of the synchronous
    object's, the rule given every result after a wait - and no wait inside next_list or note, by the fake's count."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = _build(tmp_path, "voice_tails_test", [])
    for src in SOURCES[1:]:
        used = subprocess.run(["g++", "-std=c++17", "-M", src], capture_output=True, text=True, timeout=300).stdout
        assert "hip/" not in used and "hip_runtime" not in used and "/opt/rocm" not in used, used
    assert "voice_tails.hpp" in subprocess.run(["g++", "-std=c++17", "-M", SOURCES[1]], capture_output=True, text=True, timeout=300).stdout
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
    walks = re.findall(r"walk depth (\d+): (\d+) steps, (\d+) lists, (\d+) BUSY", r.stdout)
    assert len(walks) == 3 and sum(int(w[1]) for w in walks) >= 20000 and all(int(w[3]) > 0 for w in walks), r.stdout


def test_host_half_under_sanitizers(tmp_path):
    """The same program as a stand-alone executable under -fsanitize=address,undefined, run directly."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    # is the sanitizers' runtime installed? asked with a program of one line, so that no error in the code under test can pass as a skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    pb = subprocess.run(["g++", "-std=c++17"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if pb.returncode != 0:
        pytest.skip("sanitizer runtime not installed: " + pb.stderr[-200:])
    exe = _build(tmp_path, "voice_tails_test_san", flags)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]


def test_entry_points_and_the_python_class_are_there():
    import madronalib_amd as ml
    from madronalib_amd import _lib
    L = _lib.load()
    for name in ("create", "destroy", "set_threshold", "clear", "next_list", "note", "pending", "wait"):
        assert hasattr(L, "mlgpu_tails_" + name)
    for name in ("set_threshold", "next_list", "note", "pending", "wait", "clear"):
        assert hasattr(ml.VoiceTails, name)
    assert L.mlgpu_tails_pending(None) == 0 and L.mlgpu_tails_wait(None) == ml.Status.ERR_INVALID
    h = open(os.path.join(ROOT, "include", "mlgpu.h")).read()
    block = h[h.index("The intended block:"):h.index("int mlgpu_graph_enable_voice_list_events")]
    assert "mlgpu_tails_next_list" in block and "mlgpu_tails_note" in block
    assert b"voice_tails_kernel" in open(_lib.LIB_PATH, "rb").read()


def test_python_restatement_of_the_rule():
    """tests/tails_rule.py, which the GPU tests compare the object against, on the header's own small cases."""
    r = tails_rule.Rule(hold=2)
    assert list(r.next_list([1, 5])) == [1, 5]
    r.note(1, loud=[False, False])
    assert list(r.next_list([], taken_in=0)) == [1, 5]           # nothing taken in: both stay through S_1
    r.note(1, loud=[False, True])
    assert list(r.next_list([])) == [1, 5]                       # launch 1: in S_1. launch 2: voice 1 quiet 1, voice 5 loud
    r.note(1, loud=[False, False])
    assert list(r.next_list([])) == [5]                          # voice 1: quiet 2, the hold
    r.note(3, loud=[False])
    assert list(r.next_list([7])) == [7]
    assert list(r.next_list([])) == [7]                          # the list before was never noted: only its must-set's reset
    assert r.quiet_behind == {1: 2, 5: 4}                        # voice 5: one quiet vector, then three
    assert tails_rule.loud_bits(np.array([0, 9, 10, 11, 0x7fc00000], np.uint32), 10).tolist() == [False, False, False, True, True]
