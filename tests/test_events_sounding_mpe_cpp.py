"""The host event router's sounding set as graph voice indices in either protocol (EventRouter::soundingGraphVoices in
madronalib_amd/csrc/events_router.cpp), without a device: tests/cpp/events_sounding_mpe_test.cpp built with g++ from that file and
events_router.cpp alone, as tests/test_events_sounding_cpp.py builds its program - here with the address and undefined-behaviour
sanitizers: a stand-alone program with its own main."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sounding_graph_voices_on_the_cpu(tmp_path):
    """Hand-written MPE performances, polyphony 2, 5 and 16 (G = 4, 8 and 32): the exact set after each routed launch - a note on a
    member channel, its note-off in a later launch, a stolen voice, a channel-1 bend alone, an instrument's first event (all its voices,
    neither its main lane nor a padding lane), all-notes-off, a capacity too small, clear(), a protocol switch and back, route_ahead;
    under MIDI the set is soundingVoices'."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "events_sounding_mpe_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "cpp", "events_sounding_mpe_test.cpp"),
                        os.path.join(ROOT, "madronalib_amd", "csrc", "events_router.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
