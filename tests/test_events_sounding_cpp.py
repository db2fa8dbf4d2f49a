"""The host event router's sounding set and its routing ahead of the launch (EventRouter::soundingVoices / routeAhead in
madronalib_amd/csrc/events_router.cpp), without a device: tests/cpp/events_sounding_test.cpp built with g++ from that one file, as
tests/test_host_cpp.py builds the router test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sounding_voices_and_route_ahead_on_the_cpu(tmp_path):
    """Hand-written performances, polyphony 2 and 4: the exact sounding set after each routed launch - note on, note off in a later
    launch, a stolen voice, unison, a pedal-sustained key released after the pedal, a launch with no events; route_ahead followed by
    the process-side route gives the records a single route gives; a mismatch is reported and consumes nothing."""
    if not os.path.exists("/usr/bin/g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "events_sounding_test")
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", os.path.join(ROOT, "tests", "cpp", "events_sounding_test.cpp"),
                        os.path.join(ROOT, "madronalib_amd", "csrc", "events_router.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "All tests passed" in r.stdout, (r.stdout + r.stderr)[-3000:]
