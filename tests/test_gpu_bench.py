"""bench.py end to end on the device: a plain run prints the headline line and launches nothing beside its steps; everything
else it can measure (laps, the same-pattern kernel, counter passes, CPU baseline, other configs, CRC parity) is behind --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "voice-samples/sec (SawGen->SVF chain)"
    assert line["unit"] == "voice-samples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    for key in ("other_configs", "cpu_baseline", "parity_512", "sustained"):
        assert key not in line, key
    roof = line["roofline"]
    for key in ("kernel_ms_p50", "same_pattern_gain_kernel", "frac_of_ceiling", "crc_all_match", "cfg4_frac", "rt_misses"):
        assert key not in roof, key
    assert roof["traffic_source"] is None or "pmc_workloads.json" in roof["traffic_source"]   # no counter passes of its own
