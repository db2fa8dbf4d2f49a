"""Developer tool: which of bench.py's workloads ever launch in two parts. Sets each workload up as bench.py does, with the engine's
launch parts at --parts (default 0: by size), runs two steps of its launches and prints Engine.launch_stats() - (launches in two parts,
times the streams met) - for the launches and, apart, for the set-up; then the same for the real-time case (bench.py's rt_case), whose
free-running leg of plain process calls comes before its paced blocks. One JSON line per workload.

  python tools/launch_parts_stats.py [--parts 0|1|2|3]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bench  # noqa: E402
import madronalib_amd as ml  # noqa: E402

PARTS = int(sys.argv[sys.argv.index("--parts") + 1]) if "--parts" in sys.argv else 0

for name in ("cfg3", "cfg4", "cfg5", "synth"):
    eng = ml.Engine(0)
    eng.set_launch_parts(PARTS)
    eng._bench_two_streams = False
    V, T, L = bench.WORKLOADS[name]
    eng._bench_launches = 2 * L + 1
    launch, alg, kname, desc, keep = bench.setup_workload(eng, name, V, T, 0, V)
    eng.sync()
    before = eng.launch_stats()
    for _ in range(2 * L):
        launch()
    eng.sync()
    after = eng.launch_stats()
    print(json.dumps({"workload": name, "parts": PARTS, "launches": 2 * L, "split_launches": after[0] - before[0], "joins": after[1] - before[1],
                      "split_launches_in_setup": before[0]}), flush=True)
    bench._release(keep)
    eng.close()
eng = ml.Engine(0)
eng.set_launch_parts(PARTS)
r = bench.rt_case(eng, blocks=150, lead_in=10, two_calls=False)
s = eng.launch_stats()
print(json.dumps({"workload": "rt", "parts": PARTS, "paced_blocks": 150, "split_launches": s[0], "joins": s[1],
                  "note": "the split launches are rt_case's free-running leg of plain bank.process calls (kernel_us); the paced blocks are process_mixdown",
                  "voice_kernel_us_free_running": r.get("voice_kernel_us_free_running") if isinstance(r, dict) else None}), flush=True)
eng.close()
