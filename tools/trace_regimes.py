#!/usr/bin/env python3
"""Reading of a rocprofv3 --kernel-trace CSV of chain kernels that run on two streams (a launch in parts, or the two engines of
tools/launch_parts_probe.py): per queue and grid size the kernels' durations; for each kernel the offset of its start to the nearest
start on the other queue, as a histogram in 20 us bins; and the durations apart for kernels that started IN STEP with one on the other
queue (offset under 25 us) and STAGGERED (anything else).

  python tools/trace_regimes.py kernel_trace.csv [kernels to skip at the start]"""
import bisect
import csv
import statistics as st
import sys


def stats(d):
    return "n %d, us: mean %.1f min %.1f median %.1f max %.1f" % (len(d), st.mean(d), min(d), st.median(d), max(d))


rows = [r for r in csv.DictReader(open(sys.argv[1])) if "chain_kernel" in r["Kernel_Name"]]
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
rows = rows[int(sys.argv[2]) if len(sys.argv) > 2 else 0:]
for r in rows:
    r["s"], r["e"] = int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3
    r["d"] = r["e"] - r["s"]
print("kernels", len(rows), "span ms %.2f" % ((rows[-1]["e"] - rows[0]["s"]) / 1e3))
groups = {}
for r in rows:
    groups.setdefault((r["Queue_Id"], r.get("Stream_Id", ""), r["Grid_Size_X"]), []).append(r["d"])
for key, d in groups.items():
    print("queue %s stream %s grid %s:" % key, stats(d))
queues = sorted({r["Queue_Id"] for r in rows})
if len(queues) >= 2:
    starts = {q: [r["s"] for r in rows if r["Queue_Id"] == q] for q in queues}
    regimes, offsets = {"in step": {}, "staggered": {}}, []
    for r in rows:
        near = []
        for q in queues:
            if q == r["Queue_Id"]:
                continue
            i = bisect.bisect_left(starts[q], r["s"])
            near += [abs(starts[q][j] - r["s"]) for j in (i - 1, i) if 0 <= j < len(starts[q])]
        if not near:
            continue
        offsets.append(min(near))
        regimes["in step" if min(near) < 25 else "staggered"].setdefault(r["Grid_Size_X"], []).append(r["d"])
    print("start offset to the other queue, us: min %.1f median %.1f max %.1f" % (min(offsets), st.median(offsets), max(offsets)))
    hist = {}
    for o in offsets:
        hist[int(o // 20) * 20] = hist.get(int(o // 20) * 20, 0) + 1
    print("offsets in 20 us bins:", sorted(hist.items()))
    for name, by_grid in regimes.items():
        for grid, d in by_grid.items():
            print(f"{name}, grid {grid}:", stats(d))
