"""Developer tool: what clearing the delay ring of some voices costs (MLGPU_UPDATE_CLEAR_RINGS in Graph.apply_updates), beside the one
way there was before: mlgpu_graph_clear_proc, which zeroes the node's rings for every voice.

A one-node IntegerDelay graph whose ring memory is about 1 GiB - a ring of 4 096 words at 65 536 voices, and a ring of 65 536 words
at 4 096 voices - in ring layouts 0, 2 and 4; a clear of 1, 16 and 256 voices. Measured per case, the two calls alternating in one
loop on an idle stream: the time from enqueue to completion (stream events around the one call: the record upload and the two small
kernels; for clear_proc its fill), median of the repeats after warm-up, and the host call's duration (perf_counter around the call).
mlgpu_graph_clear_proc is the same code before and after the new target: its figure is the former way's.

  python tools/ring_clear_bench.py [repeats] [--md profiles/param_updates.md]     (--md replaces that file's section on ring clears)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd.constants import Proc  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
REPEATS, WARMUP = (int(args[0]) if args else 30), 5
HEADING = "## Clearing the delay ring of some voices"
SHAPES = [(4096, 65536), (65536, 4096)]        # (ring length in words, voices): 1 GiB of ring memory each
LAYOUTS = [(0, False), (2, 2), (4, 4)]
FIRST = 1000                                   # (a range of 256 voices from here lies in two 256-voice blocks)

eng = ml.Engine(0)
rows = []
for ring, V in SHAPES:
    for layout, arg in LAYOUTS:
        g = ml.Graph(eng, V, [dict(name="x", type="input"), dict(name="d", type="proc", kind=Proc.INTEGER_DELAY, inputs=["x"], max_delay=float(ring - 64))],
                     ["d"], delay_windows=arg)
        g.clear()
        node = g.ids["d"]
        g.reserve_updates(64)
        L, h = g.L, g.h
        for voices in (1, 16, 256):
            recs = (ml.Update * 1)(ml.Update.clear_rings(node, FIRST, voices))
            calls = {"clear_rings": lambda: L.mlgpu_graph_apply_updates(h, recs, 1), "clear_proc": lambda: L.mlgpu_graph_clear_proc(h, node)}
            dev_us = {k: [] for k in calls}
            host_us = {k: [] for k in calls}
            for k in range(WARMUP + REPEATS):
                for name, call in calls.items():
                    eng.sync()
                    eng.timer_start()
                    t0 = time.perf_counter()
                    st = call()
                    t1 = time.perf_counter()
                    ms = eng.timer_stop_ms()
                    assert st == 0, (name, st)
                    if k >= WARMUP:
                        dev_us[name].append(ms * 1e3)
                        host_us[name].append((t1 - t0) * 1e6)
            med = lambda xs: float(np.median(xs))
            row = (ring, V, layout, voices, g.update_device_records(recs), med(dev_us["clear_rings"]), float(np.min(dev_us["clear_rings"])), float(np.max(dev_us["clear_rings"])),
                   med(host_us["clear_rings"]), med(dev_us["clear_proc"]), med(host_us["clear_proc"]))
            rows.append(row)
            print("ring %6d x %6d voices, layout %d, clear of %3d voices (%d device records, %5d KiB): device %7.1f us (min %.1f, max %.1f), host call %5.1f us | "
                  "clear_proc (%d MiB) device %7.1f us, host call %5.1f us" % (row[:5] + (voices * ring * 4 // 1024,) + row[5:9] + (ring * V * 4 >> 20,) + row[9:]), flush=True)
        g.close()

if md:
    old = open(md).read() if os.path.exists(md) else ""
    if HEADING in old:
        old = old[:old.index(HEADING)]
    with open(md, "w") as f:
        f.write(old.rstrip("\n") + "\n\n" if old.strip() else "")
        f.write(HEADING + f" ({eng.device_info()['name'].strip().strip('()')})\n\n"
                f"`tools/ring_clear_bench.py {REPEATS}`: a graph of one IntegerDelay with 1 GiB of ring memory; one `MLGPU_UPDATE_CLEAR_RINGS` record for voices\n"
                f"[{FIRST}, {FIRST} + n) through `apply_updates`, beside `mlgpu_graph_clear_proc` of the same node - every voice's ring, the only clear of a ring\n"
                "before the target, and the same code since. Device: stream events around the one call on an idle stream (record upload + kernels, or\n"
                f"the fill), median (min - max) of {REPEATS} after {WARMUP}, the two calls alternating. Host: `perf_counter` around the call, median.\n\n"
                "| ring (words) | voices | layout | cleared voices | device records | KiB zeroed | clear_rings device (us) | clear_rings host (us) | clear_proc device (us) | clear_proc host (us) |\n"
                "|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for ring, V, layout, voices, nrec, dev, lo, hi, host, pdev, phost in rows:
            f.write(f"| {ring} | {V} | {layout} | {voices} | {nrec} | {voices * ring * 4 // 1024} | {dev:.1f} ({lo:.1f} - {hi:.1f}) | {host:.1f} | {pdev:.1f} | {phost:.1f} |\n")
        sixteen = [r for r in rows if r[3] == 16]
        f.write(f"\nThe clear of 16 voices takes {min(r[5] for r in sixteen):.1f} - {max(r[5] for r in sixteen):.1f} us against {min(r[9] for r in sixteen):.1f} - "
                f"{max(r[9] for r in sixteen):.1f} us for the whole node. Up to a few MiB the call is bound by the record upload and the launch, not by the bytes it writes.\n")
eng.close()
