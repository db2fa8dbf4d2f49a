"""Developer tool: what changing one param of some instruments costs between back-to-back launches of the synth16 graph.

Per block: one launch of T DSPVectors, then - while its voice kernel is in flight - the `pitch` param of 1, 256 or 16 384 instruments
of 16 voices is changed, either with Graph.apply_updates (one record per instrument, after reserve_updates) or with the whole-row
mlgpu_graph_set_param, the route there was before. Measured: the host call's duration (perf_counter around the one call, p50 / p99
over the blocks; the engine is drained after the measurement so that every block meets the same queue), and the device time of the
update alone on an idle stream (events around the call: the record upload and apply_updates_kernel; the row upload for set_param).

  python tools/param_updates_bench.py [voices] [vectors] [blocks] [--md profiles/param_updates.md]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd.patches import synth16  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, T, BLOCKS = (int(args[0]) if args else 262144), (int(args[1]) if len(args) > 1 else 16), (int(args[2]) if len(args) > 2 else 200)
G, WARMUP = 16, 10
n = V * T * 64

eng = ml.Engine(0)
rng = np.random.default_rng(0)
desc, outs = synth16()
g = ml.Graph(eng, V, desc, outs)
g.clear()
pitch = rng.uniform(-1.0, 3.0, V).astype(np.float32)
g.set_param("pitch", pitch)
g.set_param("baseFreq", 110.0 / 48000.0)
g.set_param("width", 0.5)
g.set_param("lfoFreq", 3.0 / 48000.0)
g.set_param("noiseLevel", 0.1)
g.set_state("noise", 0, np.arange(V, dtype=np.uint32) + 1)
g.set_coeffs("lp", [float(c) for c in ml.Lopass.makeCoeffs(0.1, 0.7)])
g.set_coeffs("hp", [float(c) for c in ml.Hipass.makeCoeffs(0.001, 0.9)])
g.set_coeffs("smooth", [float(c) for c in ml.OnePole.makeCoeffs(0.3)])
g.set_coeff("dc", 0, float(ml.DCBlocker.makeCoeffs(0.0005)))
g.set_coeffs("env", [float(c) for c in ml.ADSR.calcCoeffs(0.01, 0.05, 0.6, 0.1, 48000.0)])
d_gate = eng.to_device(np.ones(n, np.float32))
d_out = eng.alloc(4 * n)
g.reserve_updates(V // G)
pitch_id = g.ids["pitch"]
L, h = g.L, g.h


def pct(xs, p):
    return float(np.percentile(np.asarray(xs), p))


rows = []
for instruments in (1, 256, 16384):
    instruments = min(instruments, V // G)
    which = np.sort(rng.choice(V // G, instruments, replace=False))
    lists = []          # two alternating lists, so that a block really changes the values
    wholes = []
    for value in (0.5, 1.5):
        recs = (ml.Update * instruments)(*[ml.Update.param(pitch_id, int(i) * G, G, value) for i in which])
        row = pitch.copy()
        row.reshape(V // G, G)[which] = value
        lists.append(recs)
        wholes.append(row)

    def new_call(k):
        return L.mlgpu_graph_apply_updates(h, lists[k & 1], instruments)

    def old_call(k):
        return L.mlgpu_graph_set_param(h, pitch_id, wholes[k & 1].ctypes.data_as(ctypes.c_void_p))

    res = {}
    for name, call in (("apply_updates", new_call), ("set_param", old_call)):
        host_us = []
        for k in range(WARMUP + BLOCKS):
            g.process(T, [d_gate], [d_out])
            t0 = time.perf_counter()
            st = call(k)
            t1 = time.perf_counter()
            assert st == 0, st
            eng.sync()
            if k >= WARMUP:
                host_us.append((t1 - t0) * 1e6)
        dev_ms = []
        for k in range(30):
            eng.sync()
            eng.timer_start()
            call(k)
            dev_ms.append(eng.timer_stop_ms())
        res[name] = (pct(host_us, 50), pct(host_us, 99), pct(dev_ms[5:], 50) * 1e3)
    # the voice kernel alone, for scale
    eng.sync()
    eng.timer_start()
    g.process(T, [d_gate], [d_out])
    launch_us = eng.timer_stop_ms() * 1e3
    want = wholes[(29) & 1]
    assert (g.get_param("pitch").view(np.uint32) == want.view(np.uint32)).all()
    rows.append((instruments, res, launch_us))
    print(f"{instruments:6d} instruments x {G} voices: apply_updates host p50 {res['apply_updates'][0]:.1f} us p99 {res['apply_updates'][1]:.1f} us, device "
          f"{res['apply_updates'][2]:.1f} us | set_param (whole row, {4 * V // 1024} KiB) host p50 {res['set_param'][0]:.1f} us p99 {res['set_param'][1]:.1f} us, device "
          f"{res['set_param'][2]:.1f} us | voice kernel of {T} vectors {launch_us:.0f} us", flush=True)

if md:
    with open(md, "w") as f:
        f.write(f"# Changing one param of some instruments between launches ({eng.device_info()['name']})\n\n"
                f"`tools/param_updates_bench.py {V} {T} {BLOCKS}`: synth16 graph, {V} voices, launches of {T} DSPVectors back to back; after each launch the\n"
                f"`pitch` param of some instruments of {G} voices is changed while the voice kernel is in flight. Host call: `perf_counter` around the one\n"
                f"call, {BLOCKS} blocks. Device: events around the call on an idle stream (upload + kernel), median of 25.\n\n"
                "| instruments | apply_updates host p50 / p99 (us) | apply_updates device (us) | set_param whole row host p50 / p99 (us) | set_param device (us) | voice kernel (us) |\n"
                "|---:|---:|---:|---:|---:|---:|\n")
        for instruments, res, launch_us in rows:
            a, s = res["apply_updates"], res["set_param"]
            f.write(f"| {instruments} | {a[0]:.1f} / {a[1]:.1f} | {a[2]:.1f} | {s[0]:.1f} / {s[1]:.1f} | {s[2]:.1f} | {launch_us:.0f} |\n")
        f.write("\nThe whole-row setter ends in a stream synchronize: its host call lasts as long as the voice kernel in flight. apply_updates returns\n"
                "once the records are packed and enqueued, whatever runs on the device.\n")
g.close()
eng.close()
