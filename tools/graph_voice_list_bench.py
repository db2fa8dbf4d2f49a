"""Developer tool: what a listed launch of a graph costs. The config-5 synth voice (patches.synth16), a graph of V voices of which
K = V / 8 are listed, in one process:
  (a) Graph.process_listed of the K listed voices (with their peaks),
  (b) Graph.process of a separate K-voice graph holding the same voices - the yardstick for "cost proportional to K",
  (c) Graph.process of the full graph - what a caller pays without a list.
Once with a seeded random ascending list and once with the list as one contiguous range of K voices, which separates the cost of
the gather from the rest. The three routes alternate every 25 launches; device time per launch from events on the engine's stream
(Engine.lap_times_ms: mlgpu_timer_laps_*), p10 / p50 / p90. Checks first that (a) and (b) give the same bits.

  python tools/graph_voice_list_bench.py [voices] [vectors] [launches per route] [--md profiles/graph_voice_list.md]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.constants import Layout  # noqa: E402
from madronalib_amd.sharding import cfg5_gate_quad, cfg5_voice_params  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, T, LAUNCHES = (int(args[0]) if args else 262144), (int(args[1]) if len(args) > 1 else 16), (int(args[2]) if len(args) > 2 else 300)
K, BLOCK, WARMUP = V // 8, 25, 25

eng = ml.Engine(0)
rng = np.random.default_rng(0)
desc, outs = patches.synth16()
params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)
gate = cfg5_gate_quad(0, V, T)   # QUAD: [16 T][V][4]


def graph_of(voices, voice_lists):
    g = ml.Graph(eng, voices.size, desc, outs, voice_lists=voice_lists)
    g.clear()
    for k, v in params.items():
        g.set_param(k, np.ascontiguousarray(v[voices]) if np.ndim(v) else float(v))
    for k, c in coeffs.items():
        g.set_coeffs(k, [np.ascontiguousarray(r[voices]) for r in c])
    g.set_state("noise", 0, seeds[voices])
    return g


lists = {"seeded random, ascending": np.sort(rng.choice(V, K, replace=False)).astype(np.uint32),
         "one contiguous range": np.arange(V // 2, V // 2 + K, dtype=np.uint32)}
d_gate = eng.to_device(gate)
d_full, d_listed, d_small, d_peak = eng.alloc(4 * V * T * 64), eng.alloc(4 * K * T * 64), eng.alloc(4 * K * T * 64), eng.alloc(4 * K)
name = eng.device_info()["name"]
lines = [
    "# What a listed launch of a graph costs",
    "",
    f"`python tools/graph_voice_list_bench.py {V} {T} {LAUNCHES}` on {name}: the config-5 synth voice (`patches.synth16`), a graph of "
    f"V = {V} voices, K = V / 8 = {K} of them listed, {T} DSPVectors per launch, QUAD in and out. (a) `Graph.process_listed` with peaks, "
    "(b) `Graph.process` of a separate K-voice graph holding the same voices, (c) `Graph.process` of the full graph. One process, the "
    f"three routes alternating every {BLOCK} launches after {WARMUP} warm-up launches of each; device time per launch between events on "
    "the engine's stream. (a) and (b) were compared first: the same bits.",
    "",
    "| list | route | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|---|",
]
ratios = []
for label, L in lists.items():
    full, small = graph_of(np.arange(V), True), graph_of(L.astype(np.int64), False)   # (both from clear: (a) and (b) start alike)
    full.reserve_voice_list(K)
    d_gate_small = eng.to_device(np.ascontiguousarray(gate[:, L.astype(np.int64), :]))
    full.set_voice_list(L)
    routes = {"(a) process_listed, K of V": lambda: full.process_listed(T, [d_gate], [d_listed], Layout.QUAD, Layout.QUAD, d_peak=d_peak),
              "(b) process, K-voice graph": lambda: small.process(T, [d_gate_small], [d_small]),
              "(c) process, V-voice graph": lambda: full.process(T, [d_gate], [d_full])}
    list(routes.values())[0]()
    list(routes.values())[1]()
    differ = int((d_listed.download(np.uint32) != d_small.download(np.uint32)).sum())
    assert differ == 0, f"{label}: process_listed and the K-voice graph differ in {differ} words"
    for _ in range(WARMUP):
        for work in routes.values():
            work()
    eng.sync()
    times = {k: [] for k in routes}
    for _ in range((LAUNCHES + BLOCK - 1) // BLOCK):
        for k, work in routes.items():
            times[k].append(eng.lap_times_ms(work, BLOCK))
    pct = {k: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for k, v in times.items()}
    for k in routes:
        lines.append(f"| {label} | {k} | {np.concatenate(times[k]).size} | {pct[k][0]:.1f} | {pct[k][1]:.1f} | {pct[k][2]:.1f} |")
    a, b, c = (pct[k][1] for k in routes)
    ratios.append(f"{label}: (a)/(b) = {a / b:.2f}, (a)/(c) = {a / c:.3f} at p50 (K/V = {K / V:.3f}).")
    small.close()
    full.close()
lines += [""] + ratios
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
eng.close()
