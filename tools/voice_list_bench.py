"""Developer tool: what a listed launch costs. SawGen -> Bandpass -> Gain on per-voice constant frequencies, a bank of V voices of which
K = V / 8 are listed, in one process:
  (a) Bank.process_listed of the K listed voices (with their peaks),
  (b) Bank.process of a separate K-voice bank holding the same voices - the yardstick for "cost proportional to K",
  (c) Bank.process of the full bank - what a caller pays without a list.
Once with a seeded random ascending list and once with the list as one contiguous range of K voices, which separates the cost of
the gather from the rest. The three routes alternate every 25 launches; device time per launch from events on the engine's stream
(Engine.lap_times_ms: mlgpu_timer_laps_*), p10 / p50 / p90. Checks first that (a) and (b) give the same bits.

  python tools/voice_list_bench.py [voices] [vectors] [launches per route] [--md profiles/voice_list.md]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd.constants import Layout, Proc  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, T, LAUNCHES = (int(args[0]) if args else 262144), (int(args[1]) if len(args) > 1 else 30), (int(args[2]) if len(args) > 2 else 300)
K, BLOCK, WARMUP = V // 8, 25, 25
PROCS = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]

eng = ml.Engine(0)
rng = np.random.default_rng(0)
freq = (55.0 * 2.0 ** (5.0 * rng.random(V)) / 48000.0).astype(np.float32)
few = np.stack([ml.Bandpass.makeCoeffs(0.01 + 0.4 * j / 256, 0.05 + 0.5 * (j % 7) / 7) for j in range(256)], 1)   # [3][256]
coeffs = np.ascontiguousarray(np.concatenate([few[:, rng.integers(0, 256, V)], np.full((1, V), 0.25, np.float32)], 0))


def bank_of(voices):
    b = eng.bank(PROCS, voices.size)
    b.clear()
    b.set_all_coeffs(np.ascontiguousarray(coeffs[:, voices]))
    b.set_input_const(np.ascontiguousarray(freq[voices]))
    return b


lists = {"seeded random, ascending": np.sort(rng.choice(V, K, replace=False)).astype(np.uint32),
         "one contiguous range": np.arange(V // 2, V // 2 + K, dtype=np.uint32)}
full = bank_of(np.arange(V))
full.reserve_voice_list(K)
d_full, d_listed, d_small, d_peak = eng.alloc(4 * V * T * 64), eng.alloc(4 * K * T * 64), eng.alloc(4 * K * T * 64), eng.alloc(4 * K)
name = eng.device_info()["name"]
lines = [
    "# What a listed launch costs",
    "",
    f"`python tools/voice_list_bench.py {V} {T} {LAUNCHES}` on {name}: SawGen -> Bandpass -> Gain on per-voice constant frequencies, a "
    f"bank of V = {V} voices, K = V / 8 = {K} of them listed, {T} DSPVectors per launch, QUAD output. (a) `Bank.process_listed` with "
    "peaks, (b) `Bank.process` of a separate K-voice bank holding the same voices, (c) `Bank.process` of the full bank. One process, "
    f"the three routes alternating every {BLOCK} launches after {WARMUP} warm-up launches of each; device time per launch between "
    "events on the engine's stream. (a) and (b) were compared first: the same bits.",
    "",
    "| list | route | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|---|",
]
ratios = []
for label, L in lists.items():
    small = bank_of(L.astype(np.int64))
    full.clear()      # (the K-voice bank starts from clear(): so do the listed voices)
    full.set_voice_list(L)
    routes = {"(a) process_listed, K of V": lambda: full.process_listed(T, d_listed, Layout.QUAD, d_peak=d_peak),
              "(b) process, K-voice bank": lambda: small.process(T, d_small, Layout.QUAD),
              "(c) process, V-voice bank": lambda: full.process(T, d_full, Layout.QUAD)}
    list(routes.values())[0]()
    list(routes.values())[1]()
    differ = int((d_listed.download(np.uint32) != d_small.download(np.uint32)).sum())
    assert differ == 0, f"{label}: process_listed and the K-voice bank differ in {differ} words"
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
lines += [""] + ratios
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
full.close()
eng.close()
