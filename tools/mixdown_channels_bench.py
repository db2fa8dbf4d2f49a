"""Developer tool: what a two-channel mix of a fused bank costs. SawGen -> Bandpass -> Gain (the config-3 chain) on per-voice constant
frequencies, V voices, T DSPVectors per launch, a pan per voice (constant power), in one process:
  (a) the route the two-channel call replaces: Bank.process into V rows of memory, then Engine.mixdown once per channel,
  (b) the floor: Bank.process_mixdown, ONE channel, with per-voice gains,
  (c) Bank.process_mixdown_channels, two channels.
The three routes alternate every 25 launches; device time per launch between events on the engine's stream (Engine.lap_times_ms:
mlgpu_timer_laps_*), p10 / p50 / p90. Checks first that (c) has the bits of (a) in both channels and of (b) in the first.

  python tools/mixdown_channels_bench.py [voices] [vectors] [launches per route] [--md file to append the table to]"""
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
V, T, LAUNCHES = (int(args[0]) if args else 262144), (int(args[1]) if len(args) > 1 else 1), (int(args[2]) if len(args) > 2 else 300)
C, BLOCK, WARMUP = 2, 25, 25
PROCS = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]

eng = ml.Engine(0)
eng.mixdown_reserve_channels(V, T, C)
rng = np.random.default_rng(0)
freq = (55.0 * 2.0 ** (5.0 * rng.random(V)) / 48000.0).astype(np.float32)
few = np.stack([ml.Bandpass.makeCoeffs(0.01 + 0.4 * j / 256, 0.05 + 0.5 * (j % 7) / 7) for j in range(256)], 1)   # [3][256]
coeffs = np.ascontiguousarray(np.concatenate([few[:, rng.integers(0, 256, V)], np.full((1, V), 0.25, np.float32)], 0))
pan = rng.random(V).astype(np.float32)
gains = np.ascontiguousarray(np.stack([np.cos(0.5 * np.pi * pan), np.sin(0.5 * np.pi * pan)]).astype(np.float32))   # [2][V]


def bank():
    b = eng.bank(PROCS, V)
    b.clear()
    b.set_all_coeffs(coeffs)
    b.set_input_const(freq)
    return b


banks = {k: bank() for k in "abc"}
d_gains = eng.to_device(gains)
d_sig = eng.alloc(4 * V * T * 64)
d_a, d_b, d_c = eng.alloc(4 * C * T * 64), eng.alloc(4 * T * 64), eng.alloc(4 * C * T * 64)


def three_calls():
    banks["a"].process(T, d_sig, Layout.QUAD)
    for c in range(C):
        eng.mixdown(d_sig, Layout.QUAD, V, T, d_a.ptr + 4 * c * T * 64, d_gains.ptr + 4 * c * V)


routes = {"(a) process + 2 x mixdown": three_calls,
          "(b) process_mixdown, one channel": lambda: banks["b"].process_mixdown(T, d_b, None, Layout.QUAD, d_gains),
          "(c) process_mixdown_channels, two channels": lambda: banks["c"].process_mixdown_channels(T, C, d_gains, d_c)}
for work in routes.values():
    work()
out_a, out_b, out_c = d_a.download(np.uint32), d_b.download(np.uint32), d_c.download(np.uint32)
assert (out_a != out_c).sum() == 0, f"(a) and (c) differ in {int((out_a != out_c).sum())} words"
assert (out_b != out_c[:T * 64]).sum() == 0, "(b) and the first channel of (c) differ"
assert (out_c[:T * 64] != out_c[T * 64:]).any() and np.isfinite(out_c.view(np.float32)).all() and np.abs(out_c.view(np.float32)).max() > 1e-6

for _ in range(WARMUP):
    for work in routes.values():
        work()
eng.sync()
times = {k: [] for k in routes}
for _ in range((LAUNCHES + BLOCK - 1) // BLOCK):
    for k, work in routes.items():
        times[k].append(eng.lap_times_ms(work, BLOCK))
pct = {k: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for k, v in times.items()}
lines = [f"`python tools/mixdown_channels_bench.py {V} {T} {LAUNCHES}` on {eng.device_info()['name']}: V = {V} voices, {T} DSPVectors per launch, "
         f"the routes alternating every {BLOCK} launches after {WARMUP} warm-up launches of each. (c) was compared first with (a), both "
         "channels, and with (b), the first channel: the same bits.",
         "",
         "| route | launches | p10 us | p50 us | p90 us |",
         "|---|---|---|---|---|"]
for k in routes:
    lines.append(f"| {k} | {np.concatenate(times[k]).size} | {pct[k][0]:.1f} | {pct[k][1]:.1f} | {pct[k][2]:.1f} |")
a, b, c = (pct[k][1] for k in routes)
lines += ["", f"V = {V}, T = {T}: (a)/(c) = {a / c:.2f}, (c)/(b) = {c / b:.2f} at p50.", ""]
print("\n".join(lines))
if md:
    with open(md, "a") as f:
        f.write("\n".join(lines) + "\n")
for b_ in banks.values():
    b_.close()
eng.close()
