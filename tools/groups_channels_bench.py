"""Developer tool: what a stereo mix per instrument of a fused bank costs. SawGen -> Bandpass -> Gain (the config-3 chain) on per-voice
constant frequencies, V voices as V / G instruments of G, T DSPVectors per launch, a pan per voice (constant power), in one process:
  (a) the route the two-channel call replaces: Bank.process into V rows of memory, then per channel a multiply by the gains (a bank of
      Gain processors, one float multiply per sample) into V more rows and Engine.mixdown_groups over those,
  (b) the floor: Bank.process_groups, ONE channel, with per-voice gains,
  (c) Bank.process_groups_channels, two channels.
With --listed F the bank runs a random ascending list of about F * V voices and (b), (c) are Bank.process_listed_groups and
Bank.process_listed_groups_channels; there is no (a).
The routes alternate every 25 launches; device time per launch between events on the engine's stream (Engine.lap_times_ms:
mlgpu_timer_laps_*), p10 / p50 / p90. Checks first that (c) has the bits of (a) in both channels and of (b) in the first.

  python tools/groups_channels_bench.py [voices] [group] [vectors] [launches per route] [--listed F] [--md file to append the table to]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd.constants import Layout, Proc  # noqa: E402


def option(name):
    if name not in sys.argv:
        return None
    i = sys.argv.index(name)
    value = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return value


md, listed = option("--md"), option("--listed")
args = sys.argv[1:]
V, G, T, LAUNCHES = (int(args[i]) if len(args) > i else d for i, d in enumerate((262144, 16, 1, 300)))
C, BLOCK, WARMUP = 2, 25, 25
PROCS = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]
R = V // G

eng = ml.Engine(0)
rng = np.random.default_rng(0)
freq = (55.0 * 2.0 ** (5.0 * rng.random(V)) / 48000.0).astype(np.float32)
few = np.stack([ml.Bandpass.makeCoeffs(0.01 + 0.4 * j / 256, 0.05 + 0.5 * (j % 7) / 7) for j in range(256)], 1)   # [3][256]
coeffs = np.ascontiguousarray(np.concatenate([few[:, rng.integers(0, 256, V)], np.full((1, V), 0.25, np.float32)], 0))
pan = rng.random(V).astype(np.float32)
gains = np.ascontiguousarray(np.stack([np.cos(0.5 * np.pi * pan), np.sin(0.5 * np.pi * pan)]).astype(np.float32))   # [2][V]
d_gains = eng.to_device(gains)


def bank():
    b = eng.bank(PROCS, V)
    b.clear()
    b.set_all_coeffs(coeffs)
    b.set_input_const(freq)
    return b


banks = {k: bank() for k in ("b", "c") + (() if listed else ("a",))}
if listed:
    L = np.nonzero(rng.random(V) < float(listed))[0].astype(np.uint32)
    for b in banks.values():
        b.reserve_voice_list_groups(L.size, G)
        b.set_voice_list(L)
    R = banks["c"].listed_groups.size
    what = f"a list of {L.size} voices in {R} instruments"
    d_b, d_c = eng.alloc(4 * R * T * 64), eng.alloc(4 * C * R * T * 64)
    routes = {"(b) process_listed_groups, one channel": lambda: banks["b"].process_listed_groups(T, d_b, Layout.QUAD, d_gains=d_gains),
              "(c) process_listed_groups_channels, two channels": lambda: banks["c"].process_listed_groups_channels(T, d_c, Layout.QUAD, n_channels=C, d_gains=d_gains)}
else:
    what = "all voices"
    pans = []
    for c in range(C):
        p = eng.bank([Proc.GAIN], V)
        p.clear()
        p.set_all_coeffs(np.ascontiguousarray(gains[c:c + 1]))
        pans.append(p)
    d_sig, d_scaled = eng.alloc(4 * V * T * 64), eng.alloc(4 * V * T * 64)
    d_a, d_b, d_c = eng.alloc(4 * C * R * T * 64), eng.alloc(4 * R * T * 64), eng.alloc(4 * C * R * T * 64)

    class At:   # (channel c's part of d_a: Engine.mixdown_groups reads .ptr)
        def __init__(self, ptr):
            self.ptr = ptr

    def replaced():
        banks["a"].process(T, d_sig, Layout.QUAD)
        for c in range(C):
            pans[c].process(T, d_scaled, Layout.QUAD, d_sig, Layout.QUAD)
            eng.mixdown_groups(d_scaled, Layout.QUAD, R, G, T, At(d_a.ptr + 4 * c * R * T * 64), Layout.QUAD)

    routes = {"(a) process + 2 x (gain, mixdown_groups)": replaced,
              "(b) process_groups, one channel": lambda: banks["b"].process_groups(T, d_b, G, Layout.QUAD, d_gains=d_gains),
              "(c) process_groups_channels, two channels": lambda: banks["c"].process_groups_channels(T, d_c, G, Layout.QUAD, n_channels=C, d_gains=d_gains)}

for work in routes.values():
    work()
out_b, out_c = d_b.download(np.uint32), d_c.download(np.uint32)
if not listed:
    out_a = d_a.download(np.uint32)
    assert (out_a != out_c).sum() == 0, f"(a) and (c) differ in {int((out_a != out_c).sum())} words"
assert (out_b != out_c[:R * T * 64]).sum() == 0, "(b) and the first channel of (c) differ"
assert (out_c[:R * T * 64] != out_c[R * T * 64:]).any() and np.isfinite(out_c.view(np.float32)).all() and np.abs(out_c.view(np.float32)).max() > 1e-6

for _ in range(WARMUP):
    for work in routes.values():
        work()
eng.sync()
times = {k: [] for k in routes}
for _ in range((LAUNCHES + BLOCK - 1) // BLOCK):
    for k, work in routes.items():
        times[k].append(eng.lap_times_ms(work, BLOCK))
pct = {k: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for k, v in times.items()}
lines = [f"`python tools/groups_channels_bench.py {V} {G} {T} {LAUNCHES}{' --listed ' + listed if listed else ''}` on {eng.device_info()['name']}: V = {V} voices in "
         f"instruments of {G}, {what}, {T} DSPVectors per launch, the routes alternating every {BLOCK} launches after {WARMUP} warm-up launches of "
         "each. (c) was compared first with " + ("" if listed else "(a), both channels, and with ") + "(b), the first channel: the same bits.",
         "",
         "| route | launches | p10 us | p50 us | p90 us |",
         "|---|---|---|---|---|"]
for k in routes:
    lines.append(f"| {k} | {np.concatenate(times[k]).size} | {pct[k][0]:.1f} | {pct[k][1]:.1f} | {pct[k][2]:.1f} |")
p50 = [pct[k][1] for k in routes]
lines += ["", f"V = {V}, G = {G}, T = {T}: " + ("" if listed else f"(a)/(c) = {p50[0] / p50[-1]:.2f}, ") + f"(c)/(b) = {p50[-1] / p50[-2]:.2f} at p50.", ""]
print("\n".join(lines))
if md:
    with open(md, "a") as f:
        f.write("\n".join(lines) + "\n")
for b_ in banks.values():
    b_.close()
eng.close()
