"""Developer tool: what per-instrument sums of the listed voices cost. SawGen -> Bandpass -> Gain on per-voice constant frequencies, a bank
of V voices as V / 16 instruments of 16, of which K = V / 8 voices are listed, in one process:
  (a) Bank.process_listed_groups of the list (with the peaks): J rows, one per listed instrument,
  (b) Bank.process_listed of the same list: K rows, which a host would still have to add up by instrument,
  (c) Bank.process_groups(out_group=16) of the whole bank: V / 16 rows - the only other way to per-instrument channels in one launch.
Two lists: "spread", two sounding voices in every instrument (J = V / 16), and "clustered", every voice of every eighth instrument
(J = V / 128). The three routes alternate every 25 launches; device time per launch from events on the engine's stream
(Engine.lap_times_ms), p10 / p50 / p90. Checks first that (a)'s rows are, bit for bit, the in-order float32 sums made on the host
from (b)'s rows.

  python tools/voice_list_groups_bench.py [voices] [vectors] [launches per route] [--md FILE]"""
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
G, BLOCK, WARMUP = 16, 25, 25
K = V // 8
assert V % (8 * G) == 0
PROCS = [Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN]

eng = ml.Engine(0)
rng = np.random.default_rng(0)
freq = (55.0 * 2.0 ** (5.0 * rng.random(V)) / 48000.0).astype(np.float32)
few = np.stack([ml.Bandpass.makeCoeffs(0.01 + 0.4 * j / 256, 0.05 + 0.5 * (j % 7) / 7) for j in range(256)], 1)   # [3][256]
coeffs = np.ascontiguousarray(np.concatenate([few[:, rng.integers(0, 256, V)], np.full((1, V), 0.25, np.float32)], 0))

inst = np.arange(V // G, dtype=np.int64)
lists = {"spread: 2 voices of every instrument": np.sort(np.concatenate([inst * G + 3, inst * G + 11])).astype(np.uint32),
         "clustered: all 16 voices of every 8th instrument": (inst[::8, None] * G + np.arange(G)[None, :]).reshape(-1).astype(np.uint32)}
bank = eng.bank(PROCS, V)
bank.set_all_coeffs(coeffs)
bank.set_input_const(freq)
bank.reserve_voice_list_groups(K, G)
d_groups, d_listed, d_full = eng.alloc(4 * (V // G) * T * 64), eng.alloc(4 * K * T * 64), eng.alloc(4 * (V // G) * T * 64)
d_rows, d_peak = eng.alloc(4 * K * T * 64), eng.alloc(4 * K)
name = eng.device_info()["name"]
lines = [
    "# What per-instrument sums of the listed voices cost",
    "",
    f"`python tools/voice_list_groups_bench.py {V} {T} {LAUNCHES}` on {name}: SawGen -> Bandpass -> Gain on per-voice constant "
    f"frequencies, a bank of V = {V} voices as {V // G} instruments of {G}, K = V / 8 = {K} voices listed, {T} DSPVectors per launch, QUAD "
    "output. (a) `Bank.process_listed_groups` with peaks (J rows), (b) `Bank.process_listed` of the same list (K rows), (c) "
    f"`Bank.process_groups(out_group={G})` of the whole bank (V / {G} rows). One process, the three routes alternating every {BLOCK} launches "
    f"after {WARMUP} warm-up launches of each; device time per launch between events on the engine's stream. (a)'s rows were compared "
    "first with the in-order float32 sums made on the host from (b)'s rows: the same bits.",
    "",
    "| list | J | lanes N | route | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|---|---|---|",
]
ratios = []
for label, L in lists.items():
    assert L.size == K
    bank.set_voice_list(L)
    M = bank.listed_groups
    J = M.size
    row = np.searchsorted(M, L // G)
    rank = np.arange(K) - np.searchsorted(row, row, side="left")
    lanes = 0   # the plan's lane count, as the header states the rule
    for n in np.diff(np.concatenate([np.nonzero(rank == 0)[0], [K]])):
        if n > 64 - lanes % 64:
            lanes += 64 - lanes % 64
        lanes += int(n)
    # (a) against the host's sums of (b), both from clear()
    bank.clear()
    bank.process_listed_groups(T, d_groups, Layout.QUAD, d_peak=d_peak)
    eng.layout_convert(d_groups, Layout.QUAD, d_rows, Layout.VOICE_MAJOR, J, T)
    got = d_rows.download(np.float32, J * 64 * T).reshape(J, 64 * T)
    bank.clear()
    bank.process_listed(T, d_listed, Layout.QUAD)
    eng.layout_convert(d_listed, Layout.QUAD, d_rows, Layout.VOICE_MAJOR, K, T)
    y = d_rows.download(np.float32, K * 64 * T).reshape(K, 64 * T)
    want = np.zeros((J, 64 * T), np.float32)
    for r in range(int(rank.max()) + 1):
        sel = np.nonzero(rank == r)[0]
        want[row[sel]] = want[row[sel]] + y[sel]      # float32 adds, one per listed voice in voice order
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert differ == 0 and np.abs(want).max() > 1e-6, f"{label}: process_listed_groups and the host's sums of process_listed differ in {differ} words"
    del got, y, want
    routes = {"(a) process_listed_groups, J rows": lambda: bank.process_listed_groups(T, d_groups, Layout.QUAD, d_peak=d_peak),
              "(b) process_listed, K rows": lambda: bank.process_listed(T, d_listed, Layout.QUAD),
              f"(c) process_groups({G}), V / {G} rows": lambda: bank.process_groups(T, d_full, G, Layout.QUAD)}
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
        lines.append(f"| {label} | {J} | {lanes} | {k} | {np.concatenate(times[k]).size} | {pct[k][0]:.1f} | {pct[k][1]:.1f} | {pct[k][2]:.1f} |")
    a, b, c = (pct[k][1] for k in routes)
    ratios.append(f"{label}: (a)/(b) = {a / b:.2f}, (a)/(c) = {a / c:.3f} at p50 (K/V = {K / V:.3f}); (a) < (c): {'yes' if a < c else 'NO'}.")
lines += [""] + ratios
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
bank.close()
eng.close()
