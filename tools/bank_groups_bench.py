"""Developer tool: a bank of 16-resonator filter banks (Bandpass, per-voice coefficients, one excitation row and one mixed channel per
16 voices) as ONE launch - Bank.process_groups, in_group = out_group = 16 - against the two steps it replaces: Bank.process on an
input already expanded to one row per voice, then Engine.mixdown_groups. Both in one process on the same bank size, alternating every
25 launches; device time per launch from events on the engine's stream (Engine.lap_times_ms), p10 / p50 / p90, and the signal bytes
each route moves through memory (computed from the shapes). Checks first that both routes give the same bits.

  python tools/bank_groups_bench.py [voices] [vectors] [launches per route] [--md profiles/bank_groups.md]"""
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
V, T, LAUNCHES = (int(args[0]) if args else 262144), (int(args[1]) if len(args) > 1 else 16), (int(args[2]) if len(args) > 2 else 1000)
G, BLOCK, WARMUP = 16, 25, 50
C, n = V // G, V * T * 64

eng = ml.Engine(0)
rng = np.random.default_rng(0)
few = np.stack([ml.Bandpass.makeCoeffs(0.01 + 0.4 * j / 256, 0.05 + 0.5 * (j % 7) / 7) for j in range(256)], 1)   # [3][256]
voice_kind = rng.integers(0, 256, V)
banks = [eng.bank([Proc.BANDPASS], V) for _ in range(2)]
for b in banks:
    b.clear()
    b.set_coeffs(0, [np.ascontiguousarray(few[i][voice_kind]) for i in range(3)])
x = rng.standard_normal((C, 64 * T)).astype(np.float32)
d_rows_vm, d_rows = eng.to_device(x), eng.alloc(4 * C * 64 * T)
eng.layout_convert(d_rows_vm, Layout.VOICE_MAJOR, d_rows, Layout.QUAD, C, T)
d_exp_vm, d_exp = eng.to_device(np.ascontiguousarray(np.repeat(x, G, axis=0))), eng.alloc(4 * n)
eng.layout_convert(d_exp_vm, Layout.VOICE_MAJOR, d_exp, Layout.QUAD, V, T)
d_voices, d_two, d_one = eng.alloc(4 * n), eng.alloc(4 * C * 64 * T), eng.alloc(4 * C * 64 * T)


def one_kernel():
    banks[0].process_groups(T, d_one, G, Layout.QUAD, d_rows, Layout.QUAD, G)


def two_steps():
    banks[1].process(T, d_voices, Layout.QUAD, d_exp, Layout.QUAD)
    eng.mixdown_groups(d_voices, Layout.QUAD, C, G, T, d_two, Layout.QUAD)


one_kernel()
two_steps()
same = bool((d_one.download(np.uint32) == d_two.download(np.uint32)).all())
assert same, "the two routes differ"
for _ in range(WARMUP):
    one_kernel()
    two_steps()
eng.sync()
times = {"one": [], "two": []}
for _ in range((LAUNCHES + BLOCK - 1) // BLOCK):
    times["one"].append(eng.lap_times_ms(one_kernel, BLOCK))
    times["two"].append(eng.lap_times_ms(two_steps, BLOCK))
# (the first lap of a block starts at the block's first event: every lap is one launch's device time plus the gap in front of it)
pct = {k: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for k, v in times.items()}
count = {k: int(np.concatenate(v).size) for k, v in times.items()}
state_bytes = 4 * V * (3 + 2 + 2)   # coefficients read, state read and written
bytes_one = 4 * C * 64 * T * 2 + state_bytes                       # rows in, channels out
bytes_two = 4 * n * 3 + 4 * C * 64 * T + state_bytes              # expanded in, voices out, voices read back, channels out
name = eng.device_info()["name"]
lines = [
    "# Filter banks on a fused bank: one launch against two",
    "",
    f"`python tools/bank_groups_bench.py {V} {T} {LAUNCHES}` on {name}: `Bandpass` with per-voice coefficients, {V} voices, "
    f"`in_group = out_group = {G}`, {T} DSPVectors per launch. Both routes in one process, alternating every {BLOCK} launches after "
    f"{WARMUP} warm-up launches of each; device time per launch between events on the engine's stream. The two routes' outputs were "
    "compared first: the same bits.",
    "",
    "| route | launches | p10 us | p50 us | p90 us | signal + state bytes per launch | bytes per voice-sample | GB/s at p50 |",
    "|---|---|---|---|---|---|---|---|",
]
for key, label, nbytes in (("one", "`Bank.process_groups` (one kernel)", bytes_one), ("two", "`Bank.process` + `Engine.mixdown_groups`", bytes_two)):
    p = pct[key]
    lines.append(f"| {label} | {count[key]} | {p[0]:.1f} | {p[1]:.1f} | {p[2]:.1f} | {nbytes} | {nbytes / n:.3f} | {nbytes / p[1] / 1e3:.0f} |")
lines += ["", f"Signal bytes alone: {4 * n * 3 / (4 * C * 64 * T * 2):.0f} times fewer in one kernel. p50 of two steps over p50 of one kernel: "
          f"{pct['two'][1] / pct['one'][1]:.2f}."]
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
for b in banks:
    b.close()
eng.close()
