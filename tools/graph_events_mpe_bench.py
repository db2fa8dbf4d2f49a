"""Developer tool: what the instrument bank's event rows cost under the MPE protocol, and what the build switch
mlgpu_graph_enable_mpe_events costs a MIDI-only host. The instrument bank of `bench.py --workload synth` with the voice of
patches.synth16_mod_z (pitch, gate, z and mod), the voices summed per instrument of P. Four legs, in one process:
  (a) MPE today: Events.process writing the pitch, gate, z and mod rows of all voices on an MPE object, the graph reading them as inputs,
      then Engine.mixdown_groups - the three-kernel route, the only one an MPE object had;
  (b) Graph.process_events of the graph built with the switch, on an MPE object;
  (c) the same graph WITHOUT the switch on a MIDI object;
  (d) the graph with the switch on a MIDI object.
The performance is bench.py's in MPE clothes: every block about 2 % of the instruments get a note on or off on a member channel, a mod
controller and a channel pressure on that channel, and a pitch bend on channel 1 (the main voice; under MIDI every event goes to
channel 1 and the bend reaches all voices). The legs alternate every 25 launches after 25 warm-up launches each; device time per
launch between events on the engine's stream, launches back to back, p10 / p50 / p90.

  python tools/graph_events_mpe_bench.py [instruments] [polyphony] [vectors] [launches per leg] [--md profiles/graph_events_mpe_bench.md]

The kernels alone. `--sequential` runs the legs one after the other instead (a, b, c, d: warm-up and launches of one leg, then the
next), which is the order a kernel trace can be read in: run that under `rocprofv3 --kernel-trace --output-format csv -d DIR --`, then
  python tools/graph_events_mpe_bench.py [same numbers] --trace DIR/.../*_kernel_trace.csv [--md FILE]
prints p50 of the control kernel and of the voice kernel of each leg from the trace (no device needed)."""
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

flags = {}
args = []
it = iter(sys.argv[1:])
for a in it:
    if a in ("--md", "--trace"):
        flags[a] = next(it)
    elif a.startswith("--"):
        flags[a] = True
    else:
        args.append(a)
N, P, T, LAUNCHES = (int(args[i]) if len(args) > i else d for i, d in enumerate((16384, 16, 16, 300)))
V, BLOCK, WARMUP = N * P, 25, 25
laps = (LAUNCHES + BLOCK - 1) // BLOCK
LEGS = "abcd"
LABEL = {"a": "(a) MPE, three kernels: events.process (pitch, gate, z, mod rows) + graph.process + mixdown_groups",
         "b": "(b) MPE, process_events of the graph with the switch",
         "c": "(c) MIDI, process_events of the graph without the switch",
         "d": "(d) MIDI, process_events of the graph with the switch"}


def emit(lines):
    print("\n".join(lines))
    if "--md" in flags:
        with open(flags["--md"], "w") as f:
            f.write("\n".join(lines) + "\n")


def read_trace(path):
    """p50 per leg of the control kernel and of the voice kernel, from a kernel trace of a --sequential run: the k-th dispatch of a
    kind belongs to leg k // (WARMUP + laps * BLOCK), and a leg's first WARMUP dispatches are not counted."""
    per_leg = WARMUP + laps * BLOCK
    kinds = {"control": [], "voice": []}
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
        if "e2s_kernel" in name or "e2s_ctl" in name:
            kinds["control"].append((name, us))
        elif "mlgpu_graph_kernel" in name:
            kinds["voice"].append((name, us))
    lines = [f"Kernels alone, from a kernel trace of `--sequential` ({N} instruments x {P} voices, {T} DSPVectors per launch; the first {WARMUP} dispatches of "
             "a leg not counted). (a)'s control kernel is `e2s_kernel` writing four whole rows; its voice kernel reads them and writes the voices' audio, "
             "which `mixdown_groups` (not in this table) sums.", "",
             "| leg | control kernel | p50 us | voice kernel p50 us |", "|---|---|---|---|"]
    for i, leg in enumerate(LEGS):
        c = kinds["control"][i * per_leg + WARMUP:(i + 1) * per_leg]
        v = kinds["voice"][i * per_leg + WARMUP:(i + 1) * per_leg]
        assert len(c) == len(v) == laps * BLOCK, f"leg {leg}: {len(c)} control and {len(v)} voice dispatches in the trace, expected {laps * BLOCK} each"
        names = sorted({re.search(r"e2s_\w+", n).group(0) for n, _ in c})
        lines.append(f"| ({leg}) | `{', '.join(names)}` | {np.percentile([u for _, u in c], 50):.1f} | {np.percentile([u for _, u in v], 50):.1f} |")
    return lines


if "--trace" in flags:
    emit(read_trace(flags["--trace"]))
    sys.exit(0)

import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.constants import EventRow, Layout  # noqa: E402
from madronalib_amd.sharding import cfg5_voice_params  # noqa: E402

ROWS = [EventRow.PITCH, EventRow.GATE, EventRow.Z, EventRow.MOD]
eng = ml.Engine(0)
params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)


def rig(fused, mpe, **switches):
    ev = ml.Events(eng, N, P, 48000.0)
    ev.configure(mpe=mpe, glide_seconds=0.01, drift=0.5, mpe_pitch_bend=48.0)
    ev.set_wanted_rows(ROWS)
    desc, outs = patches.synth16_mod_z(event_rows=fused)
    g = ml.Graph(eng, V, desc, outs, output_groups={0: P} if fused else None, **switches)
    g.clear()
    for k, v in params.items():
        if k != "pitch":
            g.set_param(k, v if np.ndim(v) else float(v))
    for k, c in coeffs.items():
        g.set_coeffs(k, [np.ascontiguousarray(r) for r in c])
    g.set_state("noise", 0, seeds)
    if fused:
        g.bind_events(ev)
        ev.reserve_for_graph(T, rows=ROWS)
    return ev, g


def performance(seed, blocks, mpe):
    rng = np.random.default_rng(seed)
    held, out = {}, []
    for _ in range(blocks):
        insts, evs = [], []
        for i in rng.integers(0, N, max(1, N // 50)):
            i = int(i)
            t = int(rng.integers(0, 64 * T - 3))
            chan = int(rng.integers(2, 2 + P)) if mpe else 1
            if held.get(i):
                c, key = held[i].pop()
                evs.append(ml.Event(4, c, key, t, 0.0, 0.0))
            else:
                key = int(rng.integers(36, 84))
                held.setdefault(i, []).append((chan, key))
                evs.append(ml.Event(1, chan, key, t, (key - 60) / 12.0, 0.8))
            evs.append(ml.Event(6, chan, 16, t + 1, float(rng.random()), 0.0))        # the mod controller
            evs.append(ml.Event(9, chan, 0, t + 2, float(rng.random()), 0.0))         # channel pressure
            evs.append(ml.Event(7, 1, 0, t + 3, float(rng.uniform(-1, 1)), 0.0))      # pitch bend on channel 1
            insts += [i, i, i, i]
        out.append(ml.Events.pack_events(insts, evs))
    return out


n_blocks = WARMUP + laps * BLOCK
blocks = {True: performance(1, n_blocks, True), False: performance(1, n_blocks, False)}
rigs = {"a": rig(False, 1), "b": rig(True, 1, mpe_events=True), "c": rig(True, 0), "d": rig(True, 0, mpe_events=True)}
d_mix = eng.alloc(4 * N * T * 64)
d_voices = eng.alloc(4 * V * T * 64)
d_rows = {r: eng.alloc(4 * V * T * 64) for r in ROWS}
by_name = dict(pitch=EventRow.PITCH, gate=EventRow.GATE, z=EventRow.Z, mod=EventRow.MOD)
inputs_a = [d_rows[by_name[nm]] for nm in rigs["a"][1].inputs]
k = {leg: 0 for leg in LEGS}


def step(leg):
    ev, g = rigs[leg]
    ev.add_events_packed(blocks[leg in "ab"][k[leg]])
    if leg == "a":
        ev.process(T, 0, [d_rows.get(r) for r in range(8)], Layout.QUAD)
        g.process(T, inputs_a, [d_voices])
        eng.mixdown_groups(d_voices, Layout.QUAD, N, P, T, d_mix)
    else:
        g.process_events(T, 0, [], [d_mix])
    ev.clear_events()
    k[leg] += 1


times = {leg: [] for leg in LEGS}
if "--sequential" in flags:
    for leg in LEGS:
        for _ in range(WARMUP):
            step(leg)
        eng.sync()
        for _ in range(laps):
            times[leg].append(eng.lap_times_ms(lambda: step(leg), BLOCK))
else:
    for _ in range(WARMUP):
        for leg in LEGS:
            step(leg)
    eng.sync()
    for _ in range(laps):
        for leg in LEGS:
            times[leg].append(eng.lap_times_ms(lambda: step(leg), BLOCK))
pct = {leg: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for leg, v in times.items()}
order = "one after the other (--sequential: the order of a kernel trace; take the block times from a run without it)" if "--sequential" in flags \
    else f"alternating every {BLOCK} launches after {WARMUP} warm-up launches each"
lines = [
    f"`python tools/graph_events_mpe_bench.py {N} {P} {T} {LAUNCHES}` on {eng.device_info()['name']}: `patches.synth16_mod_z`, {N} instruments x {P} voices "
    f"summed per instrument, {T} DSPVectors per launch; every block {max(1, N // 50)} instruments get a note on or off, a mod controller, a channel "
    f"pressure and a channel-1 pitch bend. One process, the legs {order}; device time per launch between events on the engine's stream (the events "
    "object's kernels and the uploads are inside).",
    "",
    f"Reserve of the events object, `Events.graph_reserve_bytes({T}, rows)`: MPE {rigs['b'][0].graph_reserve_bytes(T, ROWS)} bytes "
    f"({N} x {rigs['b'][0].graph_reserve_bytes(1, ROWS) // (1048 * N)} lanes), MIDI {rigs['c'][0].graph_reserve_bytes(T, ROWS)} bytes.",
    "",
    "| leg | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|",
]
for leg in LEGS:
    lines.append(f"| {LABEL[leg]} | {np.concatenate(times[leg]).size} | {pct[leg][0]:.1f} | {pct[leg][1]:.1f} | {pct[leg][2]:.1f} |")
lines += ["", f"(b)/(a) = {pct['b'][1] / pct['a'][1]:.3f}, (d)/(c) = {pct['d'][1] / pct['c'][1]:.3f}, (b)/(c) = {pct['b'][1] / pct['c'][1]:.3f} at p50."]
emit(lines)
for ev, g in rigs.values():
    g.close()
    ev.close()
eng.close()
