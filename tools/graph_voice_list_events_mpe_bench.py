"""Developer tool: what an MPE instrument bank costs when it runs only the voices that sound. The instrument bank with the voice of
patches.synth16_mod_z (pitch, gate, z and mod as event rows), the voices summed per instrument of P, on an MPE events object - three
legs, in one process:
  (a) Graph.process_events of all V voices, the graph built with mpe_events only;
  (b) the listed block: Events.route_ahead + Events.sounding_graph_voices + the host's tails + Graph.set_voice_list +
      Graph.process_events_listed_groups, the graph built with voice_list_mpe_events;
  (c) the route an MPE host had before: Events.process writing the pitch, gate, z and mod rows of all voices, then
      Graph.process_listed_groups of the twin graph that reads them as inputs, with the same lists.
The performance is tools/graph_events_mpe_bench.py's: every block about 2 % of the instruments get a note on or off on a member
channel, a mod controller and a channel pressure on that channel, and a pitch bend on channel 1. `--held H`: every instrument also
holds H notes from the first block on (H = 2 of 16 voices: about V / 8 voices sound).
The tails: a voice stays listed until its peak (d_peak) has fallen below 1e-4, looked at every 25 launches, between the timed runs
(tools/graph_voice_list_events_bench.py). The legs alternate every 25 launches after 25 warm-up launches each; device time per launch
between events on the engine's stream, launches back to back, p10 / p50 / p90; for (b) the wall time of its host steps per block.

  python tools/graph_voice_list_events_mpe_bench.py [instruments] [polyphony] [vectors] [launches per leg] [--held H] [--md FILE]

The kernels alone. `--sequential` runs the legs one after the other (a, b, c), the order a kernel trace can be read in: run that under
`rocprofv3 --kernel-trace --output-format csv -d DIR --`, then
  python tools/graph_voice_list_events_mpe_bench.py [same numbers] --trace DIR/.../*_kernel_trace.csv [--md FILE]
prints p50 of the control kernel and of the voice kernel of each leg from the trace (no device needed)."""
import csv
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

flags = {}
args = []
it = iter(sys.argv[1:])
for a in it:
    if a in ("--md", "--trace", "--held"):
        flags[a] = next(it)
    elif a.startswith("--"):
        flags[a] = True
    else:
        args.append(a)
N, P, T, LAUNCHES = (int(args[i]) if len(args) > i else d for i, d in enumerate((16384, 16, 16, 300)))
HELD = int(flags.get("--held", 0))
V, BLOCK, WARMUP, QUIET = N * P, 25, 25, np.float32(1e-4).view(np.uint32)
laps = (LAUNCHES + BLOCK - 1) // BLOCK
LEGS = "abc"
LABEL = {"a": "(a) process_events, all V voices (mpe_events)",
         "b": "(b) route_ahead + sounding_graph_voices + tails + set_voice_list + process_events_listed_groups (voice_list_mpe_events)",
         "c": "(c) events.process (four rows, V voices) + process_listed_groups of the twin graph, the same lists"}


def emit(lines):
    print("\n".join(lines))
    if "--md" in flags:
        with open(flags["--md"], "w") as f:
            f.write("\n".join(lines) + "\n")


def read_trace(path):
    """p50 per leg of the control kernel and of the voice kernel, from a kernel trace of a --sequential run: every launch of a leg
    has one control kernel (e2s_ctl_rows_mpe_kernel, or (c)'s e2s_kernel) and one voice kernel; the k-th dispatch of a kind belongs to
    leg k // (WARMUP + laps * BLOCK), and a leg's first WARMUP dispatches are not counted."""
    per_leg = WARMUP + laps * BLOCK
    control, voice = [], []
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name, us = r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
        if "e2s_kernel" in name or "e2s_ctl" in name:
            control.append((name, us))
        elif "mlgpu_graph_kernel" in name or "mlgpu_graph_listed_kernel" in name:
            voice.append((name, us))
    lines = [f"Kernels alone, from a kernel trace of `--sequential` ({N} instruments x {P} voices, {T} DSPVectors per launch, {HELD} held notes per "
             f"instrument; the first {WARMUP} dispatches of a leg not counted).", "",
             "| leg | control kernel | p50 us | voice kernel | p50 us |", "|---|---|---|---|---|"]
    for i, leg in enumerate(LEGS):
        c = control[i * per_leg + WARMUP:(i + 1) * per_leg]
        v = voice[i * per_leg + WARMUP:(i + 1) * per_leg]
        assert len(c) == len(v) == laps * BLOCK, f"leg {leg}: {len(c)} control and {len(v)} voice dispatches in the trace, expected {laps * BLOCK} each"
        cn = sorted({re.search(r"e2s_\w+", n).group(0) for n, _ in c})
        vn = sorted({re.search(r"mlgpu_graph_\w+", n).group(0) for n, _ in v})
        lines.append(f"| ({leg}) | `{', '.join(cn)}` | {np.percentile([u for _, u in c], 50):.1f} | `{', '.join(vn)}` | {np.percentile([u for _, u in v], 50):.1f} |")
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


def rig(fused, **switches):
    ev = ml.Events(eng, N, P, 48000.0)
    ev.configure(mpe=1, glide_seconds=0.01, drift=0.5, mpe_pitch_bend=48.0)
    ev.set_wanted_rows(ROWS)
    desc, outs = patches.synth16_mod_z(event_rows=fused)
    g = ml.Graph(eng, V, desc, outs, output_groups={0: P}, **switches)
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
    if switches.get("voice_list_groups"):
        g.reserve_voice_list_groups(V)
    return ev, g


def performance(seed, blocks):
    rng = np.random.default_rng(seed)
    held, out = {}, []
    for b in range(blocks):
        insts, evs = [], []
        if b == 0:      # --held: H notes per instrument on the last member channels, never released
            for i in range(N):
                for h in range(HELD):
                    evs.append(ml.Event(1, 2 + P - 1 - h, 48 + h, h, (h - 12) / 12.0, 0.8))
                    insts.append(i)
        for i in rng.integers(0, N, max(1, N // 50)):
            i = int(i)
            t = int(rng.integers(HELD, 64 * T - 3))
            chan = int(rng.integers(2, 2 + P - HELD))
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


blocks = performance(1, WARMUP + laps * BLOCK)
rigs = {"a": rig(True, mpe_events=True), "b": rig(True, voice_list_groups=True, voice_list_mpe_events=True), "c": rig(False, voice_list_groups=True)}
assert "mlev::CtlVoiceMpe ev_0;" in rigs["b"][1].listed_source()
d_mix = eng.alloc(4 * N * T * 64)
d_rows = {r: eng.alloc(4 * V * T * 64) for r in ROWS}
d_peak = eng.alloc(4 * V)
by_name = dict(pitch=EventRow.PITCH, gate=EventRow.GATE, z=EventRow.Z, mod=EventRow.MOD)
inputs_c = [d_rows[by_name[nm]] for nm in rigs["c"][1].inputs]
lists, host_us, k = [], [], {leg: 0 for leg in LEGS}
tails = np.zeros(0, np.uint32)


def step_a():
    ev, g = rigs["a"]
    ev.add_events_packed(blocks[k["a"]])
    g.process_events(T, 0, [], [d_mix])
    ev.clear_events()
    k["a"] += 1


def step_b():
    global tails
    ev, g = rigs["b"]
    ev.add_events_packed(blocks[k["b"]])
    t0 = time.perf_counter()
    ev.route_ahead(T, 0)
    L = np.union1d(ev.sounding_graph_voices(), tails).astype(np.uint32)
    tails = L
    g.set_voice_list(L)
    host_us.append((time.perf_counter() - t0) * 1e6)
    g.process_events_listed_groups(T, 0, [], [d_mix], d_peak=d_peak)
    ev.clear_events()
    lists.append(L)
    k["b"] += 1


def read_tails():
    """Between the timed runs: the voices of the last list whose peak has not died away; until the next look every voice listed since
    stays listed (step_b's union with the list before)."""
    global tails
    L = lists[-1]
    tails = L[d_peak.download(np.uint32, L.size) > QUIET] if L.size else L


def step_c():
    ev, g = rigs["c"]
    ev.add_events_packed(blocks[k["c"]])
    g.set_voice_list(lists[k["c"]])
    ev.process(T, 0, [d_rows.get(r) for r in range(8)], Layout.QUAD)
    ev.clear_events()
    g.process_listed_groups(T, inputs_c, [d_mix], d_peak=d_peak)
    k["c"] += 1


def run_b(n):
    out = eng.lap_times_ms(step_b, n)
    read_tails()
    return out


times = {leg: [] for leg in LEGS}
if "--sequential" in flags:      # (b before c: c runs b's lists)
    for leg, run in (("a", lambda n: eng.lap_times_ms(step_a, n)), ("b", run_b), ("c", lambda n: eng.lap_times_ms(step_c, n))):
        run(WARMUP)
        eng.sync()
        if leg == "b":
            host_us.clear()
        for _ in range(laps):
            times[leg].append(run(BLOCK))
else:
    run_b(WARMUP)
    for _ in range(WARMUP):
        step_a()
        step_c()
    eng.sync()
    host_us.clear()
    for _ in range(laps):
        times["a"].append(eng.lap_times_ms(step_a, BLOCK))
        times["b"].append(run_b(BLOCK))
        times["c"].append(eng.lap_times_ms(step_c, BLOCK))
pct = {leg: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for leg, v in times.items()}
ks = np.array([L.size for L in lists[WARMUP:]])
js = np.array([np.unique(L // P).size for L in lists[WARMUP:]])
order = "one after the other (--sequential: the order of a kernel trace; take the block times from a run without it)" if "--sequential" in flags \
    else f"alternating every {BLOCK} launches after {WARMUP} warm-up launches each"
lines = [
    f"`python tools/graph_voice_list_events_mpe_bench.py {N} {P} {T} {LAUNCHES}{' --held ' + str(HELD) if HELD else ''}` on {eng.device_info()['name']}: "
    f"`patches.synth16_mod_z`, {N} instruments x {P} voices summed per instrument, MPE, {T} DSPVectors per launch; every block {max(1, N // 50)} instruments "
    f"get a note on or off, a mod controller, a channel pressure and a channel-1 pitch bend{', and every instrument holds ' + str(HELD) + ' notes' if HELD else ''}. "
    f"One process, the legs {order}; device time per launch between events on the engine's stream (the events object's kernels, the uploads and the "
    "list's upload are inside).",
    "",
    f"K over the measured launches: K p10 / p50 / p90 = {np.percentile(ks, 10):.0f} / {np.percentile(ks, 50):.0f} / {np.percentile(ks, 90):.0f} listed voices "
    f"(K/V = {np.percentile(ks, 50) / V:.4f} at p50), J p50 = {np.percentile(js, 50):.0f} listed instruments of {N}. The tails: a voice stays listed until "
    f"its peak is below 1e-4, looked at every {BLOCK} launches (between the timed runs).",
    "",
    "| leg | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|",
]
for leg in LEGS:
    lines.append(f"| {LABEL[leg]} | {np.concatenate(times[leg]).size} | {pct[leg][0]:.1f} | {pct[leg][1]:.1f} | {pct[leg][2]:.1f} |")
h = np.percentile(np.array(host_us), [50, 99])
lines += ["", f"(b)/(a) = {pct['b'][1] / pct['a'][1]:.3f}, (b)/(c) = {pct['b'][1] / pct['c'][1]:.3f} at p50.", "",
          f"(b)'s host steps per block (route_ahead, sounding_graph_voices, the union with the tails, set_voice_list - wall time): p50 {h[0]:.0f} us, "
          f"p99 {h[1]:.0f} us. The read-back of the peaks that makes the tails is outside the timed launches."]
emit(lines)
for ev, g in rigs.values():
    g.close()
    ev.close()
eng.close()
