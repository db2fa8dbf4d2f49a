"""Developer tool: what a voice that reads the mod wheel and aftertouch costs, the instrument bank of `bench.py --workload synth` with the
voice of patches.synth16_mod_z (the filter input scaled by 1 + mod, z added to the amp envelope), the voices summed per instrument of
P. Three forms, in one process:
  (a) Events.process writing the gate, pitch, z and mod rows of all voices, the graph reading them as inputs, then
      Engine.mixdown_groups - the only form there was before the rows z and mod could be source nodes;
  (b) Graph.process_events of the graph whose gate, pitch, z and mod are event rows, the sum made in the voice kernel;
  (c) (b) for the voices that sound: Events.route_ahead + Events.sounding_voices + a fixed tail + Graph.set_voice_list +
      Graph.process_events_listed_groups.
The performance is bench.py's - every block about 2 % of the instruments get a note on or off - and each of those instruments also gets
a mod-wheel event (controller 16) and a channel pressure in the block, so both glides move in about 2 % of the instruments at any time.
(c)'s list is sounding_voices() united with the sets of the two launches before (a fixed tail of two launches: with z added to the
envelope a voice under channel pressure never falls silent, so the peak rule of tools/graph_voice_list_events_bench.py would keep
nearly every voice listed). The forms alternate every 25 launches after 25 warm-up launches each; device time per launch
between events on the engine's stream, launches back to back, p10 / p50 / p90.

  python tools/graph_event_rows_bench.py [voices] [polyphony] [vectors] [launches per form] [--md profiles/graph_event_rows_bench.md]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.constants import EventRow, Layout  # noqa: E402
from madronalib_amd.sharding import cfg5_voice_params  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, P, T, LAUNCHES = (int(args[i]) if len(args) > i else d for i, d in enumerate((262144, 16, 16, 300)))
N, BLOCK, WARMUP = V // P, 25, 25
ROWS = [EventRow.PITCH, EventRow.GATE, EventRow.Z, EventRow.MOD]
eng = ml.Engine(0)
params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)


def rig(fused, **switches):
    ev = ml.Events(eng, N, P, 48000.0)
    ev.configure(glide_seconds=0.01, drift=0.5)
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
    if switches:
        g.reserve_voice_list_groups(V)
    return ev, g


def performance(seed, blocks):
    rng = np.random.default_rng(seed)
    held, out = {}, []
    for _ in range(blocks):
        insts, evs = [], []
        for i in rng.integers(0, N, max(1, N // 50)):
            i = int(i)
            t = int(rng.integers(0, 64 * T - 2))
            if held.get(i):
                evs.append(ml.Event(4, 1, held[i].pop(), t, 0.0, 0.0))
            else:
                key = int(rng.integers(36, 84))
                held.setdefault(i, []).append(key)
                evs.append(ml.Event(1, 1, key, t, (key - 60) / 12.0, 0.8))
            evs.append(ml.Event(6, 1, 16, t + 1, float(rng.random()), 0.0))     # the mod wheel
            evs.append(ml.Event(9, 1, 0, t + 2, float(rng.random()), 0.0))      # channel pressure
            insts += [i, i, i]
        out.append(ml.Events.pack_events(insts, evs))
    return out


laps = (LAUNCHES + BLOCK - 1) // BLOCK
blocks = performance(1, WARMUP + laps * BLOCK)
ev_a, g_a = rig(False)
ev_b, g_b = rig(True)
ev_c, g_c = rig(True, voice_list_groups=True, voice_list_events=True)
d_mix = eng.alloc(4 * N * T * 64)
d_voices = eng.alloc(4 * V * T * 64)
d_rows = {r: eng.alloc(4 * V * T * 64) for r in ROWS}
d_peak = eng.alloc(4 * V)
by_name = dict(pitch=EventRow.PITCH, gate=EventRow.GATE, z=EventRow.Z, mod=EventRow.MOD)
inputs_a = [d_rows[by_name[nm]] for nm in g_a.inputs]
lists, sets, k = [], [], {"a": 0, "b": 0, "c": 0}


def step_a():
    ev_a.add_events_packed(blocks[k["a"]])
    ev_a.process(T, 0, [d_rows.get(r) for r in range(8)], Layout.QUAD)
    ev_a.clear_events()
    g_a.process(T, inputs_a, [d_voices])
    eng.mixdown_groups(d_voices, Layout.QUAD, N, P, T, d_mix)
    k["a"] += 1


def step_b():
    ev_b.add_events_packed(blocks[k["b"]])
    g_b.process_events(T, 0, [], [d_mix])
    ev_b.clear_events()
    k["b"] += 1


def step_c():
    ev_c.add_events_packed(blocks[k["c"]])
    ev_c.route_ahead(T, 0)
    sets.append(ev_c.sounding_voices())
    L = np.unique(np.concatenate(sets[-3:])).astype(np.uint32)
    g_c.set_voice_list(L)
    g_c.process_events_listed_groups(T, 0, [], [d_mix], d_peak=d_peak)
    ev_c.clear_events()
    lists.append(L)
    k["c"] += 1


eng.lap_times_ms(step_c, WARMUP)
for _ in range(WARMUP):
    step_a()
    step_b()
eng.sync()
times = {"a": [], "b": [], "c": []}
for _ in range(laps):
    times["a"].append(eng.lap_times_ms(step_a, BLOCK))
    times["b"].append(eng.lap_times_ms(step_b, BLOCK))
    times["c"].append(eng.lap_times_ms(step_c, BLOCK))
pct = {r: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for r, v in times.items()}
ks = np.array([L.size for L in lists[WARMUP:]])
label = {"a": "(a) events.process (gate, pitch, z, mod rows of V voices) + graph.process + mixdown_groups",
         "b": "(b) process_events: the four rows made in the voice kernel, all V voices",
         "c": "(c) route_ahead + sounding_voices + the two launches before + set_voice_list + process_events_listed_groups"}
lines = [
    f"`python tools/graph_event_rows_bench.py {V} {P} {T} {LAUNCHES}` on {eng.device_info()['name']}: `patches.synth16_mod_z`, the voices summed per "
    f"instrument of {P}, V = {V} voices, {T} DSPVectors per launch; every block {max(1, N // 50)} of {N} instruments get a note on or off, a mod-wheel "
    f"event and a channel pressure. One process, the forms alternating every {BLOCK} launches after {WARMUP} warm-up launches each; device time per "
    "launch between events on the engine's stream (the events object's kernels, the uploads and for (c) the list's upload are inside).",
    "",
    f"Reserve of the events object for (b) and (c), `Events.graph_reserve_bytes({T}, rows)`: {ev_b.graph_reserve_bytes(T, ROWS)} bytes "
    f"(pitch and gate alone: {ev_b.graph_reserve_bytes(T)}). (c)'s list over the measured launches: K p10 / p50 / p90 = "
    f"{np.percentile(ks, 10):.0f} / {np.percentile(ks, 50):.0f} / {np.percentile(ks, 90):.0f} listed voices (K/V = {np.percentile(ks, 50) / V:.4f} at p50).",
    "",
    "| form | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|",
]
for r in "abc":
    lines.append(f"| {label[r]} | {np.concatenate(times[r]).size} | {pct[r][0]:.1f} | {pct[r][1]:.1f} | {pct[r][2]:.1f} |")
lines += ["", f"(b)/(a) = {pct['b'][1] / pct['a'][1]:.3f}, (c)/(b) = {pct['c'][1] / pct['b'][1]:.3f} at p50."]
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
for o in (g_a, g_b, g_c, ev_a, ev_b, ev_c):
    o.close()
eng.close()
