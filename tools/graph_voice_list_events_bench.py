"""Developer tool: what the instrument bank costs when it runs only the voices that sound. The `synth` workload of bench.py - its
patch (patches.synth16(pitch_input=True, event_rows=True), the voices summed per instrument of P) and its synthetic performance (every
block about 2 % of the instruments get a note on or off) - three ways, in one process:
  (a) today's Graph.process_events of all V voices;
  (b) Events.route_ahead + Events.sounding_voices + the host's tails + Graph.set_voice_list + Graph.process_events_listed_groups;
  (c) Events.process writing the pitch and gate rows of all voices, then Graph.process_listed_groups of the twin graph that reads them as
      inputs, with the same lists.
The tails: a voice stays listed until its peak (d_peak) has fallen below 1e-4 - profiles/voice_list.md. Reading the peaks back waits
for the stream, so this tool looks at them every 25 launches, between the timed runs (a host looks a block late, from a pinned copy):
a released voice stays listed for up to 25 launches, which makes K a little larger than a host's. The routes alternate every 25
launches after 25 warm-up launches each; device time per launch between events on the engine's stream, launches back to back, p10 /
p50 / p90; for (b) the wall time of its host steps per block, p50 / p99.

  python tools/graph_voice_list_events_bench.py [voices] [polyphony] [vectors] [launches per route] [--md profiles/graph_voice_list_events.md]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.constants import Layout  # noqa: E402
from madronalib_amd.sharding import cfg5_voice_params  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, P, T, LAUNCHES = (int(args[i]) if len(args) > i else d for i, d in enumerate((262144, 16, 16, 300)))
N, BLOCK, WARMUP, QUIET = V // P, 25, 25, np.float32(1e-4).view(np.uint32)
eng = ml.Engine(0)
params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)


def rig(fused, **switches):
    ev = ml.Events(eng, N, P, 48000.0)
    ev.configure(glide_seconds=0.01, drift=0.5)
    ev.set_wanted_rows([0, 1])
    desc, outs = patches.synth16(pitch_input=True, event_rows=fused)
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
        ev.reserve_for_graph(T)
    if switches:
        g.reserve_voice_list_groups(V)
    return ev, g


def performance(seed, blocks):
    """bench.py's: every block max(1, N / 50) instruments get a note - on if they hold none, else the held one off."""
    rng = np.random.default_rng(seed)
    held, out = {}, []
    for _ in range(blocks):
        insts, evs = [], []
        for i in rng.integers(0, N, max(1, N // 50)):
            i = int(i)
            t = int(rng.integers(0, 64 * T))
            insts.append(i)
            if held.get(i):
                evs.append(ml.Event(4, 1, held[i].pop(), t, 0.0, 0.0))
            else:
                key = int(rng.integers(36, 84))
                held.setdefault(i, []).append(key)
                evs.append(ml.Event(1, 1, key, t, (key - 60) / 12.0, 0.8))
        out.append(ml.Events.pack_events(insts, evs))
    return out


laps = (LAUNCHES + BLOCK - 1) // BLOCK
blocks = performance(1, WARMUP + laps * BLOCK)
ev_a, g_a = rig(True)
ev_b, g_b = rig(True, voice_list_groups=True, voice_list_events=True)
ev_c, g_c = rig(False, voice_list_groups=True)
d_mix = eng.alloc(4 * N * T * 64)
d_rows = [eng.alloc(4 * V * T * 64), eng.alloc(4 * V * T * 64)]
d_peak = eng.alloc(4 * V)
names = g_c.inputs
lists, host_us, k = [], [], {"a": 0, "b": 0, "c": 0}
tails = np.zeros(0, np.uint32)


def step_a():
    ev_a.add_events_packed(blocks[k["a"]])
    g_a.process_events(T, 0, [], [d_mix])
    ev_a.clear_events()
    k["a"] += 1


def step_b():
    global tails
    ev_b.add_events_packed(blocks[k["b"]])
    t0 = time.perf_counter()
    ev_b.route_ahead(T, 0)
    L = np.union1d(ev_b.sounding_voices(), tails).astype(np.uint32)
    tails = L
    g_b.set_voice_list(L)
    host_us.append((time.perf_counter() - t0) * 1e6)
    g_b.process_events_listed_groups(T, 0, [], [d_mix], d_peak=d_peak)
    ev_b.clear_events()
    lists.append(L)
    k["b"] += 1


def read_tails():
    """Between the timed runs: the voices of the last list whose peak has not died away; until the next look every voice listed since
    stays listed (step_b's union with the list before)."""
    global tails
    L = lists[-1]
    tails = L[d_peak.download(np.uint32, L.size) > QUIET] if L.size else L


def step_c():
    ev_c.add_events_packed(blocks[k["c"]])
    g_c.set_voice_list(lists[k["c"]])
    ev_c.process(T, 0, d_rows + [None] * 6, Layout.QUAD)
    ev_c.clear_events()
    g_c.process_listed_groups(T, [d_rows[1] if nm == "gate" else d_rows[0] for nm in names], [d_mix], d_peak=d_peak)
    k["c"] += 1


def run_b(n):
    out = eng.lap_times_ms(step_b, n)
    read_tails()
    return out


run_b(WARMUP)
for _ in range(WARMUP):
    step_a()
    step_c()
eng.sync()
host_us.clear()
times = {"a": [], "b": [], "c": []}
for _ in range(laps):
    times["a"].append(eng.lap_times_ms(step_a, BLOCK))
    times["b"].append(run_b(BLOCK))
    times["c"].append(eng.lap_times_ms(step_c, BLOCK))
pct = {r: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for r, v in times.items()}
ks = np.array([L.size for L in lists[WARMUP:]])
js = np.array([np.unique(L // P).size for L in lists[WARMUP:]])
label = {"a": "(a) process_events, all V voices", "b": "(b) route_ahead + sounding_voices + tails + set_voice_list + process_events_listed_groups",
         "c": "(c) events.process (two rows, V voices) + process_listed_groups of the twin graph, the same lists"}
lines = [
    "# Voice lists for graphs with event rows: the instrument bank runs the voices that sound",
    "",
    f"`python tools/graph_voice_list_events_bench.py {V} {P} {T} {LAUNCHES}` on {eng.device_info()['name']}: the `synth` workload's patch "
    f"(`patches.synth16(pitch_input=True, event_rows=True)`, the voices summed per instrument of {P}) and its synthetic performance (every block "
    f"{max(1, N // 50)} of {N} instruments get a note on or off), V = {V} voices, {T} DSPVectors per launch. One process, the routes alternating every "
    f"{BLOCK} launches after {WARMUP} warm-up launches each; device time per launch between events on the engine's stream (for (b) and (c) the events "
    "object's kernels and the list's upload are inside).",
    "",
    f"K/V of the performance over the measured launches: K p10 / p50 / p90 = {np.percentile(ks, 10):.0f} / {np.percentile(ks, 50):.0f} / {np.percentile(ks, 90):.0f} "
    f"listed voices (K/V = {np.percentile(ks, 50) / V:.4f} at p50), J p50 = {np.percentile(js, 50):.0f} listed instruments of {N}. The tails: a voice stays "
    f"listed until its peak is below 1e-4, looked at every {BLOCK} launches (between the timed runs).",
    "",
    "| route | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|",
]
for r in "abc":
    lines.append(f"| {label[r]} | {np.concatenate(times[r]).size} | {pct[r][0]:.1f} | {pct[r][1]:.1f} | {pct[r][2]:.1f} |")
h = np.percentile(np.array(host_us), [50, 99])
lines += ["",
          f"(b)/(a) = {pct['b'][1] / pct['a'][1]:.3f}, (b)/(c) = {pct['b'][1] / pct['c'][1]:.3f} at p50.",
          "",
          f"(b)'s host steps per block (route_ahead, sounding_voices, the union with the tails, set_voice_list - wall time): p50 {h[0]:.0f} us, p99 {h[1]:.0f} us. "
          "The read-back of the peaks that makes the tails is outside the timed launches. Where these steps take longer than the launch's kernels the stream "
          "waits for the host, and the device time between events is the host's time."]
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
for o in (g_a, g_b, g_c, ev_a, ev_b, ev_c):
    o.close()
eng.close()
