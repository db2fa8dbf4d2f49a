"""Developer tool: what the tails step of the intended block costs and what it buys. The `synth` workload's patch and the synthetic
performance of tools/graph_voice_list_events_bench.py, two hosts in one process:
  (b) that tool's route: route_ahead + sounding_voices + the union with every voice listed since the last look + set_voice_list +
      process_events_listed_groups; the peaks are read back - which waits for the stream - every 25 launches, between the timed runs;
  (d) VoiceTails every block: route_ahead + sounding_voices + next_list + set_voice_list + process_events_listed_groups + note, with no
      synchronisation anywhere in the loop. hold_vectors = the launch's DSPVectors: a voice leaves after one quiet launch, the rule
      (b) applies at its looks.
The routes alternate every 25 launches after 25 warm-up launches each, twice over: first with the launches back to back - the host runs
ahead of the device as far as the runtime lets it, so results are late and notes can be refused (BUSY) -, then paced, a block every
PACE microseconds, as an audio callback paces a host. Device time per launch between events on the engine's stream, p10 / p50 / p90 (paced:
the pace, not the work); K per route; the wall time of the host steps; and how many noted launches had not been taken in at each
next_list.

  python tools/voice_tails_bench.py [voices] [polyphony] [vectors] [launches per route and phase] [pace us] [--md profiles/voice_tails.md]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.sharding import cfg5_voice_params  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, P, T, LAUNCHES, PACE = (int(args[i]) if len(args) > i else d for i, d in enumerate((262144, 16, 16, 300, 3000)))
N, BLOCK, WARMUP, DEPTH, QUIET = V // P, 25, 25, 8, np.float32(1e-4).view(np.uint32)
eng = ml.Engine(0)
params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)


def rig():
    ev = ml.Events(eng, N, P, 48000.0)
    ev.configure(glide_seconds=0.01, drift=0.5)
    ev.set_wanted_rows([0, 1])
    desc, outs = patches.synth16(pitch_input=True, event_rows=True)
    g = ml.Graph(eng, V, desc, outs, output_groups={0: P}, voice_list_groups=True, voice_list_events=True)
    g.clear()
    for k, v in params.items():
        if k != "pitch":
            g.set_param(k, v if np.ndim(v) else float(v))
    for k, c in coeffs.items():
        g.set_coeffs(k, [np.ascontiguousarray(r) for r in c])
    g.set_state("noise", 0, seeds)
    g.bind_events(ev)
    ev.reserve_for_graph(T)
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
blocks = performance(1, WARMUP + 2 * laps * BLOCK)
ev_b, g_b = rig()
ev_d, g_d = rig()
d_mix = eng.alloc(4 * N * T * 64)
d_peak_b, d_peak_d = eng.alloc(4 * V), eng.alloc(4 * V)
tails = ml.VoiceTails(eng, V, V, depth=DEPTH)
tails.set_threshold(1e-4, T)
k = {"b": 0, "d": 0}
sizes = {"b": [], "d": []}
host_us = {"b": [], "d": []}
behind, busy = [], [0]
since_look = np.zeros(0, np.uint32)
last_b = np.zeros(0, np.uint32)
pace = [0.0]
due = [0.0]


def paced():
    if pace[0] > 0.0:
        while time.perf_counter() < due[0]:
            pass
        due[0] = max(due[0], time.perf_counter() - pace[0]) + pace[0]


def step_b():
    global since_look, last_b
    paced()
    ev_b.add_events_packed(blocks[k["b"]])
    t0 = time.perf_counter()
    ev_b.route_ahead(T, 0)
    L = np.union1d(ev_b.sounding_voices(), since_look).astype(np.uint32)
    since_look = L
    g_b.set_voice_list(L)
    host_us["b"].append((time.perf_counter() - t0) * 1e6)
    g_b.process_events_listed_groups(T, 0, [], [d_mix], d_peak=d_peak_b)
    ev_b.clear_events()
    last_b = L
    sizes["b"].append(L.size)
    k["b"] += 1


def look_b():
    """Between the timed runs: the voices of the last list whose peak has not died away; until the next look every voice listed since
    stays listed."""
    global since_look
    since_look = last_b[d_peak_b.download(np.uint32, last_b.size) > QUIET] if last_b.size else last_b


def step_d():
    paced()
    ev_d.add_events_packed(blocks[k["d"]])
    t0 = time.perf_counter()
    ev_d.route_ahead(T, 0)
    L = tails.next_list(ev_d.sounding_voices())
    behind.append(tails.pending)
    g_d.set_voice_list(L)
    t1 = time.perf_counter()
    g_d.process_events_listed_groups(T, 0, [], [d_mix], d_peak=d_peak_d)
    t2 = time.perf_counter()
    try:
        tails.note(T, d_peak_d)
    except ml.MlgpuError as err:
        if err.status != ml.Status.ERR_BUSY:
            raise
        busy[0] += 1
    host_us["d"].append((t1 - t0 + time.perf_counter() - t2) * 1e6)
    ev_d.clear_events()
    sizes["d"].append(L.size)
    k["d"] += 1


def run(step, n):
    due[0] = time.perf_counter()
    return eng.lap_times_ms(step, n)


def phase(pace_us):
    pace[0] = pace_us * 1e-6
    for v in (sizes, host_us):
        v["b"].clear(), v["d"].clear()
    behind.clear()
    busy[0] = 0
    times = {"b": [], "d": []}
    for _ in range(laps):
        times["b"].append(run(step_b, BLOCK))
        look_b()
        times["d"].append(run(step_d, BLOCK))
    eng.sync()
    return dict(times={r: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for r, v in times.items()},
                K={r: np.percentile(np.array(v), [10, 50, 90]) for r, v in sizes.items()},
                host={r: np.percentile(np.array(v), [50, 99]) for r, v in host_us.items()},
                behind=np.bincount(np.array(behind), minlength=DEPTH + 1), busy=busy[0], n=laps * BLOCK)


run(step_b, WARMUP)
look_b()
run(step_d, WARMUP)
eng.sync()
results = [("launches back to back", phase(0)), (f"paced, a block every {PACE} us", phase(PACE))]
label = {"b": "(b) peaks read back every 25 launches", "d": "(d) VoiceTails every block, no synchronisation"}
lines = [
    "# Voice tails: the engine tells which listed voices have died away",
    "",
    f"`python tools/voice_tails_bench.py {V} {P} {T} {LAUNCHES} {PACE}` on {eng.device_info()['name']}: the `synth` workload's patch "
    f"(`patches.synth16(pitch_input=True, event_rows=True)`, the voices summed per instrument of {P}) and its synthetic performance (every block "
    f"{max(1, N // 50)} of {N} instruments get a note on or off), V = {V} voices, {T} DSPVectors per launch. One process, two hosts with an events "
    f"object and a graph each, alternating every {BLOCK} launches after {WARMUP} warm-up launches each. (b) is the route of "
    "`tools/graph_voice_list_events_bench.py`: it reads the peaks back, which waits for the stream, every 25 launches between the timed runs, and keeps "
    f"every voice listed since. (d) calls `VoiceTails.next_list` and `note` every block (depth {DEPTH}, quiet 1e-4, hold_vectors {T}: a voice leaves "
    "after one quiet launch, the rule (b) applies at its looks) and never synchronises. Device time per launch: between events on the engine's stream, the "
    "events object's kernels, the list's upload and, for (d), the tails kernel and its copy inside; in the paced phase it is the pace, not the work.",
]
for title, r in results:
    lines += ["", f"## {title} ({r['n']} launches per route)", "",
              "| route | K p10 | K p50 | K p90 | device us p10 | p50 | p90 | host steps us p50 | p99 |", "|---|---|---|---|---|---|---|---|---|"]
    for x in "bd":
        lines.append(f"| {label[x]} | {r['K'][x][0]:.0f} | {r['K'][x][1]:.0f} | {r['K'][x][2]:.0f} | {r['times'][x][0]:.1f} | {r['times'][x][1]:.1f} | "
                     f"{r['times'][x][2]:.1f} | {r['host'][x][0]:.0f} | {r['host'][x][1]:.0f} |")
    lines += ["",
              f"K(d) / K(b) at p50 = {r['K']['d'][1] / max(r['K']['b'][1], 1):.3f}; device time (d) / (b) at p50 = {r['times']['d'][1] / r['times']['b'][1]:.3f}.",
              "",
              "Noted launches not yet taken in after each `next_list` of (d) (0 .. depth), launches counted: "
              + ", ".join(f"{i}: {c}" for i, c in enumerate(r["behind"])) + f". Notes refused with BUSY (the list then goes without peaks): {r['busy']}.",
              "",
              "Host steps: (b) route_ahead, sounding_voices, the union, set_voice_list; (d) route_ahead, sounding_voices, next_list, set_voice_list and note - "
              "wall time, the process call itself not included."]
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
for o in (tails, g_b, g_d, ev_b, ev_d):
    o.close()
eng.close()
