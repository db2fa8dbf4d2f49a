"""Developer tool: what a listed launch of a graph with delay rings costs in each ring layout (mlgpu_graph_enable_voice_list_rings).

Two workloads of bench.py, per-voice delay times as there: the plucked-string bank (`--workload strings`: one FractionalDelay ring,
262 144 voices) in ring layouts 0, 1 and 4, and four Allpass<PitchbendableDelay> in series (`--workload allpass4`, 131 072 voices) in
layouts 0 and 4. Per graph: Graph.process_listed with every voice listed, with a seeded random quarter and with a random sixteenth,
next to Graph.process of all voices in the same layout (on that bank, and on a bank from clear). Before anything is timed the lists
ROTATE: warm-up launches of 1, 2, 3 and 5 DSPVectors with a fresh random half of the voices each, so that the write indices of a
wavefront's voices differ by multiples of 64 - what a bank of sounding voices looks like. The rows of one workload alternate
inside one process, 10 launches at a time; device time per launch between events on the engine's stream (Engine.lap_times_ms), p10 / p50 / p90. Bytes per second: the algorithmic bytes of
the K listed voices (bench.py's count: in + out + each ring's write and read + each kept DSPVector's read and write) over p50.
Last, one A/B of layout 4's aligned test in the listed kernel: each lane on a sector boundary (the default) against the plain
kernel's test, equal write indices in the wavefront (MLGPU_GRAPH_RING_LANE_CLOCK=0), on the rotated strings bank.

  python tools/graph_voice_list_rings_bench.py [launches per row] [--small] [--md profiles/graph_voice_list_rings.md]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.constants import Layout, Op, Proc  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
SMALL = "--small" in sys.argv     # a rehearsal size, not a measurement
LAUNCHES = int(args[0]) if args else 100
T, BLOCK, HBM_PEAK = 16, 10, 8.0e12
SIZES = {"strings": 4096 if SMALL else 262144, "allpass4": 2048 if SMALL else 131072}
BYTES_PER_VOICE_SAMPLE = {"strings": 8.0 + 8.0 + 8.0, "allpass4": 8.0 + 4 * (2 * 8.0 + 8.0)}

eng = ml.Engine(0)


def strings_graph(V, layout, listed):
    desc = [dict(name="x", type="input"), dict(name="g", type="const", value=0.995),
            dict(name="fb", type="feedback", source="damp"),
            dict(name="fbg", type="op", kind=Op.MULTIPLY, inputs=["fb", "g"]),
            dict(name="sum", type="op", kind=Op.ADD, inputs=["x", "fbg"]),
            dict(name="line", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=["sum"], max_delay=1024.0),
            dict(name="damp", type="proc", kind=Proc.ONE_POLE, inputs=["line"])]
    g = ml.Graph(eng, V, desc, ["damp"], delay_windows=layout, voice_lists=listed, voice_list_rings=bool(listed and layout))
    g.clear()
    g.set_coeffs("damp", ml.OnePole.makeCoeffs(0.3))
    length = 48000.0 / (46.0 * 2.0 ** (4.0 * ((np.arange(V) * 7919) % V) / V)) - 64.0   # 46 Hz .. 736 Hz, scattered over the voices
    rounded = np.round(length, 2)
    uniq, inverse = np.unique(rounded, return_inverse=True)
    words = np.stack([ml.FractionalDelay.makeState(float(d)) for d in uniq]).astype(np.float32)[inverse]   # [V][2]: delayInt bits, allpass coefficient
    g.set_state("line", 3, np.ascontiguousarray(words[:, 0]).view(np.uint32))
    g.set_state("line", 4, np.ascontiguousarray(words[:, 1]).view(np.uint32))
    return g


def allpass4_graph(V, layout, listed):
    desc = [dict(name="x", type="input"), dict(name="dl", type="param")]
    src = "x"
    for j in range(4):
        sub, src = patches.allpass(f"ap{j}_", src, Proc.PITCHBENDABLE_DELAY, 4096.0 - 64.0, "dl")
        desc += sub
    g = ml.Graph(eng, V, desc, [src], delay_windows=layout, voice_lists=listed, voice_list_rings=bool(listed and layout))
    g.clear()
    for j in range(4):
        g.set_param(f"ap{j}_gain", 0.6)
    g.set_param("dl", (400.0 + 3000.0 * (np.arange(V) % 97) / 96.0).astype(np.float32))
    return g


MAKE = {"strings": (strings_graph, "line"), "allpass4": (allpass4_graph, "ap0_delay")}


def pcts(laps):
    return np.percentile(np.concatenate(laps) * 1000.0, [10, 50, 90])


def rotate(g, V, d_x, d_out, seed):
    """The warm-up in which lists rotate: launches of 1, 2, 3 and 5 DSPVectors, each with a fresh random half of the voices."""
    rng = np.random.default_rng(seed)
    for n in (1, 2, 3, 5, 2, 1, 3, 5):
        g.set_voice_list(np.sort(rng.choice(V, V // 2, replace=False)).astype(np.uint32))
        g.process_listed(n, [d_x], [d_out], Layout.QUAD, Layout.QUAD)
    eng.sync()


def measure(routes):
    """{label: (setup, work)} -> {label: [p10, p50, p90] us}: a warm-up block of each, then the routes alternating, BLOCK launches at a
    time. setup() runs before each block, outside the timed laps (the list's upload is not the launch's time)."""
    for setup, work in routes.values():
        setup()
        for _ in range(BLOCK):
            work()
    eng.sync()
    laps = {k: [] for k in routes}
    for _ in range((LAUNCHES + BLOCK - 1) // BLOCK):
        for k, (setup, work) in routes.items():
            setup()
            eng.sync()
            laps[k].append(eng.lap_times_ms(work, BLOCK))
    return {k: pcts(v) for k, v in laps.items()}


def noise(V):
    nb = eng.bank([Proc.NOISE_GEN], V)
    nb.set_state(0, 0, np.arange(V, dtype=np.uint32))
    d_x = eng.alloc(4 * V * T * 64)
    nb.process(T, d_x, Layout.QUAD)
    eng.sync()
    nb.close()
    return d_x


name = eng.device_info()["name"].strip() or "an MI355X"
lines = [
    "# Listed launches of graphs with delay rings, by ring layout",
    "",
    f"`python tools/graph_voice_list_rings_bench.py {LAUNCHES}` on {name}: bench.py's plucked-string bank (one FractionalDelay ring, V = {SIZES['strings']}) and its "
    f"four Allpass<PitchbendableDelay> in series (eight rings, V = {SIZES['allpass4']}), per-voice delay times, {T} DSPVectors per launch, QUAD in and out. "
    "`process_listed` with all voices, a seeded random quarter and a random sixteenth listed, next to `process` of all voices in the same layout - on the same bank and on a bank "
    "from clear, where all write indices are equal (layouts 1 and 4 under `mlgpu_graph_enable_voice_list_rings`). Before the timing the lists rotate - launches of 1, 2, 3 and 5 DSPVectors with a "
    "fresh random half of the voices each - so the write indices differ by voice. The list is set before each block of launches, outside the timed laps. One process per workload, the rows alternating every "
    f"{BLOCK} launches after {BLOCK} warm-up launches of each; device time per launch between events on the engine's stream. GB/s: the algorithmic "
    "bytes of the K listed voices over p50; the share is of the 8 TB/s HBM peak.",
    "",
    "| workload | layout | route | K | launches | p10 us | p50 us | p90 us | GB/s | of peak |",
    "|---|---|---|---|---|---|---|---|---|---|",
]
notes = []
p50 = {}
for workload, layouts in (("strings", (0, 1, 4)), ("allpass4", (0, 4))):
    V = SIZES[workload]
    make, ring_node = MAKE[workload]
    rng = np.random.default_rng(1)
    lists = {"all": np.arange(V, dtype=np.uint32), "quarter": np.sort(rng.choice(V, V // 4, replace=False)).astype(np.uint32),
             "sixteenth": np.sort(rng.choice(V, V // 16, replace=False)).astype(np.uint32)}
    d_x, d_out = noise(V), eng.alloc(4 * V * T * 64)
    graphs, fresh, routes, ks = {}, {}, {}, {}
    for layout in layouts:
        g = graphs[layout] = make(V, layout, True)
        assert g.delay_layout == layout
        print(f"{workload}, layout {layout}: compiled", file=sys.stderr, flush=True)
        g.reserve_voice_list(V)
        rotate(g, V, d_x, d_out, 7)
        indices = g.get_state(ring_node, 0)
        notes.append(f"{workload}, layout {layout}: after the rotation the write indices take {np.unique(indices).size} values over the bank; "
                     f"{int((indices.reshape(-1, 64) != indices.reshape(-1, 64)[:, :1]).any(axis=1).sum())} of {V // 64} wavefronts of the full list hold more than one.")
        for lname, L in lists.items():
            routes[(layout, f"process_listed, {lname}")] = (lambda g=g, L=L: g.set_voice_list(L), lambda g=g: g.process_listed(T, [d_x], [d_out], Layout.QUAD, Layout.QUAD))
            ks[(layout, f"process_listed, {lname}")] = L.size
        # the plain kernel twice: on this bank, whose write indices now differ by voice, and on a bank from clear - its own best case
        try:
            g.process(T, [d_x], [d_out])
            routes[(layout, "process, all voices, the rotated bank")] = (lambda: None, lambda g=g: g.process(T, [d_x], [d_out]))
        except ml.MlgpuError:   # (a PitchbendableDelay in layout 4: the plain kernel is refused after a listed launch)
            notes.append(f"{workload}, layout {layout}: `process` of the rotated bank is refused (a PitchbendableDelay in layout 4 after listed launches); no such row.")
        fresh[layout] = make(V, layout, False)
        routes[(layout, "process, all voices, a bank from clear")] = (lambda: None, lambda g=fresh[layout]: g.process(T, [d_x], [d_out]))
        ks[(layout, "process, all voices, the rotated bank")] = ks[(layout, "process, all voices, a bank from clear")] = V
    res = measure(routes)
    for (layout, route), p in res.items():
        K = ks[(layout, route)]
        gbs = BYTES_PER_VOICE_SAMPLE[workload] * K * T * 64 / (p[1] * 1e-6) / 1e9
        p50[(workload, layout, route)] = p[1]
        lines.append(f"| {workload} | {layout} | {route} | {K} | {(LAUNCHES + BLOCK - 1) // BLOCK * BLOCK} | {p[0]:.1f} | {p[1]:.1f} | {p[2]:.1f} | {gbs:.0f} | {gbs * 1e9 / HBM_PEAK:.3f} |")
    if workload == "strings":
        # the A/B of the aligned test: the same rotated bank in layout 4, the listed kernel built with the strict test
        os.environ["MLGPU_GRAPH_RING_LANE_CLOCK"] = "0"
        strict = make(V, 4, True)
        del os.environ["MLGPU_GRAPH_RING_LANE_CLOCK"]
        assert "MLGPU_RING_LANE_CLOCK" not in strict.listed_source() and "MLGPU_RING_LANE_CLOCK" in graphs[4].listed_source()
        strict.reserve_voice_list(V)
        rotate(strict, V, d_x, d_out, 7)
        ab = {}
        for lname in ("all", "quarter"):
            for label, g in (("each lane on a sector boundary", graphs[4]), ("equal write indices (strict)", strict)):
                ab[(lname, label)] = (lambda g=g, L=lists[lname]: g.set_voice_list(L), lambda g=g: g.process_listed(T, [d_x], [d_out], Layout.QUAD, Layout.QUAD))
        res = measure(ab)
        for lname in ("all", "quarter"):
            a, b = res[(lname, "each lane on a sector boundary")], res[(lname, "equal write indices (strict)")]
            notes.append(f"A/B of layout 4's aligned test, strings, rotated lists, list `{lname}`: each lane on a sector boundary {a[1]:.1f} us at p50 "
                         f"(p10 {a[0]:.1f}, p90 {a[2]:.1f}); equal write indices in the wavefront {b[1]:.1f} us (p10 {b[0]:.1f}, p90 {b[2]:.1f}): {b[1] / a[1]:.2f} x.")
        strict.close()
    for g in list(graphs.values()) + list(fresh.values()):
        g.close()
    del d_x, d_out
for workload, layouts in (("strings", (1, 4)), ("allpass4", (4,))):
    for lname in ("all", "quarter", "sixteenth"):
        base = p50[(workload, 0, f"process_listed, {lname}")]
        notes.append(f"{workload}, list `{lname}`: listed layout 0 takes " + ", ".join(f"{base / p50[(workload, lay, f'process_listed, {lname}')]:.2f} x layout {lay}'s time" for lay in layouts) + " at p50.")
lines += [""] + notes
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
eng.close()
