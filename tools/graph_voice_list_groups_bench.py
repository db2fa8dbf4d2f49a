"""Developer tool: what a graph's listed group sum costs. The config-5 synth voice (patches.synth16) with its output summed by 16, a
graph of V voices of which K = V / 8 are listed, in one process:
  (a)  Graph.process_listed_groups, two voices listed in every instrument (segments of 2: J = V / 16 rows),
  (a') Graph.process_listed_groups, every voice of every eighth instrument listed (segments of 16: J = V / 128 rows),
  (b), (b') Graph.process_listed of the same two lists on the same graph without the sum (K rows),
  (c)  Graph.process of the full graph with the group sum (V / 16 rows) - what a caller pays without a list.
The routes alternate every 25 launches; device time per launch from events on the engine's stream (Engine.lap_times_ms), p10 / p50 /
p90. Checks first that the rows of (a) and (a') are (b)'s and (b')'s rows added up per instrument in float32, bit for bit (numpy's
float32 add is IEEE; the engine is in its default mode and this voice's output is clamped to [-1, 1], far from the denormals).

`--resources` (no device): the compiler's numbers for the lane-plan form of this voice's listed kernel.

  python tools/graph_voice_list_groups_bench.py [voices] [vectors] [launches per route] [--md profiles/graph_voice_list_groups.md]
  python tools/graph_voice_list_groups_bench.py --resources [voices]"""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd import patches  # noqa: E402
from madronalib_amd.constants import Layout  # noqa: E402
from madronalib_amd.sharding import cfg5_gate_quad, cfg5_voice_params  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else None
if md:
    args.remove(md)
V, T, LAUNCHES = (int(args[0]) if args else 262144), (int(args[1]) if len(args) > 1 else 16), (int(args[2]) if len(args) > 2 else 300)
G, K, BLOCK, WARMUP = 16, V // 8, 25, 25
desc, outs = patches.synth16()


def resources(n_voices):
    """The lane-plan listed kernel of the voice, compiled without a device: its metadata note's numbers."""
    g = ml.Graph(ml.OfflineEngine(), n_voices, desc, outs, compile_now=False, voice_list_groups=True, output_groups={0: G})
    _, code = g.emit_listed()
    g.close()
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
    keys = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")
    n = {k: int(re.search(r"\.%s:\s+(\d+)" % k, notes).group(1)) for k in keys}
    # a SIMD has 512 VGPRs per lane, handed out in blocks of 8, and eight wavefront slots; a workgroup here is one wavefront per SIMD
    n["waves_per_simd"] = min(8, 512 // max(8, (n["vgpr_count"] + n["agpr_count"] + 7) & ~7))
    n["workgroups_per_cu_by_lds"] = (160 * 1024) // max(1, n["group_segment_fixed_size"])
    return n


def resource_lines(n_voices):
    n = resources(n_voices)
    return [f"`mlgpu_graph_listed_kernel` of this voice by the lane plan, V = {n_voices}, from the code object's metadata note: {n['vgpr_count']} VGPRs "
            f"(+ {n['agpr_count']} AGPRs), {n['sgpr_count']} SGPRs ({n['sgpr_spill_count']} spilled to VGPR lanes), {n['vgpr_spill_count']} VGPRs spilled, "
            f"{n['private_segment_fixed_size']} bytes of scratch per lane, {n['group_segment_fixed_size']} bytes of LDS per workgroup (the segment strips: "
            f"4 x 4 KiB + 256 B): {n['waves_per_simd']} wavefronts per SIMD by registers, {n['workgroups_per_cu_by_lds']} workgroups per CU by LDS."]


if "--resources" in sys.argv:
    print("\n".join(resource_lines(V)))
    sys.exit(0)

eng = ml.Engine(0)
params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)
gate = cfg5_gate_quad(0, V, T)   # QUAD: [16 T][V][4]


def graph_of(**kw):
    g = ml.Graph(eng, V, desc, outs, **kw)
    g.clear()
    for k, v in params.items():
        g.set_param(k, v if np.ndim(v) else float(v))
    for k, c in coeffs.items():
        g.set_coeffs(k, list(c))
    g.set_state("noise", 0, seeds)
    return g


inst = np.arange(V // G, dtype=np.int64)
lists = {"two voices in every instrument": np.sort(np.concatenate([inst * G + 3, inst * G + 11])).astype(np.uint32),
         "every voice of every eighth instrument": (inst[::8, None] * G + np.arange(G)[None, :]).reshape(-1).astype(np.uint32)}
assert all(L.size == K for L in lists.values())
summed, listed = graph_of(voice_list_groups=True, output_groups={0: G}), graph_of(voice_lists=True)   # (both from clear)
summed.reserve_voice_list_groups(K)
listed.reserve_voice_list(K)
d_gate = eng.to_device(gate)
d_full, d_rows, d_listed, d_peak = eng.alloc(4 * (V // G) * T * 64), eng.alloc(4 * (V // G) * T * 64), eng.alloc(4 * K * T * 64), eng.alloc(4 * K)
name = eng.device_info()["name"]
lines = [
    "# What a graph's listed group sum costs",
    "",
    f"`python tools/graph_voice_list_groups_bench.py {V} {T} {LAUNCHES}` on {name}: the config-5 synth voice (`patches.synth16`) with its output "
    f"summed by {G}, a graph of V = {V} voices, K = V / 8 = {K} of them listed, {T} DSPVectors per launch, QUAD in and out. (a) / (a') "
    "`Graph.process_listed_groups` with peaks, (b) / (b') `Graph.process_listed` with peaks of the same list on the same graph without the sum, "
    f"(c) `Graph.process` of the full graph with the group sum. One process, the routes alternating every {BLOCK} launches after {WARMUP} warm-up "
    "launches of each; device time per launch between events on the engine's stream. The rows of (a) and (a') were compared first with "
    "(b)'s and (b')'s rows added up per instrument: the same bits.",
    "",
    "| list | route | rows out | launches | p10 us | p50 us | p90 us |",
    "|---|---|---|---|---|---|---|",
]
ratios = []


def routes_of(L, J):
    return {"process_listed_groups, K of V": (J, lambda: summed.process_listed_groups(T, [d_gate], [d_rows], Layout.QUAD, Layout.QUAD, d_peak=d_peak)),
            "process_listed, K of V, no sum": (K, lambda: listed.process_listed(T, [d_gate], [d_listed], Layout.QUAD, Layout.QUAD, d_peak=d_peak)),
            "process, V voices, group sum": (V // G, lambda: summed.process(T, [d_gate], [d_full]))}


# the same bits, before anything else runs: the two graphs have the same state as long as they run the same voices, so one launch of
# each per list, and (b)'s rows added per instrument in list order from +0.0
for label, L in lists.items():
    J = np.unique(L // G).size
    summed.set_voice_list(L)
    listed.set_voice_list(L)
    assert summed.listed_groups.size == J
    routes = routes_of(L, J)
    routes["process_listed_groups, K of V"][1]()
    routes["process_listed, K of V, no sum"][1]()
    d_vm = eng.alloc(4 * K * T * 64)
    eng.layout_convert(d_listed, Layout.QUAD, d_vm, Layout.VOICE_MAJOR, K, T)
    y = d_vm.download(np.float32, K * T * 64).reshape(K, T * 64)
    d_vm = eng.alloc(4 * J * T * 64)
    eng.layout_convert(d_rows, Layout.QUAD, d_vm, Layout.VOICE_MAJOR, J, T)
    rows = d_vm.download(np.float32, J * T * 64).reshape(J, T * 64)
    seg = y.reshape(J, K // J, T * 64)   # (both lists: every listed instrument has K / J listed voices)
    acc = np.zeros((J, T * 64), np.float32)
    for r in range(K // J):
        acc = acc + seg[:, r]
    differ = int((acc.view(np.uint32) != rows.view(np.uint32)).sum())
    assert differ == 0 and np.abs(rows).max() > 1e-3, f"{label}: the rows differ from process_listed's rows added up in {differ} words"
for label, L in lists.items():
    J = np.unique(L // G).size
    summed.set_voice_list(L)
    listed.set_voice_list(L)
    routes = routes_of(L, J)
    for _ in range(WARMUP):
        for _, work in routes.values():
            work()
    eng.sync()
    times = {k: [] for k in routes}
    for _ in range((LAUNCHES + BLOCK - 1) // BLOCK):
        for k, (_, work) in routes.items():
            times[k].append(eng.lap_times_ms(work, BLOCK))
    pct = {k: np.percentile(np.concatenate(v) * 1000.0, [10, 50, 90]) for k, v in times.items()}
    for k, (r, _) in routes.items():
        lines.append(f"| {label} | {k} | {r} | {np.concatenate(times[k]).size} | {pct[k][0]:.1f} | {pct[k][1]:.1f} | {pct[k][2]:.1f} |")
    a, b, c = (pct[k][1] for k in routes)
    spread = ", ".join(f"{k.split(',')[0]} p10-p90 {pct[k][0]:.0f}-{pct[k][2]:.0f} us" for k in routes)
    ratios.append(f"{label} (segments of {K // J}): groups / listed = {a / b:.2f}, groups / full = {a / c:.3f} at p50 (K/V = {K / V:.3f}); {spread}.")
summed.close()
listed.close()
lines += [""] + ratios + ["", "## The compiler's numbers", ""] + resource_lines(V)
print("\n".join(lines))
if md:
    with open(md, "w") as f:
        f.write("\n".join(lines) + "\n")
eng.close()
