"""Developer tool: what moving voices with their sound costs (Graph.export_voices / import_voices), beside a device-to-device copy of
the same byte count - the ceiling - and, for the table part only, the one way there was before: whole-row get_state / set_state
(get_coeff / set_coeff) of every row through the host.

The subject is the string bank at 262 144 voices: feedback -> FractionalDelay (max_delay 1024: a ring of 2 048 words) -> OnePole,
in ring layouts 0, 2 and 4. Per layout: export and import of 16 adjacent voices, of 1 024 scattered voices and of all voices - stream
events around the one call on an idle stream (the upload of the voice list and the kernel), median (min - max) of the repeats after
warm-up, and perf_counter around the host call - then the same bytes through hipMemcpyDtoDAsync, the tables' rows through the host,
and the launch time of Graph.process (1 DSPVector) before and after one voice of every wavefront has been imported from a donor graph
that stands on another write clock.

  python tools/voice_records_bench.py [repeats] [--voices V] [--md profiles/voice_records.md]"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import madronalib_amd as ml  # noqa: E402
from madronalib_amd.constants import Op, Proc  # noqa: E402


def option(name, default):
    if name in sys.argv:
        value = sys.argv[sys.argv.index(name) + 1]
        del sys.argv[sys.argv.index(name):sys.argv.index(name) + 2]
        return value
    return default


md = option("--md", None)
V = int(option("--voices", 262144))
REPEATS, WARMUP = (int(sys.argv[1]) if len(sys.argv) > 1 else 20), 3
LAYOUTS = [(0, False), (2, 2), (4, 4)]
DONOR_V = V // 64


def strings(eng, voices, layout):
    desc = [dict(name="x", type="input"), dict(name="g", type="const", value=0.995),
            dict(name="fb", type="feedback", source="damp"),
            dict(name="fbg", type="op", kind=Op.MULTIPLY, inputs=["fb", "g"]),
            dict(name="sum", type="op", kind=Op.ADD, inputs=["x", "fbg"]),
            dict(name="line", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=["sum"], max_delay=1024.0),
            dict(name="damp", type="proc", kind=Proc.ONE_POLE, inputs=["line"])]
    g = ml.Graph(eng, voices, desc, ["damp"], delay_windows=layout)
    g.clear()
    g.set_coeffs("damp", [float(c) for c in ml.OnePole.makeCoeffs(0.2)])
    st = ml.FractionalDelay.makeState(777.3)
    g.set_state("line", 3, np.full(voices, st.view(np.uint32)[0], np.uint32))
    g.set_state("line", 4, np.full(voices, st.view(np.uint32)[1], np.uint32))
    return g


def timed(eng, call, repeats=None):
    """(device us: median, min, max; host us: median) of `call` on an idle stream."""
    dev, host = [], []
    for k in range(WARMUP + (repeats or REPEATS)):
        eng.sync()
        eng.timer_start()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        ms = eng.timer_stop_ms()
        if k >= WARMUP:
            dev.append(ms * 1e3)
            host.append((t1 - t0) * 1e6)
    return float(np.median(dev)), float(np.min(dev)), float(np.max(dev)), float(np.median(host))


try:
    hip = ctypes.CDLL("libamdhip64.so")
except OSError:
    hip = ctypes.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
hip.hipMemcpyDtoDAsync.restype = ctypes.c_int
hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]

eng = ml.Engine(0)
stream = ctypes.c_void_p(eng.stream)
rng = np.random.default_rng(7)
cases = [("16 adjacent", np.arange(1000, 1016, dtype=np.uint32)), ("1 024 scattered", np.sort(rng.choice(V, min(1024, V), replace=False)).astype(np.uint32)),
         ("all %d" % V, np.arange(V, dtype=np.uint32))]
rows, process_rows, host_rows = [], [], []
x = eng.to_device(np.zeros(V * 64, np.float32))
y = eng.alloc(4 * V * 64)
for layout, arg in LAYOUTS:
    g = strings(eng, V, arg)
    W, sig = g.voice_record_words, g.voice_record_signature
    g.reserve_voice_records(V)
    d_rec = eng.alloc(4 * V * W)
    d_copy = eng.alloc(4 * V * W)
    vectors = 0

    def process():
        global vectors
        g.process(1, [x], [y])
        vectors += 1
    before = timed(eng, process)
    for name, voices in cases:
        n, few = voices.size, (5 if voices.size == V else None)
        nbytes = 4 * n * W

        def copy():
            assert hip.hipMemcpyDtoDAsync(ctypes.c_void_p(d_copy.ptr), ctypes.c_void_p(d_rec.ptr), nbytes, stream) == 0
        ex = timed(eng, lambda: g.export_voices(voices, d_rec), few)
        im = timed(eng, lambda: g.import_voices(sig, voices, d_rec), few)
        cp = timed(eng, copy, few)
        rows.append((layout, name, n, nbytes, ex, im, cp))
        print("layout %d, %s voices (%d records of %d words, %.1f KiB): export %.1f us (%.1f - %.1f), host %.1f | import %.1f us (%.1f - %.1f), host %.1f | DtoD copy %.1f us"
              % (layout, name, n, W, nbytes / 1024, ex[0], ex[1], ex[2], ex[3], im[0], im[1], im[2], im[3], cp[0]), flush=True)
    # the table part the only way there was before: every state and coefficient row of all voices through the host, which waits
    state = [(name, i) for name, nid in g.ids.items() for i in range(max(0, g.L.mlgpu_graph_num_state(g.h, nid)))]
    coeff = [(name, i) for name, nid in g.ids.items() for i in range(max(0, g.L.mlgpu_graph_num_coeffs(g.h, nid)))]
    t_get, t_set = [], []
    for _ in range(3):
        eng.sync()
        t0 = time.perf_counter()
        got_s = [g.get_state(*k) for k in state]
        got_c = [g.get_coeff(*k) for k in coeff]
        t1 = time.perf_counter()
        for k, a in zip(state, got_s):
            g.set_state(k[0], k[1], a)
        for k, a in zip(coeff, got_c):
            g.set_coeff(k[0], k[1], a)
        eng.sync()
        t2 = time.perf_counter()
        t_get.append((t1 - t0) * 1e6)
        t_set.append((t2 - t1) * 1e6)
    host_rows.append((layout, len(state) + len(coeff), float(np.median(t_get)), float(np.median(t_set))))
    print("layout %d: %d table rows of all voices through the host: get %.0f us, set %.0f us" % (layout, len(state) + len(coeff), host_rows[-1][2], host_rows[-1][3]), flush=True)
    # one voice of every wavefront from a donor on another write clock
    donor = strings(eng, DONOR_V, arg)
    xd, yd = eng.to_device(np.zeros(DONOR_V * 64, np.float32)), eng.alloc(4 * DONOR_V * 64)
    ahead = 5 + (1 if (vectors - 5) % 32 == 0 else 0)
    for _ in range(ahead):
        donor.process(1, [xd], [yd])
    assert donor.voice_record_signature == sig and (vectors - ahead) % 32 != 0
    d_donor = donor.export_voices(np.arange(DONOR_V, dtype=np.uint32))
    g.import_voices(sig, (np.arange(DONOR_V, dtype=np.uint32) * 64 + 7).astype(np.uint32), d_donor)
    after = timed(eng, process)
    process_rows.append((layout, before, after))
    print("layout %d: process (1 DSPVector, %d voices) %.1f us before, %.1f us after one voice per wavefront was imported on another clock" % (layout, V, before[0], after[0]), flush=True)
    for b in (d_rec, d_copy, d_donor, xd, yd):
        b.free()
    donor.close()
    g.close()

if md:
    name = eng.device_info()["name"].strip().strip("()")
    with open(md, "w") as f:
        f.write(f"# Voice records: export and import of voices with their delay rings ({name})\n\n"
                f"`tools/voice_records_bench.py {REPEATS}`{'' if V == 262144 else ' --voices %d' % V}: the string bank (feedback -> FractionalDelay, max_delay 1024: a ring of 2 048 words -> OnePole) at\n"
                f"{V} voices; a record is {W} words ({4 * W} bytes). Every figure below was taken on the device named above. Device: stream events around the\n"
                f"one call on an idle stream (the voice list's upload and `voice_records_kernel`), median (min - max) of {REPEATS} after {WARMUP} (of 5 for all voices).\n"
                "Host: `perf_counter` around the call, median. The copy is `hipMemcpyDtoDAsync` of the records' byte count, timed the same way: the ceiling.\n\n"
                "| layout | voices | bytes | export device (us) | export host (us) | import device (us) | import host (us) | DtoD copy (us) | export / copy | import / copy |\n"
                "|---:|---|---:|---:|---:|---:|---:|---:|---:|---:|\n")
        for layout, cname, n, nbytes, ex, im, cp in rows:
            f.write(f"| {layout} | {cname} | {nbytes} | {ex[0]:.1f} ({ex[1]:.1f} - {ex[2]:.1f}) | {ex[3]:.1f} | {im[0]:.1f} ({im[1]:.1f} - {im[2]:.1f}) | {im[3]:.1f} | {cp[0]:.1f} | "
                    f"{ex[0] / cp[0]:.2f} | {im[0] / cp[0]:.2f} |\n")
        big = [r for r in rows if r[2] == V]
        f.write("\nAll voices, as bytes moved (read + written) per second: " +
                "; ".join(f"layout {r[0]}: export {2 * r[3] / r[4][0] / 1e6:.2f} TB/s, import {2 * r[3] / r[5][0] / 1e6:.2f} TB/s, copy {2 * r[3] / r[6][0] / 1e6:.2f} TB/s" for r in big) + ".\n"
                "In layout 0 a voice's ring words lie one ring row (4 x voices bytes) apart: a single voice is a sector per word by the layout's nature, and only\n"
                "neighbouring listed voices share sectors. Up to a few MiB a call is bound by the upload of its voice list and the launch, not by the bytes.\n\n"
                "## The table part the only way there was before\n\n"
                "Every state and coefficient row of ALL voices through the host (`get_state` / `get_coeff`, then `set_state` / `set_coeff`: each call waits for the device),\n"
                "wall time, median of 3. It moves no ring word.\n\n| layout | rows | get (us) | set (us) |\n|---:|---:|---:|---:|\n")
        for layout, nrows, tg, ts in host_rows:
            f.write(f"| {layout} | {nrows} | {tg:.0f} | {ts:.0f} |\n")
        f.write("\n## The plain kernel after an import on another write clock\n\n"
                f"`Graph.process` of 1 DSPVector, device time, median (min - max) of {REPEATS}: before any import, and after one voice of every wavefront (voice 64 i + 7) was\n"
                "imported from a donor graph whose write index stands elsewhere. Layouts 2 and 4 run their windows / trips on a write index that is the same in\n"
                "every lane of a wavefront; a wavefront whose lanes differ takes the per-sample path: the same samples, more slowly, until `mlgpu_graph_clear`. In layout 0\n"
                "the lanes of a wavefront read and write one ring row while their write indices agree; an imported voice's words lie in rows of their own, a sector more\n"
                "per access. Rotating a record's rings to the destination's clock at import would remove the cost; it is not done.\n\n"
                "| layout | before (us) | after (us) | after / before |\n|---:|---:|---:|---:|\n")
        for layout, b, a in process_rows:
            f.write(f"| {layout} | {b[0]:.1f} ({b[1]:.1f} - {b[2]:.1f}) | {a[0]:.1f} ({a[1]:.1f} - {a[2]:.1f}) | {a[0] / b[0]:.2f} |\n")
eng.close()
