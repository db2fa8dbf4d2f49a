"""Voice records on the device: mlgpu_graph_export_voices / _import_voices (and the bank's) move listed voices' whole state - params,
coefficients, state words, delay rings - between objects of one signature, by one small kernel on the engine's stream.

Bits, against paths that were there before: a moved voice must go on exactly as it would have gone on where it came from. `src` (600
voices) runs 5 DSPVectors, `dst` and `twin` (80 voices, the same description and ring layout) run 2: with rings of 256 samples the
write clocks stand at 64 and 128. The voices S of src are exported and imported into the voices D of dst; then all three run 5 more
vectors (ring / 64 + 1: every ring position comes out), dst and twin reading src's input rows of S at D. dst at D must be src at S -
outputs, params, coefficients, every state word -, dst elsewhere must be twin, and src an undisturbed twin of itself.

Shapes are those of tests/test_gpu_ring_clear.py: 80 voices (a last wavefront of 16 voices: layout 2's spare lanes run voice 79 again on
rings of their own) and 600 (three 256-voice blocks, the last one partial); rings of 256 samples (max delay 100), and of 4 096 where a
voice's rings are more than one pass of the kernel's lanes; reads at the maximum delay and at short delays that differ per voice."""
import ctypes

import numpy as np
import pytest

import madronalib_amd as ml
from inputs import lcg_noise
from madronalib_amd import patches
from madronalib_amd.constants import Layout, Proc, Region, Status

LAYOUTS = [pytest.param(False, id="rows"), pytest.param(True, id="windows"), pytest.param(2, id="transposed"), pytest.param(4, id="sectors"),
           pytest.param(3, id="best")]
KINDS = {"integer": Proc.INTEGER_DELAY, "fractional": Proc.FRACTIONAL_DELAY, "pitchbendable": Proc.PITCHBENDABLE_DELAY}
V_SRC, V_DST = 600, 80
S = np.array([255, 256, 599] + [250, 251, 252, 253, 254, 257, 258, 259], np.uint32)     # {255, 256, 599, 250..259}, each once
D = np.array([79, 60, 61, 62, 63, 64, 65, 66, 67, 68, 69], np.uint32)                      # voice 79, and a run over lanes 60..69


@pytest.fixture(scope="module")
def eng():
    e = ml.Engine(0)
    yield e
    e.close()


def same(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all())


def ring_len(max_delay):
    n = 1
    while n < int(max_delay) + 64:
        n *= 2
    return n


def short_delays(V, offset=0):
    """1 .. 23 samples, different in neighbouring voices, most of them under 16 and none 0."""
    return (1 + ((np.arange(V) + offset) * 5) % 23).astype(np.float32)


def delay_signal(V, T, max_delay, mode, offset=0):
    per_voice = np.full(V, ring_len(max_delay) - 64, np.float32) if mode == "max" else short_delays(V, offset)
    return np.repeat(per_voice[:, None], 64 * T, 1)


def tables(g):
    """Every per-voice row of a graph: {("p" | "c" | "s", node, index): [V] uint32}."""
    t = {}
    for name, nid in g.ids.items():
        for i in range(max(0, g.L.mlgpu_graph_num_state(g.h, nid))):
            t[("s", name, i)] = g.get_state(name, i).view(np.uint32).copy()
        for i in range(max(0, g.L.mlgpu_graph_num_coeffs(g.h, nid))):
            t[("c", name, i)] = g.get_coeff(name, i).view(np.uint32).copy()
    for name in getattr(g, "param_names", ()):
        t[("p", name, 0)] = g.get_param(name).view(np.uint32).copy()
    return t


def run(g, T, sig, listed=False):
    """T DSPVectors of all voices through mlgpu_graph_process - or, listed, through mlgpu_graph_process_listed with every voice
    listed: VOICE_MAJOR numpy in ({name: [V][64 T]}), the list of VOICE_MAJOR outputs back."""
    if not listed:
        return g.process_host(T, sig)
    eng, V = g.engine, g.V
    d_in = [eng.to_device(np.ascontiguousarray(sig[name], np.float32)) for name in g.inputs]
    d_out = [eng.alloc(4 * V * 64 * T) for _ in g.outputs]
    g.set_voice_list(np.arange(V, dtype=np.uint32))
    g.process_listed(T, d_in, d_out, Layout.VOICE_MAJOR, Layout.VOICE_MAJOR)
    return [d.download(np.float32, V * 64 * T).reshape(V, 64 * T) for d in d_out]


# ---- the graphs: one delay node of each kind, and an allpass composite around one (a feedback node, a per-voice param) ---------------
def make_graph(eng, V, kind, max_delay, layout, mode, seed, **kw):
    """The graph with its per-voice tables set differently in every voice (and differently for another seed)."""
    if kind == "allpass":
        sub, out = patches.allpass("ap_", "x", Proc.INTEGER_DELAY, max_delay + 64.0)
        g = ml.Graph(eng, V, [dict(name="x", type="input")] + sub, [out], delay_windows=layout, **kw)
        g.param_names = ["ap_gain"]
        g.clear()
        g.set_param("ap_gain", (0.8 * np.cos(0.37 * (np.arange(V) + seed))).astype(np.float32))
        g.set_state("ap_delay", 1, np.full(V, ring_len(max_delay) - 64, np.uint32) if mode == "max" else short_delays(V, seed).astype(np.uint32))
    else:
        g = ml.Graph(eng, V, [dict(name="x", type="input"), dict(name="dt", type="input"),
                              dict(name="d", type="proc", kind=KINDS[kind], inputs=["x", "dt"], max_delay=max_delay)], ["d"], delay_windows=layout, **kw)
        g.clear()
    return g


def signals(kind, V, T, max_delay, mode, seed):
    sig = {"x": lcg_noise(np.arange(V, dtype=np.uint32) + seed, 64 * T)}
    if kind != "allpass":
        sig["dt"] = delay_signal(V, T, max_delay, mode, seed)
    return sig


def carried(sig_dst, sig_src, dst_voices, src_voices):
    """dst's input rows, with src's rows of `src_voices` at `dst_voices`."""
    out = {}
    for k, a in sig_dst.items():
        a = a.copy()
        a[dst_voices] = sig_src[k][src_voices]
        out[k] = a
    return out


def refuses_import(g, kind):
    return kind == "pitchbendable" and g.delay_layout == 4


def move_and_check(eng, kind, layout, mode, max_delay, T1_src, T1_dst, T2, S, D, listed=False, what=""):
    kw = dict(voice_list_rings=True) if listed else {}
    src, src_twin = (make_graph(eng, V_SRC, kind, max_delay, layout, mode, 1, **kw) for _ in range(2))
    dst, twin = (make_graph(eng, V_DST, kind, max_delay, layout, mode, 1000, **kw) for _ in range(2))
    assert src.voice_record_signature == dst.voice_record_signature != 0 and src.voice_record_words == dst.voice_record_words
    W = src.voice_record_words
    assert W % 4 == 0 and W >= ring_len(max_delay) * (2 if kind == "pitchbendable" else 1)
    s1, d1 = signals(kind, V_SRC, T1_src, max_delay, mode, 11), signals(kind, V_DST, T1_dst, max_delay, mode, 511)
    s2 = signals(kind, V_SRC, T2, max_delay, mode, 977)
    d2 = carried(signals(kind, V_DST, T2, max_delay, mode, 1977), s2, D, S)
    for g in (src, src_twin):
        run(g, T1_src, s1, listed)
    for g in (dst, twin):
        run(g, T1_dst, d1, listed)
    before = tables(dst)
    d_rec = src.export_voices(S)
    if refuses_import(dst, kind) and not listed:
        with pytest.raises(ml.MlgpuError) as ei:
            dst.import_voices(src.voice_record_signature, D, d_rec)
        assert ei.value.status == Status.ERR_UNSUPPORTED and "PitchbendableDelay" in str(ei.value) and "mlgpu_graph_enable_voice_list_rings" in str(ei.value)
        after = tables(dst)
        assert all(same(before[k], after[k]) for k in before), (what, "a refused import changed a table")
        yd, yt = run(dst, T2, d2), run(twin, T2, d2)
        assert all(same(a, b) for a, b in zip(yd, yt)), (what, "a refused import changed the rings")
    else:
        dst.import_voices(src.voice_record_signature, D, d_rec)
        if listed and kind == "pitchbendable" and dst.delay_layout == 4:
            with pytest.raises(ml.MlgpuError) as ei:
                run(dst, T2, d2)
            assert ei.value.status == Status.ERR_UNSUPPORTED and "after a listed launch" in str(ei.value), str(ei.value)
        ts, td = tables(src), tables(dst)
        for k in ts:
            assert same(td[k][D], ts[k][S]), (what, "right after the import", k)
        ys, yst, yd, yt = run(src, T2, s2, listed), run(src_twin, T2, s2, listed), run(dst, T2, d2, listed), run(twin, T2, d2, listed)
        rest = np.setdiff1d(np.arange(V_DST), D)
        for o in range(len(ys)):
            assert np.abs(ys[o][S]).max() > 1e-3
            bad = np.flatnonzero((yd[o][D].view(np.uint32) != ys[o][S].view(np.uint32)).any(1))
            assert bad.size == 0, (what, "output", o, "moved voices that differ from where they came from: dst", D[bad], "first sample", np.flatnonzero(yd[o][D[bad[0]]] != ys[o][S[bad[0]]])[:4])
            assert same(yd[o][rest], yt[o][rest]), (what, "output", o, "a voice that was not imported changed")
            assert same(ys[o], yst[o]), (what, "output", o, "export changed src")
            assert (yd[o][D].view(np.uint32) != yt[o][D].view(np.uint32)).any(1).all(), (what, "the import changed nothing in some voice")
        ts, tst, td, tt = tables(src), tables(src_twin), tables(dst), tables(twin)
        for k in ts:
            assert same(td[k][D], ts[k][S]), (what, "after the run", k)
            assert same(td[k][rest], tt[k][rest]) and same(ts[k], tst[k]), (what, "after the run, the others", k)
        if listed and kind == "pitchbendable" and dst.delay_layout == 4:
            # after a clear the plain call is back; an import alone takes it away again, as a listed launch does; the next clear returns it
            one = {k: a[:, :64] for k, a in d2.items()}
            dst.clear()
            run(dst, 1, one)
            dst.import_voices(src.voice_record_signature, D, d_rec)
            with pytest.raises(ml.MlgpuError) as ei:
                run(dst, 1, one)
            assert ei.value.status == Status.ERR_UNSUPPORTED and "after a listed launch" in str(ei.value), str(ei.value)
            dst.clear()
            run(dst, 1, one)
    for g in (src, src_twin, dst, twin):
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["integer", "fractional", "pitchbendable", "allpass"])
def test_moved_voices(eng, kind, layout):
    """Every kind of delay node in every ring layout, both delay modes, through the plain kernel: the imported voices stand on another
    write clock than their wavefront's. The plain sector layout with a PitchbendableDelay refuses the import and changes nothing."""
    for mode in ("max", "short"):
        move_and_check(eng, kind, layout, mode, 100.0, 5, 2, 5, S, D, what=(kind, layout, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [pytest.param(True, id="windows"), pytest.param(4, id="sectors"), pytest.param(3, id="best")])
@pytest.mark.parametrize("kind", ["fractional", "pitchbendable"])
def test_moved_voices_through_the_listed_kernels(eng, kind, layout):
    """With mlgpu_graph_enable_voice_list_rings the same move, every launch through mlgpu_graph_process_listed with every voice listed;
    a PitchbendableDelay in layout 4 takes the import, and mlgpu_graph_process then answers ERR_UNSUPPORTED until mlgpu_graph_clear."""
    move_and_check(eng, kind, layout, "short", 100.0, 5, 2, 5, S, D, listed=True, what=(kind, layout, "listed"))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["integer", "fractional", "pitchbendable", "allpass"])
def test_put_back(eng, kind, layout):
    """One graph exports S, runs 5 vectors (5 x 64 is no multiple of 256: the clocks differ afterwards), imports S back and runs the
    same 5 vectors again: S repeats its bits, the rest is a twin that ran straight through."""
    V, T, max_delay, mode = V_SRC, 5, 100.0, "short"
    g, twin = (make_graph(eng, V, kind, max_delay, layout, mode, 1) for _ in range(2))
    warm, again = signals(kind, V, T, max_delay, mode, 21), signals(kind, V, T, max_delay, mode, 1021)
    for x in (g, twin):
        run(x, T, warm)
    d_rec = g.export_voices(S)
    y1, t1 = run(g, T, again), run(twin, T, again)
    if refuses_import(g, kind):
        with pytest.raises(ml.MlgpuError) as ei:
            g.import_voices(g.voice_record_signature, S, d_rec)
        assert ei.value.status == Status.ERR_UNSUPPORTED
    else:
        g.import_voices(g.voice_record_signature, S, d_rec)
    y2, t2 = run(g, T, again), run(twin, T, again)
    rest = np.setdiff1d(np.arange(V), S)
    for o in range(len(y1)):
        assert same(y1[o], t1[o]) and np.abs(y1[o][S]).max() > 1e-3
        assert same(y2[o][rest], t2[o][rest]), (kind, layout, "the voices that were not put back")
        if refuses_import(g, kind):
            assert same(y2[o], t2[o])
        else:
            bad = np.flatnonzero((y2[o][S].view(np.uint32) != y1[o][S].view(np.uint32)).any(1))
            assert bad.size == 0, (kind, layout, "voices put back that do not repeat their bits", S[bad])
            assert (t2[o][S].view(np.uint32) != t1[o][S].view(np.uint32)).any(1).all()
    g.close()
    twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [pytest.param(False, id="rows"), pytest.param(4, id="sectors")])
def test_longer_rings_more_than_one_pass(eng, layout):
    """Rings of 4 096 samples, 64 voices moved: 16 KiB per voice, far more quads than one pass of the launch's lanes per voice."""
    s64 = np.r_[224:288].astype(np.uint32)                       # over the first 256-voice block's border
    d64 = np.r_[79, 0:63].astype(np.uint32)
    move_and_check(eng, "fractional", layout, "max", 4000.0, 4096 // 64 + 3, 2, 4096 // 64 + 1, s64, d64, what=("long", layout))


def round_lists(r):
    return (np.arange(8, dtype=np.uint32) * 70 + r).astype(np.uint32), (np.arange(8, dtype=np.uint32) * 70 + 35 + r).astype(np.uint32)


@pytest.mark.gpu
def test_stream_order_without_waits(eng):
    """Five rounds of export -> process -> import back to back with no wait in between - both staging sets are reused, the third call
    takes the first call's set - give what the same rounds give with engine.sync() after every call."""
    V, T, rounds, kind, max_delay = 600, 1, 5, "fractional", 100.0
    n = V * T * 64
    outs = {}
    for waits in (False, True):
        g = make_graph(eng, V, kind, max_delay, 4, "short", 1)
        g.reserve_voice_records(8)
        run(g, 3, signals(kind, V, 3, max_delay, "short", 5))
        quad = lambda a: np.ascontiguousarray(a.reshape(V, T * 16, 4).transpose(1, 0, 2))  # noqa: E731
        sigs = [signals(kind, V, T, max_delay, "short", 30 + r) for r in range(rounds)]
        d_in = [[eng.to_device(quad(s[name])) for name in g.inputs] for s in sigs]
        d_out = [eng.alloc(4 * n) for _ in range(rounds)]
        d_rec = [eng.alloc(4 * 8 * g.voice_record_words) for _ in range(rounds)]
        eng.sync()
        for r in range(rounds):
            a, b = round_lists(r)
            for step in (lambda: g.export_voices(a, d_rec[r]), lambda: g.process(T, d_in[r], [d_out[r]]), lambda: g.import_voices(g.voice_record_signature, b, d_rec[r])):
                step()
                if waits:
                    eng.sync()
        outs[waits] = [d.download(np.float32, n).copy() for d in d_out] + [np.concatenate(list(tables(g).values()))] + run(g, 5, signals(kind, V, 5, max_delay, "short", 77))
        g.close()
    for r, (x, y) in enumerate(zip(outs[False], outs[True])):
        assert same(x, y), r
    assert np.abs(outs[False][rounds - 1]).max() > 1e-4


@pytest.mark.gpu
def test_two_engines_of_one_device(eng):
    """Export on one engine, mlgpu_fence, import on the other: what the same move gives on one engine."""
    other = ml.Engine(0)
    kind, max_delay, T = "allpass", 100.0, 5
    results = []
    for dst_engine in (eng, other):
        src = make_graph(eng, V_SRC, kind, max_delay, 2, "short", 1)
        dst = make_graph(dst_engine, V_DST, kind, max_delay, 2, "short", 1000)
        run(src, T, signals(kind, V_SRC, T, max_delay, "short", 11))
        run(dst, 2, signals(kind, V_DST, 2, max_delay, "short", 511))
        d_rec = src.export_voices(S)
        if dst_engine is not eng:
            f = eng.fence()
            eng.signal(f)
            dst_engine.wait(f)
        dst.import_voices(src.voice_record_signature, D, d_rec)
        results.append(run(dst, T, signals(kind, V_DST, T, max_delay, "short", 1977)) + [np.concatenate(list(tables(dst).values()))])
        dst.close()
        src.close()
    other.close()
    assert all(same(a, b) for a, b in zip(*results)) and np.abs(results[0][0][D]).max() > 1e-3


def staging(obj):
    four = (ctypes.c_void_p * 4)()
    cap = getattr(obj.L, "mlgpu_%s_voice_record_staging" % obj._records_owner)(obj.h, four)
    return tuple(four), int(cap)


@pytest.mark.gpu
def test_reserve(eng):
    """After reserve_voice_records(n) the staging sets stay where they are and as large as they are, calls of up to n voices pass - the
    spare lanes of layout 2 included - and n + 1 voices are ERR_RANGE with nothing changed."""
    g, twin = (make_graph(eng, V_DST, "fractional", 100.0, 2, "short", 1) for _ in range(2))
    sig = signals("fractional", V_DST, 3, 100.0, "short", 3)
    run(g, 3, sig), run(twin, 3, sig)
    assert staging(g) == ((None, None, None, None), 0)
    g.reserve_voice_records(11)
    reserved = staging(g)
    assert all(reserved[0]) and reserved[1] >= 2 * 11
    d_rec = eng.alloc(4 * 12 * g.voice_record_words)
    for _ in range(3):                                            # both staging sets, in place
        g.export_voices(D, d_rec)
        g.import_voices(g.voice_record_signature, D, d_rec)       # (voice 79: the spare lanes' entries fit the reserve too)
        assert staging(g) == reserved
    twelve = np.arange(12, dtype=np.uint32)
    for call in (lambda: g.export_voices(twelve, d_rec), lambda: g.import_voices(g.voice_record_signature, twelve, d_rec)):
        with pytest.raises(ml.MlgpuError) as ei:
            call()
        assert ei.value.status == Status.ERR_RANGE and "12" in str(ei.value) and "11" in str(ei.value)
    assert staging(g) == reserved
    ya, yb = run(g, 5, signals("fractional", V_DST, 5, 100.0, "short", 9)), run(twin, 5, signals("fractional", V_DST, 5, 100.0, "short", 9))
    assert all(same(a, b) for a, b in zip(ya, yb))
    ta, tb = tables(g), tables(twin)
    assert all(same(ta[k], tb[k]) for k in ta)
    g.close()
    twin.close()


@pytest.mark.gpu
def test_refusals_change_nothing(eng):
    """Every refusal of the header, each leaving the tables and the rings as they were (a twin that got no call gives the same bits)."""
    kind, max_delay = "allpass", 100.0
    g, twin = (make_graph(eng, V_DST, kind, max_delay, 4, "short", 1) for _ in range(2))
    other_layout = make_graph(eng, V_DST, kind, max_delay, False, "short", 1)
    sig = signals(kind, V_DST, 3, max_delay, "short", 3)
    run(g, 3, sig), run(twin, 3, sig)
    sgn, W = g.voice_record_signature, g.voice_record_words
    assert other_layout.voice_record_signature != sgn
    d_rec = eng.alloc(4 * 16 * W)
    d_rec.upload(np.full(16 * W, 0x3F000000, np.uint32))
    voices = np.array([3, 70, 79], np.uint32)
    vp = voices.ctypes.data_as(ctypes.c_void_p)
    L, rec = g.L, ctypes.c_void_p(d_rec.ptr)

    def refused(status, text, call):
        with pytest.raises(ml.MlgpuError) as ei:
            call()
        assert ei.value.status == status and text in str(ei.value), (status, text, str(ei.value))
    # MLGPU_ERR_INVALID: null pointers, a record buffer off its alignment, a voice twice in an import, a call while recording
    assert L.mlgpu_graph_export_voices(g.h, None, 3, rec) == Status.ERR_INVALID and L.mlgpu_graph_export_voices(g.h, vp, 3, None) == Status.ERR_INVALID
    assert L.mlgpu_graph_import_voices(g.h, sgn, None, 3, rec) == Status.ERR_INVALID and L.mlgpu_graph_import_voices(g.h, sgn, vp, 3, None) == Status.ERR_INVALID
    assert L.mlgpu_graph_import_voices(g.h, sgn, vp, 3, ctypes.c_void_p(d_rec.ptr + 4)) == Status.ERR_INVALID
    refused(Status.ERR_INVALID, "twice", lambda: g.import_voices(sgn, [3, 70, 3], d_rec))
    g.export_voices([3, 70, 3], d_rec)                              # (export takes repeats)
    d_rec.upload(np.full(16 * W, 0x3F000000, np.uint32))
    for call in (lambda: g.export_voices(voices, d_rec), lambda: g.import_voices(sgn, voices, d_rec), lambda: g.reserve_voice_records(4)):
        with pytest.raises(ml.MlgpuError) as ei:
            with eng.record():
                call()
        assert ei.value.status == Status.ERR_INVALID and "recording" in str(ei.value)
    # MLGPU_ERR_RANGE: a voice >= V
    refused(Status.ERR_RANGE, "position 1", lambda: g.import_voices(sgn, [3, 80, 5], d_rec))
    refused(Status.ERR_RANGE, "80 voices", lambda: g.export_voices([3, 4, 4000000000], d_rec))
    # MLGPU_ERR_UNSUPPORTED: another signature
    refused(Status.ERR_UNSUPPORTED, "signature", lambda: g.import_voices(other_layout.voice_record_signature, voices, d_rec))
    refused(Status.ERR_UNSUPPORTED, "signature", lambda: g.import_voices(0, voices, d_rec))
    # n == 0
    assert L.mlgpu_graph_export_voices(g.h, None, 0, None) == Status.OK and L.mlgpu_graph_import_voices(g.h, sgn, None, 0, None) == Status.OK
    # MLGPU_ERR_BUSY while a compile job owns a graph; MLGPU_ERR_INVALID before it is compiled
    fresh = make_fresh(eng)
    assert L.mlgpu_graph_export_voices(fresh.h, vp, 3, rec) == Status.ERR_INVALID and fresh.voice_record_words == 0
    fresh.compile_async()
    assert L.mlgpu_graph_export_voices(fresh.h, vp, 3, rec) == ml.BUSY and L.mlgpu_graph_import_voices(fresh.h, sgn, vp, 3, rec) == ml.BUSY
    assert L.mlgpu_graph_reserve_voice_records(fresh.h, 4) == ml.BUSY and fresh.voice_record_words == 0
    while not fresh.compile_poll():
        pass
    assert fresh.voice_record_words > 0
    fresh.close()
    # a DOWNSAMPLE_2X region: neither direction
    ds = ml.Graph(eng, V_DST)
    ds.add("x", "input")
    ds.begin_region(Region.DOWNSAMPLE_2X, ["x"], ["rx"])
    ds.add("lp", "proc", Proc.ONE_POLE, ["rx"])
    ds.add_output(ds.end_region("lp", "out"))
    ds.compile()
    refused(Status.ERR_UNSUPPORTED, "DOWNSAMPLE_2X", lambda: ds.export_voices(voices, d_rec))
    refused(Status.ERR_UNSUPPORTED, "DOWNSAMPLE_2X", lambda: ds.import_voices(ds.voice_record_signature, voices, d_rec))
    ds.close()
    # nothing has changed
    ta, tb = tables(g), tables(twin)
    assert all(same(ta[k], tb[k]) for k in ta)
    sig = signals(kind, V_DST, 5, max_delay, "short", 9)
    assert all(same(a, b) for a, b in zip(run(g, 5, sig), run(twin, 5, sig)))
    for x in (g, twin, other_layout):
        x.close()


def make_fresh(eng):
    g = ml.Graph(eng, V_DST, compile_now=False)
    g.add("x", "input")
    g.add("d", "proc", Proc.INTEGER_DELAY, ["x"], max_delay=100.0)
    g.add_output("d")
    return g


# ---- banks: coefficients, state and input consts; no rings -------------------------------------------------------------------------
def make_bank(eng, which, V, seed):
    v = np.arange(V) + seed
    if which == "fused":
        b = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], V)
        assert b.fused and "cascade" not in b.kernel_name
    elif which == "cascade":
        b = eng.bank([Proc.HIPASS] * 4, V)
        assert b.fused and "cascade" in b.kernel_name
    else:
        eng.set_jit(False)
        try:
            b = eng.bank([Proc.NOISE_GEN, Proc.ONE_POLE], V)
        finally:
            eng.set_jit(True)
        assert not b.fused
    b.clear()
    if which == "fused":
        co = np.stack([ml.Bandpass.makeCoeffs(0.05 + 0.2 * ((int(x) * 7) % 31) / 31.0, 0.7) for x in v], 1)
        for i in range(3):
            b.set_coeff(1, i, np.ascontiguousarray(co[i]))
        b.set_coeff(2, 0, (0.1 + 0.4 * ((v * 13) % 17) / 17.0).astype(np.float32))
        b.set_input_const((55.0 * 2.0 ** (5.0 * ((v * 11) % 97) / 97.0) / 48000.0).astype(np.float32))
    elif which == "cascade":
        for p in range(4):
            co = np.stack([ml.Hipass.makeCoeffs(0.02 + 0.01 * p + 0.001 * ((int(x) * 5) % 19), 0.9) for x in v], 1)
            for i in range(co.shape[0]):
                b.set_coeff(p, i, np.ascontiguousarray(co[i]))
    else:
        b.set_state(0, 0, (v + 5).astype(np.uint32))
        co = np.stack([ml.OnePole.makeCoeffs(0.05 + 0.01 * ((int(x) * 3) % 23)) for x in v], 1)
        for i in range(co.shape[0]):
            b.set_coeff(1, i, np.ascontiguousarray(co[i]))
    return b


def bank_tables(b):
    t = {("c", p, i): b.get_coeff(p, i).view(np.uint32).copy() for p in range(len(b.procs)) for i in range(b.num_coeffs(p))}
    t.update({("s", p, i): b.get_state(p, i).copy() for p in range(len(b.procs)) for i in range(b.num_state(p))})
    t[("i", 0, 0)] = b.get_input_const().view(np.uint32).copy()
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fused", "cascade", "unfused"])
def test_banks(eng, which):
    """Voices moved from a bank of 2 352 into a bank of 80 and, from there, into another bank of 2 352: the moved voices go on with the
    bits of where they came from, all others with a twin's."""
    big, small = 2352, 80
    s_big = np.array([2351, 255, 256] + list(range(1024, 1032)), np.uint32)
    T1, T2 = 3, 2
    src, src_twin = (make_bank(eng, which, big, 1) for _ in range(2))
    dst, twin = (make_bank(eng, which, small, 5000) for _ in range(2))
    far, far_twin = (make_bank(eng, which, big, 9000) for _ in range(2))
    assert src.voice_record_signature == dst.voice_record_signature == far.voice_record_signature != 0
    W = src.voice_record_words
    assert W % 4 == 0 and W >= sum(src.num_coeffs(p) + src.num_state(p) for p in range(len(src.procs))) + 1
    noise = lambda V, T, seed: lcg_noise(np.arange(V, dtype=np.uint32) + seed, 64 * T) if which == "cascade" else None  # noqa: E731
    for b in (src, src_twin):
        b.process_host(T1, noise(big, T1, 7))
    for b in (dst, twin):
        b.process_host(1, noise(small, 1, 8))
    for b in (far, far_twin):
        b.process_host(2, noise(big, 2, 9))
    d_rec = src.export_voices(s_big)
    dst.import_voices(src.voice_record_signature, D, d_rec)
    d_far = dst.export_voices(D[::-1])                              # ... and on, in another order
    far.import_voices(dst.voice_record_signature, s_big[::-1] - 3 * (s_big[::-1] == 2351), d_far)
    f_big = s_big - 3 * (s_big == 2351)                             # (voice 2351 goes to 2348)
    xs = noise(big, T2, 17)
    xd, xf = noise(small, T2, 18), noise(big, T2, 19)
    if which == "cascade":
        xd[D] = xs[s_big]
        xf[f_big] = xs[s_big]
    ys, yst, yd, yt, yf, yft = (b.process_host(T2, x) for b, x in ((src, xs), (src_twin, xs), (dst, xd), (twin, xd), (far, xf), (far_twin, xf)))
    assert np.abs(ys[s_big]).max() > 1e-4 and same(ys, yst)
    for y, yy, where, V in ((yd, yt, D, small), (yf, yft, f_big, big)):
        rest = np.setdiff1d(np.arange(V), where)
        assert same(y[where], ys[s_big]) and same(y[rest], yy[rest]) and not same(y[where], yy[where]), which
    ts, tst, td, tt, tf, tft = (bank_tables(b) for b in (src, src_twin, dst, twin, far, far_twin))
    for k in ts:
        assert same(ts[k], tst[k]), k
        for t, t_twin, where, V in ((td, tt, D, small), (tf, tft, f_big, big)):
            rest = np.setdiff1d(np.arange(V), where)
            assert same(t[k][where], ts[k][s_big]) and same(t[k][rest], t_twin[k][rest]), (which, k)
    # the bank's refusals
    refusals = ((Status.ERR_RANGE, lambda: dst.import_voices(dst.voice_record_signature, [1, 80], d_rec)),
                (Status.ERR_INVALID, lambda: dst.import_voices(dst.voice_record_signature, [1, 1], d_rec)),
                (Status.ERR_UNSUPPORTED, lambda: dst.import_voices(dst.voice_record_signature ^ 1, [1, 2], d_rec)))
    for status, call in refusals:
        with pytest.raises(ml.MlgpuError) as ei:
            call()
        assert ei.value.status == status
    t_after = bank_tables(dst)
    assert all(same(td[k], t_after[k]) for k in td)
    for b in (src, src_twin, dst, twin, far, far_twin):
        b.close()
