"""MLGPU_UPDATE_CLEAR_RINGS: T::clear() of some voices of a delay node, its rings included, as a record of apply_updates.

Bits, and a yardstick made of paths that were there before the target: three identical graphs run on identical noise until every
ring position holds a sample; `cleared` gets the record on the voice set S, `undisturbed` gets nothing, `other` gets
mlgpu_graph_clear_proc of the same node (mlgpu_graph_clear for node = -1), which zeroes the node's rings for every voice; then
all three run on. On S `cleared` must be `other` - outputs and every state word -, everywhere else `undisturbed`. One run reads
at the maximum delay (ring length - 64: every ring position comes out within ring length / 64 + 1 vectors), one at short delays
that differ per voice (1 .. 23 samples: what lies just behind the writer, and the short-delay path of layout 4).

Shapes: 80 voices (a last wavefront of 16 voices: layout 2's spare lanes run voice 79 again on rings of their own) and 600 (three
256-voice blocks, the last one partial) with voice sets at the blocks' borders; rings of 256 samples (max delay 100), and of 4 096
where a record is more than one slab of the kernel's work split."""
import numpy as np
import pytest

import madronalib_amd as ml
from inputs import lcg_noise
from madronalib_amd import patches
from madronalib_amd.constants import Op, Proc, Region, Status

LAYOUTS = [pytest.param(False, id="rows"), pytest.param(True, id="windows"), pytest.param(2, id="transposed"), pytest.param(4, id="sectors"),
           pytest.param(3, id="best")]
SETS = {80: [(79, 1), (60, 10), (70, 10)], 600: [(255, 1), (256, 1), (250, 270), (599, 1)]}


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


def state_rows(g):
    return [(name, i) for name, nid in g.ids.items() for i in range(max(0, g.L.mlgpu_graph_num_state(g.h, nid)))]


def read_state(g, rows):
    return {k: g.get_state(*k).view(np.uint32).copy() for k in rows}


def short_delays(V):
    """1 .. 23 samples, different in neighbouring voices, most of them under 16 and none 0 (a delay of 0 reads only what the same
    vector wrote: nothing a clear could change)."""
    return (1 + (np.arange(V) * 5) % 23).astype(np.float32)


def delay_signal(V, T, max_delay, mode):
    per_voice = np.full(V, ring_len(max_delay) - 64, np.float32) if mode == "max" else short_delays(V)
    return np.repeat(per_voice[:, None], 64 * T, 1)


def clear_like_before(g, node):
    if node is None:
        g.clear()
    else:
        g.engine._check(g.L.mlgpu_graph_clear_proc(g.h, g.ids[node]))


def three_graphs(build, sig1, sig2, T1, T2, node, ranges, what):
    """The yardstick of the module's docstring for one voice set: `ranges` [(first, n)] become one CLEAR_RINGS record each
    (node: a name, or None for -1). Returns `cleared` and its state rows for the caller's own questions; the others are closed."""
    cleared, undisturbed, other = build(), build(), build()
    V = cleared.V
    S = np.zeros(V, bool)
    for first, n in ranges:
        S[first:first + n] = True
    rows = state_rows(cleared)
    y1 = [g.process_host(T1, sig1) for g in (cleared, undisturbed, other)]
    assert all(same(a, b) and same(a, c) for a, b, c in zip(*y1)), what
    assert (np.abs(y1[0][0][S]).max(1) > 0).all(), (what, "phase 1 is silent on S")
    cleared.apply_updates([ml.Update.clear_rings(-1 if node is None else cleared.ids[node], first, n) for first, n in ranges])
    clear_like_before(other, node)
    yc, yu, yo = (g.process_host(T2, sig2) for g in (cleared, undisturbed, other))
    for o, (c, u, k) in enumerate(zip(yc, yu, yo)):
        bad = np.flatnonzero((c.view(np.uint32) != np.where(S[:, None], k.view(np.uint32), u.view(np.uint32))).any(1))
        assert bad.size == 0, (what, "output", o, "voices", bad[:8], "in S" if S[bad[0]] else "outside S")
    # not vacuous: the clear changed what every voice of S gives
    changed = np.zeros(V, bool)
    for c, u in zip(yc, yu):
        changed |= (c.view(np.uint32) != u.view(np.uint32)).any(1)
    assert changed[S].all() and not changed[~S].any(), (what, "voices of S the clear did not change", np.flatnonzero(S & ~changed)[:8])
    sc, su, so = read_state(cleared, rows), read_state(undisturbed, rows), read_state(other, rows)
    for k in rows:
        assert same(sc[k][S], so[k][S]) and same(sc[k][~S], su[k][~S]), (what, "state", k)
    undisturbed.close()
    other.close()
    return cleared, rows


# ---- one delay node of each kind, and an allpass composite around one -------------------------------------------------------------
KINDS = {"integer": Proc.INTEGER_DELAY, "fractional": Proc.FRACTIONAL_DELAY, "pitchbendable": Proc.PITCHBENDABLE_DELAY}


def build_single(eng, V, kind, max_delay, layout):
    def build():
        g = ml.Graph(eng, V, [dict(name="x", type="input"), dict(name="dt", type="input"),
                              dict(name="d", type="proc", kind=kind, inputs=["x", "dt"], max_delay=max_delay)], ["d"], delay_windows=layout)
        g.clear()
        return g
    return build


def build_allpass(eng, V, layout, mode):
    """Allpass<IntegerDelay> (patches.allpass, the description tests/test_gpu_delays.py checks against the reference class): the
    delay time is the inner delay's state word 1, a feedback node holds the delay's last vector."""
    sub, out = patches.allpass("ap_", "x", Proc.INTEGER_DELAY, 164.0)     # the inner delay: max delay 100, a ring of 256
    delays = np.full(V, 192, np.uint32) if mode == "max" else short_delays(V).astype(np.uint32)

    def build():
        g = ml.Graph(eng, V, [dict(name="x", type="input")] + sub, [out], delay_windows=layout)
        g.clear()
        g.set_param("ap_gain", np.linspace(-0.8, 0.8, V).astype(np.float32))
        g.set_state("ap_delay", 1, delays)
        return g
    return build


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", ["integer", "fractional", "pitchbendable", "allpass"])
def test_clear_rings_of_some_voices(eng, kind, layout):
    """Every kind of delay node in every ring layout, 80 and 600 voices, the voice sets of SETS, both delay modes. FractionalDelay's
    and PitchbendableDelay's allpass words are cleared with the rings (the state comparison); the write indices are not."""
    max_delay, T = 100.0, 256 // 64 + 1
    for V, sets in SETS.items():
        x1, x2 = lcg_noise(np.arange(V, dtype=np.uint32) + 11, 64 * T), lcg_noise(np.arange(V, dtype=np.uint32) + 977, 64 * T)
        for mode in ("max", "short"):
            if kind == "allpass":
                build, node, sig1, sig2 = build_allpass(eng, V, layout, mode), "ap_delay", {"x": x1}, {"x": x2}
            else:
                dt = delay_signal(V, T, max_delay, mode)
                build, node, sig1, sig2 = build_single(eng, V, KINDS[kind], max_delay, layout), "d", {"x": x1, "dt": dt}, {"x": x2, "dt": dt}
            for first, n in sets:
                g, rows = three_graphs(build, sig1, sig2, T, T, node, [(first, n)], (kind, layout, V, mode, first, n))
                w = g.get_state(node, 0)
                assert (w == w[0]).all() and w[0] == (2 * T * 64) % 256, "the write index stays, and stays the same in every voice"
                g.close()


# ---- two delay nodes of different ring lengths, a feedback node and a Lopass ------------------------------------------------------
def two_delay_desc():
    return [dict(name="x", type="input"), dict(name="dt1", type="input"), dict(name="dt2", type="input"), dict(name="g", type="param"),
            dict(name="fb", type="feedback", source="mix"), dict(name="fbs", type="op", kind=Op.MULTIPLY, inputs=["fb", "g"]),
            dict(name="sum", type="op", kind=Op.ADD, inputs=["x", "fbs"]),
            dict(name="d1", type="proc", kind=Proc.INTEGER_DELAY, inputs=["sum", "dt1"], max_delay=100.0),       # a ring of 256
            dict(name="lp", type="proc", kind=Proc.LOPASS, inputs=["d1"]),
            dict(name="d2", type="proc", kind=Proc.FRACTIONAL_DELAY, inputs=["lp", "dt2"], max_delay=400.0),     # a ring of 512
            dict(name="mix", type="op", kind=Op.ADD, inputs=["d1", "d2"])]


def build_two(eng, V, layout):
    def build():
        g = ml.Graph(eng, V, two_delay_desc(), ["mix", "d2"], delay_windows=layout)
        g.clear()
        g.set_param("g", 0.3)
        g.set_coeffs("lp", [float(c) for c in ml.Lopass.makeCoeffs(0.15, 0.8)])
        return g
    return build


def two_signals(V, T, mode, seed):
    sig = {"x": lcg_noise(np.arange(V, dtype=np.uint32) + seed, 64 * T), "dt1": delay_signal(V, T, 100.0, mode), "dt2": delay_signal(V, T, 400.0, mode)}
    return sig


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_delay_nodes_one_and_all(eng, layout):
    """One of two delay nodes: the other node's rings keep every voice's samples (`other` clears that one node too, and on S the
    two must agree). Then node = -1: both delays, the feedback node's vector and the Lopass, against mlgpu_graph_clear."""
    V, T = 600, 512 // 64 + 1
    for mode in ("max", "short"):
        sig1, sig2 = two_signals(V, T, mode, 21), two_signals(V, T, mode, 1021)
        for node in ("d1", "d2", None):
            g, rows = three_graphs(build_two(eng, V, layout), sig1, sig2, T, T, node, [(250, 270)], (layout, mode, node))
            assert g.update_device_records([ml.Update.clear_rings(-1, 250, 270)]) > 64
            g.close()
    if layout == 2:   # the spare lanes, with a second node beside the cleared one
        sig1, sig2 = two_signals(80, T, "max", 31), two_signals(80, T, "max", 1031)
        g, _ = three_graphs(build_two(eng, 80, layout), sig1, sig2, T, T, "d2", [(79, 1)], "spare lanes, d2")
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [pytest.param(False, id="rows"), pytest.param(4, id="sectors")])
def test_longer_ring_more_than_one_slab(eng, layout):
    """A ring of 4 096 samples: 16 KiB per voice, and the 270 voices' records are cut into many slabs."""
    V, max_delay = 600, 4000.0
    T = 4096 // 64 + 1
    x1, x2 = lcg_noise(np.arange(V, dtype=np.uint32) + 5, 64 * T), lcg_noise(np.arange(V, dtype=np.uint32) + 1005, 64 * T)
    for mode in ("max", "short"):
        dt = delay_signal(V, T, max_delay, mode)
        g, _ = three_graphs(build_single(eng, V, Proc.INTEGER_DELAY, max_delay, layout), {"x": x1, "dt": dt}, {"x": x2, "dt": dt}, T, T, "d", [(250, 270)],
                            (layout, mode))
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [pytest.param(False, id="rows"), pytest.param(True, id="windows")])
def test_delay_line_inside_a_rate_region(eng, layout):
    """fn = Allpass<IntegerDelay> at twice the rate (an UPSAMPLE_2X region): its ring and its feedback vector live at fn's rate."""
    V, T = 80, 3      # (six vectors at fn's rate)

    def build():
        g = ml.Graph(eng, V, delay_windows=layout)
        g.add("x", "input")
        g.begin_region(Region.UPSAMPLE_2X, ["x"], ["rx"])
        sub, y = patches.allpass("ap_", "rx", Proc.INTEGER_DELAY, 164.0)
        for n in sub:
            g.add(**{k: v for k, v in n.items() if k != "source"})
        for n in sub:
            if n["type"] == "feedback":
                g.set_feedback(n["name"], n["source"])
        out = g.end_region(y, "out")
        g.add_output(out)
        g.compile()
        g.clear()
        g.set_param("ap_gain", 0.6)
        g.set_state("ap_delay", 1, delays)
        return g
    x1, x2 = lcg_noise(np.arange(V, dtype=np.uint32) + 3, 64 * T), lcg_noise(np.arange(V, dtype=np.uint32) + 1003, 64 * T)
    for mode in ("max", "short"):
        delays = np.full(V, 192, np.uint32) if mode == "max" else short_delays(V).astype(np.uint32)
        for first, n in SETS[80]:
            g, _ = three_graphs(build, {"x": x1}, {"x": x2}, T, T, "ap_delay", [(first, n)], (layout, mode, first, n))
            g.close()


# ---- the rules of the update lists ------------------------------------------------------------------------------------------------
def all_tables(g):
    t = read_state(g, state_rows(g))
    t[("param", "g")] = g.get_param("g").view(np.uint32).copy()
    for i in range(3):
        t[("coeff", "lp", i)] = g.get_coeff("lp", i).view(np.uint32).copy()
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [pytest.param(False, id="rows"), pytest.param(2, id="transposed"), pytest.param(4, id="sectors")])
def test_mixed_list_is_the_records_one_call_at_a_time(eng, layout):
    """PARAM and STATE records over each other, two CLEAR_RINGS records over each other and over the STATE records' words, in one
    list: what the same records give applied one call at a time, in list order."""
    V, T = 600, 512 // 64 + 1
    build = build_two(eng, V, layout)
    one_list, one_by_one = build(), build()
    ids = one_list.ids
    recs = [ml.Update.param(ids["g"], 200, 200, 0.2), ml.Update.state(ids["d2"], 1, 240, 40, 0x3DCCCCCD), ml.Update.clear_rings(ids["d2"], 250, 20),
            ml.Update.param(ids["g"], 255, 3, 0.25), ml.Update.state(ids["d2"], 1, 260, 5, 0x3E000000), ml.Update.clear_rings(-1, 255, 258),
            ml.Update.state(ids["lp"], 0, 500, 30, 0x3C000000), ml.Update.state(ids["fb"], 63, 0, V, 0x3B000000)]
    sig1, sig2 = two_signals(V, T, "max", 41), two_signals(V, T, "short", 1041)
    y1 = [g.process_host(T, sig1) for g in (one_list, one_by_one)]
    before = all_tables(one_list)
    one_list.apply_updates(recs)
    for r in recs:
        one_by_one.apply_updates([r])
    ta, tb = all_tables(one_list), all_tables(one_by_one)
    for k in ta:
        assert same(ta[k], tb[k]), ("tables", k)
    assert not same(ta[("d2", 1)], before[("d2", 1)]) and ta[("d2", 1)][262] == 0 and ta[("d2", 1)][245] == 0x3DCCCCCD and ta[("d2", 1)][252] == 0
    ya, yb = one_list.process_host(T, sig2), one_by_one.process_host(T, sig2)
    assert all(same(a, b) for a, b in zip(ya, yb)) and all(same(a, b) for a, b in zip(*y1))
    ta, tb = all_tables(one_list), all_tables(one_by_one)
    for k in ta:
        assert same(ta[k], tb[k]), ("tables after the run", k)
    one_list.close()
    one_by_one.close()


def staging(g):
    import ctypes
    fn = g.L.mlgpu_graph_update_staging
    fn.restype, fn.argtypes = ctypes.c_size_t, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    four = (ctypes.c_void_p * 4)()
    cap = fn(g.h, four)
    return tuple(four), int(cap)


@pytest.mark.gpu
@pytest.mark.parametrize("layout,segments", [pytest.param(False, 1, id="rows"), pytest.param(4, 3, id="sectors"), pytest.param(2, 3, id="transposed")])
def test_reserve_counts_ring_records(eng, layout, segments):
    """What a CLEAR_RINGS record costs: the state words clear() resets (IntegerDelay none, FractionalDelay two, the feedback node 64,
    the Lopass two) plus two per ring node and segment - one segment in layout 0, one per 256-voice block touched otherwise.
    After reserve_updates(n) a list of n + 1 is ERR_RANGE and nothing changes, rings included; a list of n passes in place."""
    V, T = 600, 512 // 64 + 1
    build = build_two(eng, V, layout)
    g, twin = build(), build()
    ids = g.ids
    assert g.update_device_records([ml.Update.clear_rings(ids["d1"], 250, 270)]) == 0 + 2 * segments
    assert g.update_device_records([ml.Update.clear_rings(ids["d1"], 300, 1)]) == 2
    assert g.update_device_records([ml.Update.clear_rings(ids["d2"], 250, 270)]) == 2 + 2 * segments
    assert g.update_device_records([ml.Update.clear_rings(ids["lp"], 250, 270)]) == g.update_device_records([ml.Update.clear(ids["lp"], 250, 270)]) == 2
    assert g.update_device_records([ml.Update.clear_rings(-1, 250, 270)]) == 64 + 2 + 2 + 2 * 2 * segments
    assert g.update_device_records([ml.Update.clear(ids["d1"], 0, 1)]) == 0          # (refused)
    n = 2 + 2 * segments + 1
    g.reserve_updates(n)
    reserved = staging(g)
    assert all(reserved[0]) and reserved[1] == n
    sig1, sig2 = two_signals(V, T, "max", 51), two_signals(V, T, "max", 1051)
    g.process_host(T, sig1), twin.process_host(T, sig1)
    before = all_tables(g)
    too_many = [ml.Update.clear_rings(ids["d2"], 250, 270), ml.Update.param(ids["g"], 0, 1, 0.5), ml.Update.param(ids["g"], 1, 1, 0.5)]
    assert g.update_device_records(too_many) == n + 1
    with pytest.raises(ml.MlgpuError) as ei:
        g.apply_updates(too_many)
    assert ei.value.status == Status.ERR_RANGE and str(n + 1) in str(ei.value)
    after = all_tables(g)
    for k in before:
        assert same(before[k], after[k]), k
    ya, yb = g.process_host(T, sig2), twin.process_host(T, sig2)      # ... and the rings hold what the twin's hold
    assert all(same(a, b) for a, b in zip(ya, yb)) and staging(g) == reserved
    fits = too_many[:2]
    assert g.update_device_records(fits) == n
    for _ in range(3):                                                 # both staging sets, in place
        g.apply_updates(fits)
        assert staging(g) == reserved
    assert g.get_param("g")[0] == 0.5 and (g.get_state("d2", 1)[250:520] == 0).all()
    g.close()
    twin.close()


@pytest.mark.gpu
def test_refused_lists_leave_the_rings_alone(eng):
    """A list with a bad record behind a good CLEAR_RINGS changes nothing; CLEAR itself still stops at a ring node and says what to
    use; target 5 on a param node and target 6 are ERR_INVALID."""
    V, T = 80, 512 // 64 + 1
    build = build_two(eng, V, 4)
    g, twin = build(), build()
    ids = g.ids
    sig1, sig2 = two_signals(V, T, "max", 61), two_signals(V, T, "max", 1061)
    g.process_host(T, sig1), twin.process_host(T, sig1)
    before = all_tables(g)
    good = ml.Update.clear_rings(-1, 0, V)
    for bad, status, text in ((ml.Update.clear(ids["d1"], 0, 1), Status.ERR_UNSUPPORTED, "CLEAR_RINGS"), (ml.Update.clear(-1, 0, 1), Status.ERR_UNSUPPORTED, "rings"),
                              (ml.Update.clear_rings(ids["g"], 0, 1), Status.ERR_INVALID, "not a processor / feedback node"),
                              (ml.Update(ids["d1"], 6, 0, 0, 1, 0), Status.ERR_INVALID, "unknown target"), (ml.Update.clear_rings(ids["d1"], 79, 2), Status.ERR_RANGE, "voice range"),
                              (ml.Update.clear_rings(len(ids) + 50, 0, 1), Status.ERR_RANGE, "node index")):
        with pytest.raises(ml.MlgpuError) as ei:
            g.apply_updates([good, bad])
        assert ei.value.status == status and text in str(ei.value) and "record 1 of 2" in str(ei.value), str(ei.value)
        assert g.update_device_records([good, bad]) == 0
    after = all_tables(g)
    for k in before:
        assert same(before[k], after[k]), k
    ya, yb = g.process_host(T, sig2), twin.process_host(T, sig2)
    assert all(same(a, b) for a, b in zip(ya, yb)) and np.abs(ya[0]).max() > 0
    g.close()
    twin.close()


@pytest.mark.gpu
def test_between_the_launches_of_a_sequence(eng):
    """While recording the call is ERR_INVALID; between two launches of a recorded sequence the clear takes effect: the second launch
    gives what a direct twin gives with the same record between its two calls, and not what it gives without."""
    V, max_delay = 80, 100.0
    T = 256 // 64 + 1
    n = V * T * 64
    build = build_single(eng, V, Proc.INTEGER_DELAY, max_delay, 4)
    quad = lambda a: np.ascontiguousarray(a.reshape(V, T * 16, 4).transpose(1, 0, 2))
    d_x = eng.to_device(quad(lcg_noise(np.arange(V, dtype=np.uint32) + 71, 64 * T)))
    d_dt = eng.to_device(quad(delay_signal(V, T, max_delay, "max")))
    direct, recorded, untouched = build(), build(), build()
    d_a, d_b, d_c = eng.alloc(4 * n), eng.alloc(4 * n), eng.alloc(4 * n)
    rec = [ml.Update.clear_rings(recorded.ids["d"], 60, 20)]
    with pytest.raises(ml.MlgpuError) as ei:
        with eng.record():
            recorded.apply_updates(rec)
    assert ei.value.status == Status.ERR_INVALID and "recording" in str(ei.value)
    with eng.record() as seq:
        recorded.process(T, [d_x, d_dt], [d_b])
    outs = []
    for launch in range(2):
        direct.process(T, [d_x, d_dt], [d_a])
        untouched.process(T, [d_x, d_dt], [d_c])
        seq.launch()
        outs.append([d.download(np.float32, n).copy() for d in (d_a, d_b, d_c)])
        if launch == 0:
            direct.apply_updates(rec)
            recorded.apply_updates(rec)
    assert same(outs[0][0], outs[0][1]) and same(outs[0][0], outs[0][2])
    assert same(outs[1][0], outs[1][1]) and not same(outs[1][1], outs[1][2])
    seq.close()
    for g in (direct, recorded, untouched):
        g.close()


@pytest.mark.gpu
def test_on_a_bank_it_is_clear(eng):
    """Banks have no rings: CLEAR_RINGS gives the tables and outputs CLEAR gives, processor by processor and for all (-1)."""
    V, T = 80, 2
    banks = []
    for make in (ml.Update.clear, ml.Update.clear_rings):
        b = eng.bank([Proc.SAW_GEN, Proc.BANDPASS, Proc.GAIN], V)
        b.clear()
        b.set_coeffs(1, [float(c) for c in ml.Bandpass.makeCoeffs(0.1, 0.7)])
        b.set_coeff(2, 0, 0.25)
        b.set_input_const((55.0 * 2.0 ** (5.0 * np.arange(V) / V) / 48000.0).astype(np.float32))
        y0 = b.process_host(T)
        b.apply_updates([make(1, 60, 10), make(0, 79, 1)])
        y1 = b.process_host(T)
        b.apply_updates([make(-1, 64, 16)])
        y2 = b.process_host(T)
        banks.append((y0, y1, y2, b.get_all_state()))
        b.close()
    for a, c in zip(*banks):
        assert same(a, c)
    assert np.abs(banks[0][2]).max() > 1e-4
