"""The event rows vox, z, x, y and mod as source nodes of a voice graph, on the device (mlgpu_graph_add_event_row rows 2..6,
mlgpu_events_reserve_for_graph_rows).

THE COMPARATOR is mlgpu_events_process on a twin object fed the same events - e2s_kernel writing whole rows, itself pinned to the
reference's class by tests/test_gpu_events.py and, where oracle/_ref/libdropin_ref.so exists, compared with e2s_ref_run here too.
All comparisons are bitwise. Scenarios, performances and the engine fixture are those of tests/test_gpu_events.py. Blocks of 512
frames in launches of 3 vectors unless a test says otherwise: a 20 ms glide (15 vectors at 48 kHz) crosses launches and blocks."""
import os
import warnings

import numpy as np
import pytest

from inputs import assert_bits_equal
from test_gpu_events import CHAN_PRESS, CTRL, NOTE_ON, NOTE_PRESS, ROOT, SCENARIOS, eng, gpu_run, performance, ref_run  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu
BLOCK, N_BLOCKS = 512, 8
ROWS = (2, 3, 4, 5, 6)
ROW_NAMES = ("pitch", "gate", "vox", "z", "x", "y", "mod", "time")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdropin_ref.so")
# performance() seeds 100 k + SEED0[scenario] for instrument k: the first base, counted up from the scenario name's length as
# tests/test_gpu_events.py does, at which the rows of mlgpu_events_process satisfy moving_rows_condition (checked with the
# reference's class on the CPU)
SEED0 = dict(midi_poly4=10, midi_poly16=11, unison3=8, sustain=7, sr44k=5, sr8k=5, poly1=5)


def five_rows_desc():
    """The five rows as the graph's outputs (a source node can be one)."""
    names = [ROW_NAMES[r] for r in ROWS]
    return [dict(name=n, type="event_row", kind=r) for n, r in zip(names, ROWS)], names


def voice_desc(fused):
    """sine(pitch) * adsr(gate) * (1 + mod) + z * zAmt (a per-voice param), times one of two gains chosen by vox through select. fused:
    the five rows are event rows; else streamed inputs of the same names."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Op
    src = (lambda n, k: dict(name=n, type="event_row", kind=k)) if fused else (lambda n, k: dict(name=n, type="input"))
    op = lambda n, k, *ins: dict(name=n, type="op", kind=k, inputs=list(ins))  # noqa: E731
    return [src("pitch", 0), src("gate", 1), src("vox", 2), src("z", 3), src("mod", 6), dict(name="zAmt", type="param"),
            dict(name="one", type="const", value=1.0), dict(name="base", type="const", value=0.01), dict(name="half", type="const", value=0.5),
            dict(name="gA", type="const", value=0.75), dict(name="gB", type="const", value=0.25),
            op("ratio", Op.EXP2_APPROX, "pitch"), op("freq", Op.MULTIPLY, "ratio", "base"),
            dict(name="osc", type="proc", kind=ml.Proc.SINE_GEN, inputs=["freq"]), dict(name="env", type="proc", kind=ml.Proc.ADSR, inputs=["gate"]),
            op("amp", Op.MULTIPLY, "osc", "env"), op("m1", Op.ADD, "one", "mod"), op("wet", Op.MULTIPLY, "amp", "m1"), op("zv", Op.MULTIPLY, "z", "zAmt"),
            op("sum", Op.ADD, "wet", "zv"), op("gt", Op.GREATER_THAN, "vox", "half"), op("gain", Op.SELECT, "gA", "gB", "gt"),
            op("out", Op.MULTIPLY, "sum", "gain")], ["out"]


VOICE_ROWS = dict(pitch=0, gate=1, vox=2, z=3, mod=6)


def make_events(eng, cfg, N, wanted=None):
    import madronalib_amd as ml
    ev = ml.Events(eng, N, cfg["polyphony"], cfg.get("sr", 48000.0))
    ev.configure(mpe=0, unison=cfg.get("unison", 0), mod_cc=cfg.get("mod_cc", 16), pitch_bend=cfg.get("bend", 7.0), glide_seconds=cfg.get("glide", 0.0),
                 drift=cfg.get("drift", 0.0))
    if wanted is not None:
        ev.set_wanted_rows(wanted)
    return ev


def add_block(ev, instruments, b, block=BLOCK):
    import madronalib_amd as ml
    bi, be = [], []
    for i, evs in enumerate(instruments):
        for e in evs:
            if b * block <= e[3] < (b + 1) * block:
                bi.append(i)
                be.append(ml.Event(e[0], e[1], e[2], e[3] - b * block, e[4], e[5]))
    ev.add_events(bi, be)


def launches(vectors, block=BLOCK):
    done = 0
    while done < block // 64:
        T = min(vectors, block // 64 - done)
        yield T, done * 64
        done += T


def make_voice_graph(eng, V, fused, group=0, **switches):
    import madronalib_amd as ml
    desc, outs = voice_desc(fused)
    g = ml.Graph(eng, V, desc, outs, output_groups={0: group} if (group and (fused or switches)) else None, **switches)
    g.clear()
    g.set_param("zAmt", (0.25 + 0.5 * ((np.arange(V) * 7) % 5) / 5.0).astype(np.float32))
    g.set_coeffs("env", [np.full(V, c, np.float32) for c in ml.ADSR.calcCoeffs(0.004, 0.02, 0.6, 0.03, 48000.0)])
    return g


def fused_rows(eng, cfg, instruments, n_blocks=N_BLOCKS, vectors=3, reserve=None):
    """The five rows [5][V][frames] made by the graph of five_rows_desc through mlgpu_graph_process_events."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout
    N, P = len(instruments), cfg["polyphony"]
    V = N * P
    ev = make_events(eng, cfg, N)
    desc, outs = five_rows_desc()
    g = ml.Graph(eng, V, desc, outs)
    g.clear()
    assert "mlev::CtlRows<124u>" in g.source and "mlev::CtlVoice" not in g.source and not g.inputs
    g.bind_events(ev)
    if reserve is not None:
        ev.reserve_for_graph(*reserve)
    d_out = [eng.alloc(4 * V * vectors * 64) for _ in ROWS]
    chunks = []
    for b in range(n_blocks):
        add_block(ev, instruments, b)
        for T, off in launches(vectors):
            g.process_events(T, off, [], d_out, out_layout=Layout.VOICE_MAJOR)
            chunks.append(np.stack([d.download(np.float32, V * T * 64).reshape(V, T * 64).copy() for d in d_out]))
        ev.clear_events()
    g.close()
    ev.close()
    return np.concatenate(chunks, 2)


def distinct_in_a_vector(row):
    """row [V][frames]: the largest number of distinct values any voice has inside one DSPVector."""
    v = np.sort(row.reshape(row.shape[0], -1, 64).view(np.uint32), axis=-1)
    return int((np.diff(v, axis=-1) != 0).sum(-1).max()) + 1


def moving_rows_condition(rows8, what):
    """Of mlgpu_events_process' rows [8][V][frames]: each of z, x, y, mod has a vector with 3 or more distinct values in some voice - a
    moving glide is really expanded -, and z is back at 0 somewhere after a note-off."""
    for r in (3, 4, 5, 6):
        assert distinct_in_a_vector(rows8[r]) >= 3, f"{what}: row {ROW_NAMES[r]} never moves inside a vector"
    z, gate = rows8[3], rows8[1]
    nz = z != 0
    back = False
    for v in range(z.shape[0]):
        if nz[v].any():
            first = int(np.argmax(nz[v]))
            back = back or bool(((z[v, first:] == 0) & (gate[v, first:] == 0)).any())
    assert back, f"{what}: z never returns to 0 after a note-off"


def scenario(name, n=6, n_blocks=N_BLOCKS, drift=None):
    cfg = dict(SCENARIOS[name]) if drift is None else dict(SCENARIOS[name], drift=drift)
    kind = "sustain" if name == "sustain" else "midi"
    return cfg, [performance(kind, 100 * k + SEED0[name], BLOCK * n_blocks, cfg["polyphony"]) for k in range(n)]


@pytest.mark.parametrize("name,flush", [("midi_poly4", False), ("midi_poly4", True), ("midi_poly16", False), ("unison3", False), ("sustain", False),
                                        ("sr44k", False), ("sr8k", False), ("poly1", False)])
def test_each_row_by_itself(eng, name, flush):
    """A graph whose outputs are the five rows, 6 instruments, 8 blocks: every voice's rows have the bits of mlgpu_events_process on a
    twin object and of the reference's class."""
    cfg, instruments = scenario(name)
    eng.set_flush_denormals(flush)
    try:
        want = gpu_run(eng, cfg, instruments, BLOCK, N_BLOCKS, 3, rows=[1, 2, 3, 4, 5, 6])
        got = fused_rows(eng, cfg, instruments)
    finally:
        eng.set_flush_denormals(False)
    moving_rows_condition(want, name)
    for i, r in enumerate(ROWS):
        assert_bits_equal(got[i], want[r], True, f"{name} flush {flush}: row {ROW_NAMES[r]}, graph node vs mlgpu_events_process")
    if not os.path.exists(REF_SO):
        warnings.warn("oracle/_ref/libdropin_ref.so is not here: the event rows were NOT compared with the reference's class (e2s_ref_run)")
        return
    P = cfg["polyphony"]
    for k, evs in enumerate(instruments):
        ref = ref_run(cfg, evs, BLOCK, N_BLOCKS)
        for i, r in enumerate(ROWS):
            assert_bits_equal(got[i, k * P:(k + 1) * P], ref[r], True, f"{name}: instrument {k} row {ROW_NAMES[r]}, graph node vs the reference")


def run_voice(eng, cfg, instruments, forms, group=0, vectors=3):
    """The voice of voice_desc through the performance, block b in forms[b]: "fused" - the rows are event rows of the graph - or "mem" -
    mlgpu_events_process writes the five rows, the plain graph reads them. One events object; on a change of form the other graph takes
    the voice state over. Returns the audio [V][frames], or with `group` the instruments' [N][frames] (fused: summed in the kernel;
    mem: mlgpu_mixdown_groups)."""
    from madronalib_amd.constants import Layout
    N, P = len(instruments), cfg["polyphony"]
    V = N * P
    ev = make_events(eng, cfg, N, wanted=[0, 1, 2, 3, 6])
    graphs = {f: make_voice_graph(eng, V, f == "fused", group) for f in set(forms)}
    if "fused" in graphs:
        assert "mlev::CtlRows<76u>" in graphs["fused"].source and "mlev::CtlVoice" in graphs["fused"].source and not graphs["fused"].inputs
        graphs["fused"].bind_events(ev)
    n = V * vectors * 64
    rows = {nm: eng.alloc(4 * n) for nm in VOICE_ROWS}
    d_out, d_mix = eng.alloc(4 * n), eng.alloc(4 * n)
    chunks = []
    for b, form in enumerate(forms):
        add_block(ev, instruments, b)
        if b and forms[b - 1] != form:
            for nd in ("osc", "env"):
                for i in range(graphs[form].num_state(nd)):
                    graphs[form].set_state(nd, i, graphs[forms[b - 1]].get_state(nd, i))
        g = graphs[form]
        for T, off in launches(vectors):
            if form == "fused":
                g.process_events(T, off, [], [d_mix if group else d_out], out_layout=Layout.VOICE_MAJOR)
            else:
                ev.process(T, off, [rows.get(ROW_NAMES[r]) for r in range(8)], Layout.QUAD)
                g.process(T, [rows[nm] for nm in g.inputs], [d_out], out_layout=Layout.VOICE_MAJOR)
                if group:
                    eng.mixdown_groups(d_out, Layout.VOICE_MAJOR, N, P, T, d_mix, Layout.VOICE_MAJOR)
            R = N if group else V
            chunks.append((d_mix if group else d_out).download(np.float32, R * T * 64).reshape(R, T * 64).copy())
        ev.clear_events()
    for g in graphs.values():
        g.close()
    ev.close()
    return np.concatenate(chunks, 1)


def test_a_voice_that_uses_the_rows(eng):
    """6 instruments x 4 voices: the fused voice's audio has the bits of the rows-in-memory form."""
    cfg, instruments = scenario("midi_poly4")
    a = run_voice(eng, cfg, instruments, ["mem"] * N_BLOCKS)
    b = run_voice(eng, cfg, instruments, ["fused"] * N_BLOCKS)
    assert_bits_equal(b, a, True, "voice with mod, z and vox: fused vs rows in memory")
    assert np.abs(a).max() > 0


def test_a_voice_that_uses_the_rows_summed_per_instrument(eng):
    """37 instruments of 4 voices (a partial last wavefront), the voices summed per instrument inside the fused kernel, against
    mlgpu_mixdown_groups over the rows-in-memory form."""
    cfg = SCENARIOS["midi_poly4"]
    instruments = [performance("midi", 31 * k + 10, BLOCK * 4, 4) for k in range(37)]
    a = run_voice(eng, cfg, instruments, ["mem"] * 4, group=4, vectors=8)
    b = run_voice(eng, cfg, instruments, ["fused"] * 4, group=4, vectors=8)
    assert_bits_equal(b, a, True, "instrument audio with mod, z and vox: one kernel vs three")
    assert np.abs(a).max() > 0


@pytest.mark.parametrize("first", ["fused", "mem"])
def test_hand_over_in_the_middle_of_a_glide(eng, first):
    """Four blocks by one form, four by the other, both ways: the bits of eight two-kernel blocks. Instrument 0 gets a note, a mod-wheel
    event and a note pressure three vectors before the switch, so the mod and z glides are moving when the other form takes over."""
    cfg, instruments = scenario("midi_poly4")
    switch = 4 * BLOCK
    extra = [(NOTE_ON, 1, 100, switch - 5 * 64 + 3, 0.5, 0.8), (CTRL, 1, 16, switch - 3 * 64 + 5, float(np.float32(0.9137)), 0.0),
             (NOTE_PRESS, 1, 100, switch - 3 * 64 + 9, float(np.float32(0.77)), 0.0)]
    instruments[0] = sorted(instruments[0] + extra, key=lambda e: e[3])
    rows = gpu_run(eng, cfg, instruments, BLOCK, N_BLOCKS, 3, rows=[1, 3, 6])
    for v in range(4):      # the mod wheel reaches every voice of the instrument
        assert len(np.unique(rows[6, v, switch:switch + 64])) > 1, "the mod row rests in the first vector after the switch"
    assert max(len(np.unique(rows[3, v, switch:switch + 64])) for v in range(4)) > 1, "the z row rests in the first vector after the switch"
    other = "mem" if first == "fused" else "fused"
    want = run_voice(eng, cfg, instruments, ["mem"] * N_BLOCKS)
    got = run_voice(eng, cfg, instruments, [first] * 4 + [other] * 4)
    assert_bits_equal(got, want, True, f"four blocks {first}, then four {other}")


class ListedRig:
    """An events object and a listed graph over its voices, driven by the intended block: route_ahead, sounding_voices, the list."""

    def __init__(self, eng, cfg, N, graph, max_vectors=3):
        self.eng, self.P, self.V, self.g = eng, cfg["polyphony"], N * cfg["polyphony"], graph
        self.ev = make_events(eng, cfg, N, wanted=[0, 1, 2, 3, 6])
        self.d_out = [eng.alloc(4 * self.V * max_vectors * 64 + 64) for _ in range(len(graph.outputs))]
        self.d_peak = eng.alloc(4 * self.V + 64)
        self.rows = {nm: eng.alloc(4 * self.V * max_vectors * 64) for nm in VOICE_ROWS}

    def close(self):
        self.g.close()
        self.ev.close()


def lists_with_a_gap(P, instrument, from_launch):
    """The list of a launch: sounding_voices() united with the two launches before (the tails) - and, in the launches from_launch and
    from_launch + 1, without the first sounding voice of `instrument`, which is back in the list after them."""
    hist, state = [], dict(n=0, dropped=None)

    def make(s):
        L = np.unique(np.concatenate([s] + hist[-2:])).astype(np.uint32)
        hist.append(s)
        if state["n"] in (from_launch, from_launch + 1):
            if state["dropped"] is None:
                mine = [int(v) for v in s if v // P == instrument]
                assert mine, "no voice of the instrument sounds where one is to be dropped"
                state["dropped"] = mine[0]
            L = L[L != state["dropped"]]
        state["n"] += 1
        return L
    return make, state


def with_a_held_note_and_a_mod_event(instruments, at):
    """Instrument 0 holds a key of its own from frame at - 100 on and gets a mod-wheel event at frame `at`."""
    extra = [(NOTE_ON, 1, 100, at - 100, 0.5, 0.8), (CTRL, 1, 16, at, float(np.float32(0.8642)), 0.0)]
    instruments[0] = sorted(instruments[0] + extra, key=lambda e: e[3])


def test_listed_rows_have_the_bits_of_never_having_used_lists(eng):
    """The graph of the five rows, listed (voice_list_events), drift 0.3: every listed voice's rows z, x, y, mod - and vox - are those of
    the unlisted fused run, also for a voice left off the list for two launches right after a mod-wheel event, from its first listed
    vector on: the control kernel runs for every lane in every call."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout
    cfg, instruments = scenario("midi_poly4", drift=0.3)
    with_a_held_note_and_a_mod_event(instruments, 1000)       # block 1, its last launch (frames 896 .. 1023) is launch 5
    want = fused_rows(eng, cfg, instruments)
    desc, outs = five_rows_desc()
    V = 6 * 4
    g = ml.Graph(eng, V, desc, outs, voice_lists=True, voice_list_events=True)
    g.clear()
    rig = ListedRig(eng, cfg, 6, g)
    g.bind_events(rig.ev)
    g.reserve_voice_list(V)
    make, state = lists_with_a_gap(4, 0, 6)
    frame, relisted_moves, n = 0, False, 0
    for b in range(N_BLOCKS):
        add_block(rig.ev, instruments, b)
        for T, off in launches(3):
            rig.ev.route_ahead(T, off)
            L = make(rig.ev.sounding_voices())
            g.set_voice_list(L)
            g.process_events_listed(T, off, [], rig.d_out, out_layout=Layout.VOICE_MAJOR, d_peak=rig.d_peak)
            for i, r in enumerate(ROWS):
                got = rig.d_out[i].download(np.float32, len(L) * T * 64).reshape(len(L), T * 64)
                assert_bits_equal(got, want[i][L, frame:frame + T * 64], True, f"block {b} offset {off}: row {ROW_NAMES[r]} of the listed voices")
            if n == 8:      # the launch that has the dropped voice back
                d = state["dropped"]
                assert d is not None and d in L
                relisted_moves = len(np.unique(want[4][d, frame:frame + 64])) > 1
            frame += T * 64
            n += 1
        rig.ev.clear_events()
    assert relisted_moves, "the relisted voice's mod glide was at rest when it came back"
    rig.close()


def test_listed_voice_through_the_lane_plan(eng):
    """The voice of voice_desc, 19 instruments of 4, drift 0, listed by the lane plan (voice_list_groups, group 4) with the same gap in
    the lists: the listed instruments' sums and the peaks against the comparator - mlgpu_events_process writing the rows of all voices,
    the twin graph reading them through process_listed_groups with the same lists."""
    from madronalib_amd.constants import Layout
    cfg = dict(SCENARIOS["midi_poly4"], drift=0.0)
    N, P = 19, 4
    V = N * P
    instruments = [performance("midi", 100 * k + 10, BLOCK * 4, P) for k in range(N)]
    with_a_held_note_and_a_mod_event(instruments, 1000)
    outs = []
    for fused in (True, False):
        g = make_voice_graph(eng, V, fused, group=P, voice_lists=True, voice_list_groups=True, voice_list_events=fused)
        rig = ListedRig(eng, cfg, N, g)
        if fused:
            g.bind_events(rig.ev)
        g.reserve_voice_list_groups(V)
        make, _ = lists_with_a_gap(P, 0, 6)
        log = []
        for b in range(4):
            add_block(rig.ev, instruments, b)
            for T, off in launches(3):
                rig.ev.route_ahead(T, off)
                L = make(rig.ev.sounding_voices())
                g.set_voice_list(L)
                if fused:
                    g.process_events_listed_groups(T, off, [], rig.d_out, out_layout=Layout.VOICE_MAJOR, d_peak=rig.d_peak)
                else:
                    rig.ev.process(T, off, [rig.rows.get(ROW_NAMES[r]) for r in range(8)], Layout.VOICE_MAJOR)
                    g.process_listed_groups(T, [rig.rows[nm] for nm in g.inputs], rig.d_out, in_layout=Layout.VOICE_MAJOR, out_layout=Layout.VOICE_MAJOR,
                                            d_peak=rig.d_peak)
                J = len(g.listed_groups)
                log.append((L, rig.d_out[0].download(np.float32, J * T * 64).reshape(J, T * 64).copy(), rig.d_peak.download(np.uint32, len(L)).copy()))
            rig.ev.clear_events()
        rig.close()
        outs.append(log)
    loud = False
    for n, ((La, ya, pa), (Lb, yb, pb)) in enumerate(zip(*outs)):
        assert (La == Lb).all()
        assert_bits_equal(ya, yb, True, f"launch {n}: the listed instruments' sums")
        assert_bits_equal(pa, pb, False, f"launch {n}: peaks")
        loud = loud or bool(np.abs(ya).max() > 0)
    assert loud


def test_sleeping_instruments_and_a_ragged_bank(eng):
    """801 instruments of 3 voices = 2403 lanes (the control kernel's block remap and a ragged last block), every seventh playing: the
    rows against mlgpu_events_process; z, x, y and mod are zero for the silent instruments, vox is not."""
    cfg = dict(polyphony=3, glide=0.01, drift=0.4)
    N, n_blocks = 801, 2
    # (the performance plus one event of each controller, so that every row of a playing instrument leaves zero)
    extra = [(CTRL, 1, 16, 70, 0.4, 0.0), (CTRL, 1, 73, 130, 0.5, 0.0), (CTRL, 1, 74, 200, 0.6, 0.0), (CHAN_PRESS, 1, 0, 260, 0.7, 0.0)]
    evs = sorted(performance("midi", 11, BLOCK * n_blocks, 3) + extra, key=lambda e: e[3])
    instruments = [evs if (k % 7 == 0) else [] for k in range(N)]
    want = gpu_run(eng, cfg, instruments, BLOCK, n_blocks, 8, rows=[2, 3, 4, 5, 6])
    got = fused_rows(eng, cfg, instruments, n_blocks=n_blocks, vectors=8)
    for i, r in enumerate(ROWS):
        assert_bits_equal(got[i], want[r], True, f"2403 voices: row {ROW_NAMES[r]}")
    silent = np.array([k % 7 != 0 for k in range(N)]).repeat(3)
    for i in (1, 2, 3, 4):
        assert not got[i][silent].any(), f"row {ROW_NAMES[ROWS[i]]} of a sleeping instrument"
        assert got[i][~silent].any()
    vox = got[0].reshape(N, 3, -1)
    assert (vox[:, 0] == 0).all() and (vox[:, 1] == 1).all() and (vox[:, 2] == 2).all()


def test_reserve_by_rows(eng):
    """The bytes of a reserve by row mask; after reserve_for_graph(4, rows=[0, 1, 6]) a graph with z is refused and a 5-vector block gets
    the RANGE error, both before the router consumes anything: the same block then processed by a graph the reserve covers has the bits
    of a run without the refused calls."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Status
    cfg, instruments = scenario("midi_poly4", n=4)
    instruments[0] = sorted(instruments[0] + [(CTRL, 1, 16, 300, 0.6, 0.0)], key=lambda e: e[3])     # the mod row moves in the blocks compared
    N, P = 4, 4
    V = N * P
    ev = make_events(eng, cfg, N)
    for n in (1, 4, 16):
        assert ev.graph_reserve_bytes(n) == 528 * n * V
        for rows, k in (([0, 1], 0), ([6], 1), ([0, 1, 2], 0), ([2, 3, 6], 2), ([3, 4, 5, 6], 4), ([0, 1, 2, 3, 4, 5, 6], 4)):
            assert ev.graph_reserve_bytes(n, rows) == (16 + 512 + 260 * k) * n * V
    assert ev.graph_reserve_bytes(4, [7]) == 0
    with pytest.raises(ml.MlgpuError) as ei:
        ev.reserve_for_graph(4, rows=[0, 1, 7])
    assert ei.value.status == Status.ERR_UNSUPPORTED
    ev.close()

    def run(refusals):
        ev = make_events(eng, cfg, N)
        gm = ml.Graph(eng, V, [dict(name="mod", type="event_row", kind=6)], ["mod"])
        gz = ml.Graph(eng, V, [dict(name="z", type="event_row", kind=3), dict(name="mod", type="event_row", kind=6)], ["z", "mod"])
        for g in (gm, gz):
            g.clear()
            g.bind_events(ev)
        ev.reserve_for_graph(4, rows=[0, 1, 6])
        d = [eng.alloc(4 * V * 5 * 64), eng.alloc(4 * V * 5 * 64)]
        chunks = []
        for b in range(3):
            add_block(ev, instruments, b)
            for T, off in launches(4):
                if refusals:
                    with pytest.raises(ml.MlgpuError) as ei:
                        gz.process_events(T, off, [], d, out_layout=Layout.VOICE_MAJOR)
                    assert ei.value.status == Status.ERR_INVALID and "3 (z)" in str(ei.value)
                    with pytest.raises(ml.MlgpuError) as ei:
                        gm.process_events(5, off, [], d[:1], out_layout=Layout.VOICE_MAJOR)
                    assert ei.value.status == Status.ERR_RANGE
                gm.process_events(T, off, [], d[:1], out_layout=Layout.VOICE_MAJOR)
                chunks.append(d[0].download(np.float32, V * T * 64).reshape(V, T * 64).copy())
            ev.clear_events()
        gm.close(), gz.close(), ev.close()
        return np.concatenate(chunks, 1)
    a, b = run(False), run(True)
    assert_bits_equal(b, a, True, "the mod row after refused calls vs without them")
    assert distinct_in_a_vector(a) >= 3
