"""Event rows of a voice graph under the MPE protocol, on the device (mlgpu_graph_enable_mpe_events): an instrument is
G = nextpow2(polyphony + 1) lanes of the events object - its main voice, its playing voices, padding -, a playing voice's rows are its own
plus the main voice's, and the protocol is data of the launch.

THE COMPARATOR is mlgpu_events_process on a twin MPE object fed the same events - e2s_kernel writing whole rows, pinned to the reference's
class by tests/test_gpu_events.py (scenario mpe5) - and, where oracle/_ref/libdropin_ref.so exists, the reference's class itself
(e2s_ref_run). Every comparison is bitwise. 6 blocks of 512 frames in launches of 3, 3 and 2 vectors; glide 0.01 s, MPE bend range 48.

The performances are this file's own: tests/test_gpu_events.py's generator never sends a controller on channel 1; this one sends CC 73,
CC 74 and the mod CC there too, beside channel-1 bend and pressure and the member channels' events."""
import os
import warnings

import numpy as np
import pytest

from inputs import assert_bits_equal
from test_gpu_events import BEND, CHAN_PRESS, CTRL, NOTE_OFF, NOTE_ON, ROOT, eng, gpu_run, performance, ref_run  # noqa: F401  (eng: the module's engine fixture)

pytestmark = pytest.mark.gpu
BLOCK, N_BLOCKS = 512, 6
ROW_NAMES = ("pitch", "gate", "vox", "z", "x", "y", "mod")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libdropin_ref.so")
# polyphony, instruments, drift: where the lane arithmetic can go wrong
SHAPES = {
    "P5_V130": dict(P=5, N=26, drift=0.3),    # G = 8: instruments straddle the voice kernel's wavefronts; a partial last wavefront
    "P16_V80": dict(P=16, N=5, drift=0.0),    # G = 32: a large group
    "P7_V70": dict(P=7, N=10, drift=0.3),     # G = 8: no padding lane
    "P8_V72": dict(P=8, N=9, drift=0.0),      # G = 16: seven padding lanes
    "P1_V70": dict(P=1, N=70, drift=0.3),     # G = 2: single-voice instruments
}
SEED0 = 3     # instrument k's performance has seed 100 k + SEED0: the conditions of reference_conditions hold there (checked with the reference's class on the CPU)


def config(P, drift, mpe=1):
    return dict(polyphony=P, mpe=mpe, glide=0.01, drift=drift, mpe_bend=48.0)


def mpe_performance(seed, frames, P, burst):
    """A scripted MPE event list (type, channel, sourceIdx, time, value1, value2): notes on the member channels 2 .. P + 3 (two more
    channels than voices: voices are stolen), bends, pressure and the controllers 73, 74 and 16 (mod) on a member channel or on channel 1.
    burst: P + 1 note-ons on P + 1 channels first - the last one steals."""
    rng = np.random.default_rng(seed)
    evs, held, t = [], [], int(rng.integers(0, 150))
    if burst:
        for j in range(P + 1):
            evs.append((NOTE_ON, 2 + j, 40 + j, t, float(np.float32((j - 6) / 12.0)), float(np.float32(0.3 + 0.04 * j))))
            held.append((2 + j, 40 + j))
            t += int(rng.integers(1, 9))
    while t < frames - 10:
        r = rng.random()
        chan = int(rng.integers(2, 2 + P + 2))
        one = rng.random() < 0.4     # ... on channel 1: the main voice
        if r < 0.28 or not held:
            key = int(rng.integers(30, 90))
            evs.append((NOTE_ON, chan, key, t, float(np.float32((key - 60) / 12.0)), float(np.float32(rng.uniform(0.1, 1.0)))))
            held.append((chan, key))
        elif r < 0.45:
            c, k = held.pop(int(rng.integers(0, len(held))))
            evs.append((NOTE_OFF, c, k, t, 0.0, 0.0))
        elif r < 0.60:
            evs.append((BEND, 1 if one else chan, 0, t, float(np.float32(rng.uniform(-1, 1))), 0.0))
        elif r < 0.82:
            cc = int(rng.choice([16, 73, 74]))
            c = 1 if one else (held[int(rng.integers(0, len(held)))][0] if rng.random() < 0.7 else chan)     # mostly a channel that holds a note
            evs.append((CTRL, c, cc, t, float(np.float32(rng.random())), 0.0))
        elif r < 0.94:
            c = 1 if one else (held[int(rng.integers(0, len(held)))][0] if rng.random() < 0.7 else chan)
            evs.append((CHAN_PRESS, c, 0, t, float(np.float32(rng.random())), 0.0))
        elif r < 0.96:
            evs.append((CTRL, 1, 123, t, 0.0, 0.0))        # all notes off
            held = []
        t += int(rng.integers(1, 220)) if rng.random() < 0.9 else 0   # now and then two events on the same frame
    return evs


def shape_instruments(name, n_blocks=N_BLOCKS):
    s = SHAPES[name]
    return config(s["P"], s["drift"]), [mpe_performance(100 * k + SEED0, BLOCK * n_blocks, s["P"], burst=(k % 3 == 0)) for k in range(s["N"])]


def seven_rows_desc(with_sum=False):
    """The seven rows as the graph's outputs (a source node can be one); with_sum: one more node, (((((pitch + gate) + vox) + z) + x) + y) + mod."""
    from madronalib_amd.constants import Op
    desc = [dict(name=n, type="event_row", kind=r) for r, n in enumerate(ROW_NAMES)]
    if not with_sum:
        return desc, list(ROW_NAMES)
    acc = "pitch"
    for i, n in enumerate(ROW_NAMES[1:]):
        desc.append(dict(name=f"s{i}", type="op", kind=Op.ADD, inputs=[acc, n]))
        acc = f"s{i}"
    return desc, [acc]


def make_events(eng, cfg, N):
    import madronalib_amd as ml
    ev = ml.Events(eng, N, cfg["polyphony"], cfg.get("sr", 48000.0))
    ev.configure(mpe=cfg.get("mpe", 0), mod_cc=16, pitch_bend=cfg.get("bend", 7.0), mpe_pitch_bend=cfg.get("mpe_bend", 24.0),
                 glide_seconds=cfg.get("glide", 0.0), drift=cfg.get("drift", 0.0))
    return ev


def add_block(ev, instruments, b):
    import madronalib_amd as ml
    bi, be = [], []
    for i, evs in enumerate(instruments):
        for e in evs:
            if b * BLOCK <= e[3] < (b + 1) * BLOCK:
                bi.append(i)
                be.append(ml.Event(e[0], e[1], e[2], e[3] - b * BLOCK, e[4], e[5]))
    ev.add_events(bi, be)


LAUNCHES = ((3, 0), (3, 192), (2, 384))     # a block of 8 vectors: 3, 3 and the uneven remainder


def rows_graph(eng, V, **switches):
    import madronalib_amd as ml
    desc, outs = seven_rows_desc()
    g = ml.Graph(eng, V, desc, outs, **switches)
    g.clear()
    return g


class RowsRig:
    """An events object and the graph of the seven rows bound to it; block(): one block by the graph or by mlgpu_events_process."""

    def __init__(self, eng, cfg, N, mpe_events=True, reserve=None):
        self.eng, self.N, self.V = eng, N, N * cfg["polyphony"]
        self.ev = make_events(eng, cfg, N)
        self.g = rows_graph(eng, self.V, mpe_events=mpe_events)
        if mpe_events:
            assert "mlev::CtlVoiceMpe ev_0;" in self.g.source and "mlev::CtlRowsMpe<124u> er_0;" in self.g.source and not self.g.inputs
        self.g.bind_events(self.ev)
        if reserve is not None:
            self.ev.reserve_for_graph(reserve, rows=range(7))
        self.d = [eng.alloc(4 * self.V * 4 * 64) for _ in range(8)]

    def launch(self, T, off, fused=True):
        from madronalib_amd.constants import Layout
        if fused:
            self.g.process_events(T, off, [], self.d[:7], out_layout=Layout.VOICE_MAJOR)
        else:
            self.ev.process(T, off, self.d, Layout.VOICE_MAJOR)
        return np.stack([d.download(np.float32, self.V * T * 64).reshape(self.V, T * 64).copy() for d in self.d[:7]])

    def block(self, instruments, b, fused=True):
        add_block(self.ev, instruments, b)
        out = np.concatenate([self.launch(T, off, fused) for T, off in LAUNCHES], 2)
        self.ev.clear_events()
        return out

    def close(self):
        self.g.close()
        self.ev.close()


_cache = {}


def comparator_rows(eng, name):
    """[8][V][frames] of mlgpu_events_process on an MPE object, once per shape."""
    if ("want", name) not in _cache:
        cfg, instruments = shape_instruments(name)
        _cache["want", name] = gpu_run(eng, cfg, instruments, BLOCK, N_BLOCKS, 3)
        _cache["want", name].setflags(write=False)
    return _cache["want", name]


def one_frame_gate_gaps(gate):
    """gate [P][frames]: frames where a voice's gate is 0 between two non-zero frames - a retrigger: the voice was stolen."""
    return int(((gate[:, 1:-1] == 0) & (gate[:, :-2] != 0) & (gate[:, 2:] != 0)).sum())


def reference_conditions(name, cfg, instruments, refs):
    """On the reference's output alone: the main voice's bend reaches a playing voice's pitch row, each of z, x, y, mod moves in some
    voice, a voice is stolen."""
    for r in (3, 4, 5, 6):
        assert any(len(np.unique(ref[r, v])) > 2 for ref in refs for v in range(ref.shape[1])), f"{name}: row {ROW_NAMES[r]} is constant in every voice"
    assert sum(one_frame_gate_gaps(ref[1]) for ref in refs) > 0, f"{name}: no voice is stolen"
    for evs, ref in zip(instruments, refs):
        without = [e for e in evs if not (e[0] == BEND and e[1] == 1)]
        if len(without) != len(evs) and (ref_run(cfg, without, BLOCK, N_BLOCKS)[0].view(np.uint32) != ref[0].view(np.uint32)).any():
            return
    assert False, f"{name}: the channel-1 bends change no pitch row"


@pytest.mark.parametrize("name", list(SHAPES))
def test_rows(eng, name):
    """The seven rows passed through a graph built with the switch and bound to an MPE object: every voice and sample has the bits of
    mlgpu_events_process on a twin object and of the reference's class."""
    cfg, instruments = shape_instruments(name)
    N, P = len(instruments), cfg["polyphony"]
    want = comparator_rows(eng, name)
    rig = RowsRig(eng, cfg, N)
    got = np.concatenate([rig.block(instruments, b) for b in range(N_BLOCKS)], 2)
    rig.close()
    _cache["got", name] = got
    for r in range(7):
        assert_bits_equal(got[r], want[r], True, f"{name}: row {ROW_NAMES[r]}, graph node vs mlgpu_events_process")
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0
    if not os.path.exists(REF_SO):
        warnings.warn("oracle/_ref/libdropin_ref.so is not here: the MPE event rows were NOT compared with the reference's class (e2s_ref_run)")
        pytest.skip("oracle/_ref/libdropin_ref.so not available here: compared with mlgpu_events_process only")
    refs = [ref_run(cfg, evs, BLOCK, N_BLOCKS) for evs in instruments]
    reference_conditions(name, cfg, instruments, refs)
    for k, ref in enumerate(refs):
        for r in range(7):
            assert_bits_equal(got[r, k * P:(k + 1) * P], ref[r], True, f"{name}: instrument {k} row {ROW_NAMES[r]}, graph node vs the reference")


@pytest.mark.parametrize("P,N", [(4, 9), (16, 5)])
def test_pitch_and_gate_only(eng, P, N):
    """The instance of the control kernel without controller rows: the config-5 voice with pitch and gate as event rows, its output
    summed per instrument inside the kernel, against the three-kernel route - mlgpu_events_process writes rows 0 and 1, the same patch
    reads them as inputs, mlgpu_mixdown_groups sums."""
    import madronalib_amd as ml
    from madronalib_amd import patches
    from madronalib_amd.constants import Layout
    from madronalib_amd.sharding import cfg5_voice_params
    cfg = config(P, 0.3)
    V, n_blocks = N * P, 4
    instruments = [mpe_performance(100 * k + SEED0, BLOCK * n_blocks, P, burst=(k % 3 == 0)) for k in range(N)]
    outs = []
    for fused in (False, True):
        ev = make_events(eng, cfg, N)
        ev.set_wanted_rows([0, 1])
        params, coeffs, seeds = cfg5_voice_params(0, V, V, ml)
        desc, outn = patches.synth16(pitch_input=True, event_rows=fused)
        g = ml.Graph(eng, V, desc, outn, output_groups={0: P} if fused else None, mpe_events=fused)
        g.clear()
        for k, v in params.items():
            if k != "pitch":
                g.set_param(k, v if np.ndim(v) else float(v))
        for k, c in coeffs.items():
            g.set_coeffs(k, [np.ascontiguousarray(r) for r in c])
        g.set_state("noise", 0, seeds)
        if fused:
            assert "mlev::CtlVoiceMpe ev_0;" in g.source and "CtlRows" not in g.source and not g.inputs
            g.bind_events(ev)
        n = V * 3 * 64
        rows, d_out, d_mix = [eng.alloc(4 * n), eng.alloc(4 * n)], eng.alloc(4 * n), eng.alloc(4 * n)
        chunks = []
        for b in range(n_blocks):
            add_block(ev, instruments, b)
            for T, off in LAUNCHES:
                if fused:
                    g.process_events(T, off, [], [d_mix], out_layout=Layout.VOICE_MAJOR)
                else:
                    ev.process(T, off, rows + [None] * 6, Layout.QUAD)
                    g.process(T, [rows[1] if nm == "gate" else rows[0] for nm in g.inputs], [d_out], out_layout=Layout.VOICE_MAJOR)
                    eng.mixdown_groups(d_out, Layout.VOICE_MAJOR, N, P, T, d_mix, Layout.VOICE_MAJOR)
                chunks.append(d_mix.download(np.float32, N * T * 64).reshape(N, T * 64).copy())
            ev.clear_events()
        outs.append(np.concatenate(chunks, 1))
        g.close()
        ev.close()
    assert_bits_equal(outs[1], outs[0], True, f"polyphony {P}: instrument audio, one voice kernel vs three kernels")
    assert (np.abs(outs[0]).max(axis=1) > 0).all()


def hand_over_instruments():
    """6 instruments of 5 voices; instrument 0 is scripted: two held notes, and three vectors before every block boundary a controller,
    a pressure and a bend on their channels and a bend and a controller on channel 1 - 20 ms glides (15 vectors) that move across it."""
    cfg = config(5, 0.3)
    instruments = [mpe_performance(100 * k + SEED0, BLOCK * N_BLOCKS, 5, burst=(k % 3 == 0)) for k in range(6)]
    evs = [(NOTE_ON, 2, 50, 10, float(np.float32(-0.5)), 0.7), (NOTE_ON, 3, 57, 20, 0.25, 0.5)]
    for b in range(1, N_BLOCKS):
        t, x = b * BLOCK - 3 * 64, float(np.float32(0.11 * b))
        evs += [(CTRL, 2, 74, t + 5, x + 0.2, 0.0), (CTRL, 3, 16, t + 9, x + 0.1, 0.0), (CHAN_PRESS, 2, 0, t + 11, x + 0.3, 0.0), (CTRL, 2, 73, t + 12, 0.9 - x, 0.0),
                (BEND, 1, 0, t + 17, x - 0.4, 0.0), (BEND, 3, 0, t + 23, 0.5 - x, 0.0), (CTRL, 1, 74, t + 29, x, 0.0)]
    instruments[0] = evs
    return cfg, instruments


@pytest.mark.parametrize("first", ["graph", "events"])
def test_hand_over(eng, first):
    """One object, the blocks alternately by mlgpu_events_process and by the graph's process_events, in both starting orders: the rows of
    a twin object that only ever used mlgpu_events_process. In the first vector after every switch the main voice's bend glide and
    instrument 0's controller glides are moving."""
    cfg, instruments = hand_over_instruments()
    if "hand_over" not in _cache:
        _cache["hand_over"] = gpu_run(eng, cfg, instruments, BLOCK, N_BLOCKS, 3)
    want = _cache["hand_over"]
    for b in range(1, N_BLOCKS):
        at = slice(b * BLOCK, b * BLOCK + 64)
        for r, v in ((0, 0), (0, 1), (3, 0), (4, 0), (5, 0), (6, 1)):
            assert len(np.unique(want[r, v, at])) > 2, f"row {ROW_NAMES[r]} of voice {v} rests in the first vector of block {b}"
    rig = RowsRig(eng, cfg, len(instruments))
    got = np.concatenate([rig.block(instruments, b, fused=(b % 2 == 0) == (first == "graph")) for b in range(N_BLOCKS)], 2)
    rig.close()
    for r in range(7):
        assert_bits_equal(got[r], want[r], True, f"{first} first: row {ROW_NAMES[r]}")


def test_protocol_at_run_time(eng):
    """A graph with the switch on a MIDI object gives the bits of a graph without it on a twin; after configure(mpe=1) and new events,
    those of a fresh MPE twin; then MIDI again. A reserve made before the first switch covers every block, and a block one vector longer
    gets ERR_RANGE with its events intact."""
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Status
    P, N, n_blocks = 5, 6, 2
    # (Every performance starts with an event on frame 0 - controller 1, which nothing follows -: an instrument that has played stays awake
    # through mlgpu_events_set_protocol, as the reference's object does, while a fresh twin wakes with its first event.)
    wake = [(CTRL, 1, 1, 0, 0.0, 0.0)]
    midi = [wake + performance("midi", 100 * k + 10, BLOCK * n_blocks, P) for k in range(N)]
    midi2 = [wake + performance("midi", 100 * k + 11, BLOCK * n_blocks, P) for k in range(N)]
    mpe = [wake + mpe_performance(100 * k + SEED0, BLOCK * n_blocks, P, burst=(k % 3 == 0)) for k in range(N)]
    rig = RowsRig(eng, config(P, 0.3, mpe=0), N, reserve=3)
    twin = RowsRig(eng, config(P, 0.3, mpe=0), N, mpe_events=False)
    assert "CtlVoiceMpe" not in twin.g.source

    def refused_longer_block(b, instruments):
        add_block(rig.ev, instruments, b)
        with pytest.raises(ml.MlgpuError) as ei:
            rig.g.process_events(4, 0, [], rig.d[:7], out_layout=Layout.VOICE_MAJOR)
        assert ei.value.status == Status.ERR_RANGE, str(ei.value)
        out = np.concatenate([rig.launch(T, off) for T, off in LAUNCHES], 2)      # the block's events are still there
        rig.ev.clear_events()
        return out

    a = np.concatenate([refused_longer_block(b, midi) for b in range(n_blocks)], 2)
    b_ = np.concatenate([twin.block(midi, b) for b in range(n_blocks)], 2)
    for r in range(7):
        assert_bits_equal(a[r], b_[r], True, f"MIDI, with the switch vs without: row {ROW_NAMES[r]}")
    want = gpu_run(eng, config(P, 0.3, mpe=0), midi, BLOCK, n_blocks, 3)
    for r in range(7):
        assert_bits_equal(a[r], want[r], True, f"MIDI, with the switch vs mlgpu_events_process: row {ROW_NAMES[r]}")

    rig.ev.configure(mpe=1)
    assert rig.ev.graph_reserve_bytes(3, range(7)) == (16 + 512 + 260 * 4) * 3 * N * 8
    a = np.concatenate([refused_longer_block(b, mpe) for b in range(n_blocks)], 2)
    want = gpu_run(eng, config(P, 0.3), mpe, BLOCK, n_blocks, 3)
    for r in range(7):
        assert_bits_equal(a[r], want[r], True, f"after the switch to MPE: row {ROW_NAMES[r]}")
    assert len(np.unique(want[3])) > 2 and np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0

    rig.ev.configure(mpe=0)
    a = np.concatenate([refused_longer_block(b, midi2) for b in range(n_blocks)], 2)
    want = gpu_run(eng, config(P, 0.3, mpe=0), midi2, BLOCK, n_blocks, 3)
    for r in range(7):
        assert_bits_equal(a[r], want[r], True, f"back to MIDI: row {ROW_NAMES[r]}")
    rig.close()
    twin.close()


def test_mixed_down_output_with_spare_lanes(eng):
    """V = 130: the sum of the seven rows as the mixdown of all voices. The last wavefront's 62 spare lanes run voice 129, its lane and its
    main lane, again; the result is mlgpu_mixdown's sum of the comparator's rows added in the node order."""
    import madronalib_amd as ml
    from cpu_checkers import Oracle
    from madronalib_amd.constants import Layout
    name = "P5_V130"
    cfg, instruments = shape_instruments(name)
    rows = comparator_rows(eng, name)
    s = rows[0]
    for r in range(1, 7):
        s = (s + rows[r]).astype(np.float32)
    want = Oracle().mixdown(np.ascontiguousarray(s), None)
    V = 130
    ev = make_events(eng, cfg, 26)
    desc, outs = seven_rows_desc(with_sum=True)
    g = ml.Graph(eng, V, desc, outs, compile_now=False, mpe_events=True)
    g.set_output_mixdown(0, True)
    g.compile()
    g.clear()
    g.reserve_mixdown(3)
    g.bind_events(ev)
    d = eng.alloc(4 * 64 * 3 + 64)
    chunks = []
    for b in range(N_BLOCKS):
        add_block(ev, instruments, b)
        for T, off in LAUNCHES:
            g.process_events(T, off, [], [d], out_layout=Layout.VOICE_MAJOR)
            chunks.append(d.download(np.float32, 64 * T).copy())
        ev.clear_events()
    g.close()
    ev.close()
    assert_bits_equal(np.concatenate(chunks), want, True, "the mixdown of 130 voices' row sums")
    assert np.abs(want).max() > 0


def test_statuses(eng):
    import madronalib_amd as ml
    from madronalib_amd.constants import Layout, Status
    P, N = 5, 6
    V = N * P
    cfg = config(P, 0.3)
    instruments = [mpe_performance(100 * k + SEED0, BLOCK, P, burst=(k % 3 == 0)) for k in range(N)]

    def refused(status, words, fn, *args, **kw):
        with pytest.raises(ml.MlgpuError) as ei:
            fn(*args, **kw)
        assert ei.value.status == status and all(w in str(ei.value) for w in words), str(ei.value)

    # the bytes of a reserve go by lane: N instruments of G = 8 lanes
    ev = make_events(eng, cfg, N)
    for n in (1, 4):
        assert ev.graph_reserve_bytes(n) == 528 * n * N * 8
        assert ev.graph_reserve_bytes(n, [0, 1, 3, 6]) == (528 + 260 * 2) * n * N * 8
    # without the switch the refusals stay
    g0 = rows_graph(eng, V)
    refused(Status.ERR_UNSUPPORTED, ["MIDI"], g0.bind_events, ev)
    g0.close()
    # the switch is a build call
    g = rows_graph(eng, V, mpe_events=True, voice_lists=True, voice_list_events=True)
    refused(Status.ERR_INVALID, ["graph_enable_mpe_events", "before mlgpu_graph_compile"], g.enable_mpe_events)
    assert "CtlVoiceMpe" not in g.listed_source() and "mlev::CtlVoice ev_0;" in g.listed_source()
    g.bind_events(ev)
    # the listed form under MPE: refused naming MIDI, outputs and state untouched, the next valid call has the comparator's bits
    g.reserve_voice_list(V)
    g.set_voice_list(np.arange(V, dtype=np.uint32))
    guard = np.full(V * 3 * 64, 0x7FC0ABCD, np.uint32)
    d = [eng.alloc(4 * V * 3 * 64) for _ in range(7)]
    for x in d:
        x.upload(guard)
    d_peak = eng.alloc(4 * V)
    add_block(ev, instruments, 0)
    refused(Status.ERR_UNSUPPORTED, ["graph_process_events_listed", "MIDI"], g.process_events_listed, 3, 0, [], d, out_layout=Layout.VOICE_MAJOR, d_peak=d_peak)
    for x in d:
        assert (x.download(np.uint32, V * 3 * 64) == guard).all()
    refused(Status.ERR_UNSUPPORTED, ["MIDI"], ev.sounding_voices)
    want = gpu_run(eng, cfg, instruments, BLOCK, 1, 3)
    got = []
    for T, off in LAUNCHES:
        g.process_events(T, off, [], d, out_layout=Layout.VOICE_MAJOR)
        got.append(np.stack([x.download(np.float32, V * T * 64).reshape(V, T * 64).copy() for x in d]))
    ev.clear_events()
    got = np.concatenate(got, 2)
    for r in range(7):
        assert_bits_equal(got[r], want[r], True, f"after the refused listed call: row {ROW_NAMES[r]}")
    g.close()
    ev.close()
    # a reserve by rows under MPE: a graph with a row outside it is refused and names the row
    ev = make_events(eng, cfg, N)
    ev.reserve_for_graph(4, rows=[0, 1, 6])
    gz = ml.Graph(eng, V, [dict(name="z", type="event_row", kind=3), dict(name="mod", type="event_row", kind=6)], ["z", "mod"], mpe_events=True)
    gz.clear()
    gz.bind_events(ev)
    add_block(ev, instruments, 0)
    refused(Status.ERR_INVALID, ["3 (z)"], gz.process_events, 3, 0, [], d[:2], out_layout=Layout.VOICE_MAJOR)
    ev.route_ahead(3, 0)      # stays legal under MPE for the plain call
    gm = ml.Graph(eng, V, [dict(name="mod", type="event_row", kind=6)], ["mod"], mpe_events=True)
    gm.clear()
    gm.bind_events(ev)
    gm.process_events(3, 0, [], d[:1], out_layout=Layout.VOICE_MAJOR)
    assert_bits_equal(d[0].download(np.float32, V * 3 * 64).reshape(V, 192), want[6][:, :192], True, "the mod row after a refused call and a route ahead")
    gz.close(), gm.close(), ev.close()
